"""What the GPU cases of test_instances_gpu.py rest on, checked without a GPU.

The two output stages (k_demit of the delayed form, k_emit of the general engine), the delayed form's forward pass (k_dforward)
and the backward pass (k_backlen) are families of template instances; the host picks one per shard from the table's size, the
output/input ratio, the constants per piece and kx_config.  test_instances_gpu.py launches every one of them and proves from the
engine's own debug lines which one ran.  Each of its cases needs a fact about a program or about the planner to hold: an image
beyond 16 KiB, a delayed form at K = 2 with more than 31 byte classes, a planner that cannot give whole-piece rounds at 12 or 16
waves, inputs of an exact length.  Those facts are asserted HERE, so that a change to the table builder that moves one of them
fails on any machine and names the GPU case that lost its footing.

The planner of kx_shard_emit (kx_engine.hip) is restated as two pure functions; the GPU file predicts `maxcnt` with them and reads
the same figure from the debug line."""
import random

import numpy as np
import pytest
import kxp
from conftest import blob_of
from test_delayed_form import expect, many_classes_program
from test_dfrec8 import LENGTHS, PIECE, exactly, maxima_programs

from kleenexlang_amd import host, workloads

LDS_CAP = 160 * 1024


# ------------------------------------------------------------------------------------------------------------- the planner
# whole-piece rounds (maxcnt < 64 without half pieces): (program, emit_waves, emit_half)
ROUNDS_CASES = [("iso", 12, 1), ("iso", 8, 0), ("long", 12, 1), ("long", 4, 0), ("long", 8, 0)]


def plan_delayed(tab, W, olen, kper, emit_half=0):
    """kx_shard_emit's delayed-form branch: (maxcnt, stgb, jbytes, halfmode).  tab: the table image's bytes rounded up to 16; W: waves
    per workgroup; olen: output bytes per piece (64 * out_len / n); kper: job slots per piece (plan_kper); emit_half: kx_config's
    (0 auto, 1 off, 2 on)."""
    per_wave = ((LDS_CAP - tab) // W) & ~63

    def plan(ol, kp):
        for R in range(1, 65):
            c = (64 + R - 1) // R
            st = ((int(c * ol * 1.05) + 64) + 63) & ~63
            jb = (int(c * kp + 16) * 4 + 63) & ~63
            st = max(st, 1024)
            if st + 16 + jb <= per_wave or c == 1:
                return c, per_wave - 16 - jb, jb

    maxcnt, stgb, jbytes = plan(olen, kper)
    halfmode = maxcnt <= 32 and W in (12, 16)
    if emit_half:
        halfmode = emit_half == 2 and W in (12, 16)
    if halfmode:
        maxcnt, stgb, jbytes = plan(olen / 2, kper / 2 + 0.5)
    stgb = min(stgb, 49152) & ~15
    return maxcnt, stgb, jbytes, halfmode


def plan_general(per_wave, olen, kper, inplace=False, job_stride=False):
    """The R loop of the general engine's branch: (maxcnt, jbytes).  per_wave: a wave's LDS, ((160 KiB - tables) / W) rounded down to
    256 — the tables' size is not in the blob, the GPU file takes per_wave from the debug line (staging + 16 + job slots)."""
    for R in range(1, 65):
        c = (64 + R - 1) // R
        st = ((int(c * olen * 1.08) + 64) + 255) & ~255
        jb = 0 if inplace else (int(c * kper + 16) * 4 + 255) & ~255
        st = max(st, 1024)
        if job_stride and not inplace:
            jb = (int(c * (kper + 1.0) + 16) * 4 + 255) & ~255
        if st + 16 + jb <= per_wave or c == 1:
            return c, jb


def plan_kper(kavg, kmax, delayed=True):
    """job slots per piece from the constants the device counted: kavg = emit_ksum / emit_kn (negative: nothing counted), kmax the
    largest count of one piece"""
    kmax = min(kmax, 64)
    if kavg < 0:
        return float(kmax + 1)
    k = 1.1 * kavg + 1.0 if delayed else 1.25 * kavg + 1.5
    return min(k, float(kmax + 1))


def test_planner_gives_no_whole_piece_rounds_at_12_or_16_waves():
    """The property the rounds cases rest on: at W of 12 or 16 with emit_half = 0 every plan of fewer than 64 lanes per round is a
    plan of half pieces — whole-piece rounds need emit_half = 1 or W of 4 or 8.  (maxcnt = ceil(64 / R) is 64 or at most 32.)"""
    r = random.Random(1)
    grid = [(tab, olen, kper) for tab in (432, 4096, 8608, 15728, 31424, 40960) for olen in (1, 64, 100, 200, 265, 400, 800, 2000, 8064)
            for kper in (1.0, 2.5, 8.0, 33.0, 65.0)] + [(r.randrange(0, 2560) * 16, r.uniform(0, 8064), r.uniform(1, 65)) for _ in range(3000)]
    seen_rounds = {4: 0, 8: 0, 12: 0, 16: 0}
    for tab, olen, kper in grid:
        for W in (4, 8, 12, 16):
            maxcnt, stgb, jbytes, half = plan_delayed(tab, W, olen, kper)
            assert 1 <= maxcnt <= 64 and stgb % 16 == 0 and stgb <= 49152 and jbytes % 64 == 0
            assert tab + W * (stgb + 16 + jbytes) <= LDS_CAP or maxcnt == 1, "the plan outgrows the CU's LDS"
            if W in (12, 16):
                assert maxcnt == 64 or half, (tab, W, olen, kper, maxcnt)
            else:
                assert not half
            seen_rounds[W] += maxcnt < 64 and not half
            # pinned: off means off, on means on at 12 and 16 only
            assert not plan_delayed(tab, W, olen, kper, emit_half=1)[3]
            assert plan_delayed(tab, W, olen, kper, emit_half=2)[3] == (W in (12, 16))
    assert seen_rounds[4] and seen_rounds[8] and not seen_rounds[12] and not seen_rounds[16]


def test_planner_on_the_figures_the_rounds_cases_use():
    """iso_datetime_to_json (about 265 output bytes and 13 constants per piece, an image of 8 608 bytes) and the `long` program (8 064
    bytes per piece): whole-piece rounds with emit_half = 1 at 12 waves and by themselves at 8 — and, for `long`, at 4.  At 4 waves
    a wave has 38 KiB of LDS and 64 pieces of iso_datetime_to_json (18 KiB of output, 4 KiB of job slots) fit in one round: that
    pair is no rounds case (ROUNDS_CASES leaves it out; the k_demit matrix runs it at maxcnt = 64)."""
    for name, tab, olen, kavg, kmax in (("iso", 8608, 265.0, 13.0, 16), ("long", 880, 8064.0, 64.0, 64)):
        for W, half in ((12, 1), (4, 0), (8, 0)):
            m = plan_delayed(tab, W, olen, plan_kper(kavg, kmax), emit_half=half)
            assert not m[3]
            assert (m[0] < 64) == ((name, W, half) in ROUNDS_CASES), (name, W, m)
    assert plan_delayed(8608, 12, 265.0, plan_kper(13.0, 16))[3]          # by itself: half pieces
    per_wave = ((LDS_CAP - 16384) // 12) & ~255
    assert plan_general(per_wave, 80.0, 5.0)[0] == 64 and plan_general(per_wave, 8064.0, 5.0)[0] == 1
    assert plan_general(per_wave, 80.0, 5.0, inplace=True)[1] == 0
    assert plan_general(per_wave, 80.0, 5.0, job_stride=True)[1] > plan_general(per_wave, 80.0, 5.0)[1]


# ------------------------------------------------------------------------------------------------------------- the programs
def describe(blob, **fields):
    return host.df_describe(blob, cfg=host.config_from_env({}, **fields), with_image=False)[0]


FORWARD_8 = ({"merge_window": 5}, {"merge_window": 9}, {"delay": 1, "merge_window": 9})     # apache_log: images beyond 16 KiB


def forward_stage(image_bytes):
    """records k_dforward stages per lane: kx_shard_forward takes 16 where two workgroups fit one CU's LDS side by side,
    2 * (image + 512 lanes * 16 records * 8 bytes) <= 160 KiB — that is image <= 16 384 bytes — and 8 otherwise"""
    image = (image_bytes + 15) & ~15
    return 16 if 2 * (image + 512 * 16 * 8) <= LDS_CAP else 8


def test_images_that_select_the_8_record_forward_instance():
    blob = blob_of("apache_log")
    assert forward_stage(16384) == 16 and forward_stage(16385) == 8
    d = describe(blob)
    assert d.available == 1 and d.delay == 2 and d.image_bytes <= 16384, "test_forward_16_records... lost its footing"
    for f in FORWARD_8:
        d = describe(blob, **f)
        assert d.available == 1 and d.image_bytes > 16384 and d.delay == f.get("delay", 2), (f, d.image_bytes, "test_forward_8_records lost its footing")
        assert forward_stage(d.image_bytes) == 8
    assert describe(blob, merge_window=9).merge_window == 8 and describe(blob, delay=1, merge_window=9).escapes_start > 0


def wide_k2_program(replaced=4, width=2):
    """many_classes_program with fewer replaced letters: 36 letters, every one a byte class of its own (more than the 31 whose class * 8
    fits the class table's byte), the first `replaced` of them rewritten and the others copied one by one.  With 40 replaced letters
    a second symbol of delay squares the kinds of output that wait in a state and the image hits its cap; with 4 it is about 11 KiB,
    with 8 about 29 KiB (beyond 16 KiB: the 8-record forward instance with a class table of indices)."""
    letters = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJ"
    alts = ['~/%s/ "%s"' % (c, (c.swapcase() + c) * (width // 2)) for c in letters[:replaced]] + ["/%s/" % c for c in letters[replaced:]]
    return "main := (%s | /[0-9 ]/)*\n" % " | ".join(alts), letters


def test_a_wide_program_with_a_delayed_form_at_k2():
    """the wide K = 2 walks (piece_dfwalk2cw_k2, piece_dfwalk1cw_k2) need more than 31 byte classes AND a delayed form at K = 2;
    many_classes_program has none (too many contexts)"""
    for width in (2, 8):
        assert describe(blob_of(many_classes_program(width)[0]), delay=2).available == 0
    for replaced, width in ((4, 2), (4, 8), (8, 2)):
        blob = blob_of(wide_k2_program(replaced, width)[0])
        assert kxp.parse(blob)[0].nclasses > 31
        d = describe(blob, delay=2)
        assert d.available == 1 and d.delay == 2 and d.escapes_start == 0 and d.escapes == 0, (replaced, width, d.reason)
        assert (d.image_bytes > 16384) == (replaced == 8), (replaced, d.image_bytes)
    r = random.Random(2)
    src, letters = wide_k2_program()
    data = bytes(r.choice((letters + "0123456789 ").encode()) for _ in range(300))
    want = expect(blob_of(src), data)
    assert len(want) == len(data) + sum(data.count(c.encode()) for c in letters[:4])


def max_constant(blob):
    return int(np.diff(kxp.parse(blob)[0].pconst_off).max())


# the delayed-form programs of the k_demit matrix: (name, source or workload, pinned delay or 0, delay it runs at, input shape)
DEMIT_PROGRAMS = [("csv2json", "csv2json", 0, 1, "csv"), ("csv2json_k2", "csv2json", 2, 2, "csv"), ("apache_log", "apache_log", 0, 2, "apache_log"),
                  ("iso", "iso_datetime_to_json", 0, 1, "datetime"), ("iso_k2", "iso_datetime_to_json", 2, 2, "datetime")]


def test_delays_of_the_demit_matrix():
    for name, prog, pin, K, _ in DEMIT_PROGRAMS:
        d = describe(blob_of(prog), **({"delay": pin} if pin else {}))
        assert d.available == 1 and d.delay == K, (name, d.delay, d.reason)
        assert d.escapes_start == 0 or prog == "apache_log"      # (apache_log: contexts of escaped quotes, none in the clean logs)
    for name, src in maxima_programs().items():
        assert describe(blob_of(src)).delay == 1


def test_constants_of_at_most_16_bytes_where_the_store_sequence_is_switched():
    """KX_OFF_CMPX changes the constant stores of k_emit (the general engine), and only for a stage whose longest constant is at most
    16 bytes (DevTables::short_consts): the programs of test_general_engine_switches.  csv2json's longest is 21 bytes.  The delayed
    form's kernels read no such flag: there the switch is accepted and changes nothing."""
    assert max_constant(blob_of("csv2json")) > 16
    for prog in ("apache_log", INLINE_PROGRAM, "iso_datetime_to_json"):
        assert max_constant(blob_of(prog)) <= 16, prog[:40]
    assert kxp.parse(blob_of("iso_datetime_to_json"))[0].nclasses <= 31 and kxp.parse(blob_of("csv2json"))[0].nclasses <= 31


# ------------------------------------------------------------------------------------- the general engine's four layouts
INLINE_PROGRAM = 'main := (/[a-d]/ "1" | /[e-h]/ "\\xfe" | ~/,/ ";" | /\\n/ "<end of line>\\n")*\n'      # (test_inline_constant_layout's first)
CLASSES_PROGRAM = "main := (%s | ~/ /)*\n" % " | ".join('/%s/ "%d;"' % (("\\x%02x" % b), b) for b in range(33, 127))   # (more than 64 byte classes)
LEAVES_PROGRAM = "main := /(a?){32}a{32}\\n/"                                                                # (test_many_simultaneous_paths: 34 leaves)
WIDE_ENTRY_PROGRAM = 'main := (~/a/ "%s" | /b/ | ~/c/ "<%s>")*\n' % ("x" * 300, "y" * 130)                    # (constants of 127 bytes and more)
# (a general-layout stage of more than 32 leaves: CLASSES_PROGRAM has 96 of them, one per alternative.  Putting /(a?){32}a{32}/ in front
#  of its loop gives 128 leaves, but a blob of 1.7 MB that takes minutes to compile: no program for a quick test.)


def layout_facts(blob):
    """what chooseLayout (kx_stage.h) decides a stage's layout from: byte classes, the most leaves of a state, path entries that
    append one byte / more than one, the longest constant + copied byte of an entry"""
    st = kxp.parse(blob)[0]
    back = st.back.ravel()
    live = back[back != 0xFFFFFFFF]
    cl = np.diff(st.pconst_off).astype(np.int64)[live >> 9]
    widest = int((cl + ((live >> 8) & 1)).max()) if len(live) else 0
    return {"C": st.nclasses, "Lm": st.maxleaves, "one": int((cl == 1).sum()), "longer": int((cl > 1).sum()), "widest": widest,
            "tables": st.tables is not None}


def layout_kind(blob, inline_consts=0, job_stride=0):
    """'inline', 'job-stride', 'general' or 'plain': the k_emit / k_backlen instance family of a stage of small tables.  A restatement of
    chooseLayout's choice (kx_stage.h) for the programs used here, not all of it: symbol tables (xlat), tables beyond LDS addressing
    (big), KX_FORCE_BIG and the count of distinct constants are left out — none of these programs has them.  The engine's debug line
    names only the job-stride layout; test_the_restated_layout_meets_the_engines holds this function to the engine's own decision."""
    f = layout_facts(blob)
    small = f["C"] <= 64 and f["Lm"] <= 64 and f["widest"] < 127 and not f["tables"]
    if small and (inline_consts == 2 if inline_consts else f["one"] > 0 and f["one"] >= f["longer"]):
        return "inline"
    if small and job_stride == 2:
        return "job-stride"
    return "general" if f["C"] > 64 or f["widest"] >= 127 else "plain"


def test_layouts_and_leaf_counts_of_the_general_engine_cases():
    """k_emit<W, WIDE, EXT, JL>: plain, inline constants, general, job-stride; k_backlen<32 | 256 leaves, …>: the same families at a
    leaf count of at most 32 / more"""
    kinds = {"apache_log": ("plain", 0, 0), INLINE_PROGRAM: ("inline", 0, 0), CLASSES_PROGRAM: ("general", 0, 0), WIDE_ENTRY_PROGRAM: ("general", 0, 0),
             "iso_datetime_to_json": ("plain", 0, 0), LEAVES_PROGRAM: ("plain", 0, 0)}
    for prog, (kind, inl, jl) in kinds.items():
        assert layout_kind(blob_of(prog), inl, jl) == kind, prog[:40]
    assert layout_kind(blob_of("iso_datetime_to_json"), job_stride=2) == "job-stride"
    assert layout_kind(blob_of(LEAVES_PROGRAM), job_stride=2) == "job-stride"
    assert layout_kind(blob_of("apache_log"), inline_consts=1) == "plain" and layout_kind(blob_of(INLINE_PROGRAM), inline_consts=1) == "plain"
    leaves = {p: layout_facts(blob_of(p))["Lm"] for p in kinds}
    assert leaves["apache_log"] <= 32 and leaves[INLINE_PROGRAM] <= 32 and leaves["iso_datetime_to_json"] <= 32 and leaves[WIDE_ENTRY_PROGRAM] <= 32
    assert 32 < leaves[LEAVES_PROGRAM] <= 64
    assert leaves[CLASSES_PROGRAM] > 32 and layout_facts(blob_of(CLASSES_PROGRAM))["C"] > 64
    # (the job-stride layout keeps every constant within the first 64 pool slots of 16 bytes)
    for p in ("iso_datetime_to_json", LEAVES_PROGRAM):
        st = kxp.parse(blob_of(p))[0]
        assert sum((int(c) + 15) // 16 for c in np.diff(st.pconst_off)) <= 64


def engine_layout_kind(blob, inline_consts=0, job_stride=0):
    """layout_kind's answer as the engine's loader gives it (kx_stage_describe_cfg: no device needed)"""
    info, _ = host.stage_describe(blob, cfg=host.KxConfig(inline_consts=inline_consts, job_stride=job_stride), with_image=False)
    return "inline" if info.t.inl else "job-stride" if info.t.jl else "general" if info.general else "plain"


def test_the_restated_layout_meets_the_engines():
    """every program and switch of test_layouts_and_leaf_counts_of_the_general_engine_cases, and the whole grid of the two switches"""
    for prog in ("apache_log", INLINE_PROGRAM, CLASSES_PROGRAM, WIDE_ENTRY_PROGRAM, "iso_datetime_to_json", LEAVES_PROGRAM):
        for inl in (0, 1, 2):
            for jl in (0, 1, 2):
                assert layout_kind(blob_of(prog), inl, jl) == engine_layout_kind(blob_of(prog), inl, jl), (prog[:40], inl, jl)
        info, _ = host.stage_describe(blob_of(prog), cfg=host.KxConfig(), with_image=False)
        assert info.t.maxleaves == layout_facts(blob_of(prog))["Lm"] and info.t.nclasses == layout_facts(blob_of(prog))["C"]


# --------------------------------------------------------------------------------------------------------------- the inputs
def exactly_datetime(n, seed):
    """n bytes of whole datetime lines (a line is 21 bytes with the zone Z and 26 with an offset: every n from 500 on is a sum of
    those, and many below); where n is no such sum, the first n bytes of some lines — the engine then has to reject it where the
    oracle does"""
    lines = workloads.generate("datetime", 26 * (n // 21 + 2) * 4 + 4096, seed).split(b"\n")[:-1]
    short = [ln + b"\n" for ln in lines if len(ln) == 20]
    long_ = [ln + b"\n" for ln in lines if len(ln) == 25]
    for b in range(n // 26 + 1):
        if (n - 26 * b) % 21 == 0:
            a = (n - 26 * b) // 21
            if a <= len(short) and b <= len(long_):
                picked = short[:a] + long_[:b]
                random.Random(seed).shuffle(picked)
                return b"".join(picked)
    return b"\n".join(lines)[:n]


def exact_input(shape, n, seed):
    """n bytes of the shape: whole lines where the shape has lines, letters for the programs that take any"""
    if shape == "datetime":
        return exactly_datetime(n, seed)
    if shape in ("apache_log", "csv"):
        return exactly(shape, n, seed)
    r = random.Random(seed * 1000003 + n)
    return bytes(r.choice(shape.encode()) for _ in range(n))      # (an alphabet)


def tiled_input(shape, n, seed):
    """n bytes for the persistent loop's second trip: a block of 64 KiB of whole lines over and over, the rest as exact_input"""
    block = workloads.generate(shape, 65536, seed) if shape in ("apache_log", "csv", "datetime") else exact_input(shape, 65536, seed)
    k = max(0, (n - 8192) // len(block))
    return block * k + exact_input(shape, n - k * len(block), seed + 1)


ROUND_LENGTHS = (64, 65, 4097, 64 * 64 * 2 + 17)          # the thinned lengths (a case that crosses many switches)
GENERAL_LENGTHS = (1, 63, 64, 65, 4097, 70000)


def test_inputs_have_the_length_asked_for_and_end_in_a_whole_line():
    for n in LENGTHS + GENERAL_LENGTHS + (64 * 22, 64 * 21, 64 * 23):
        for shape in ("apache_log", "csv", "datetime"):
            d = exact_input(shape, n, 100 + n)
            assert len(d) == n, (shape, n)
            if n >= 500:
                assert d.endswith(b"\n"), (shape, n)
        assert len(exact_input("abcdefgh,\n", n, 7)) == n
    # datetime: 63 = 3 * 21 is whole lines, 64 and 65 are no sum of 21s and 26s
    blob = blob_of("iso_datetime_to_json")
    assert not isinstance(expect(blob, exact_input("datetime", 63, 5)), tuple)
    assert isinstance(expect(blob, exact_input("datetime", 64, 5)), tuple)
    for n in (2047, 2048, 2049, 4096 * 3 + 1):
        assert not isinstance(expect(blob, exact_input("datetime", n, 5)), tuple), n
    for shape, prog in (("apache_log", "apache_log"), ("csv", "csv2json"), ("datetime", "iso_datetime_to_json")):
        n = 256 * 4 * 4096 + 3 * 4096 + 1
        d = tiled_input(shape, n, 9)
        assert len(d) == n and d.endswith(b"\n") and n % PIECE == 1
        assert not isinstance(expect(blob_of(prog), d), tuple), prog


@pytest.mark.parametrize("where", [0, 7, 8, 15, 16, 31])
def test_contexts_land_in_the_pieces_the_group_cases_name(where):
    """with_context_at puts the undecided context (the backslash) where asked, modulo 32 pieces; the oracle accepts the input"""
    from test_dfrec8 import with_context_at
    lines = workloads.generate("apache_log", 200 * 1024, 17).split(b"\n")[:-1]
    d = with_context_at(lines, len(lines) // 2, where * PIECE + 20)
    assert (d.index(b'\\"') // PIECE) % 32 == where
    assert not isinstance(expect(blob_of("apache_log"), d), tuple)
