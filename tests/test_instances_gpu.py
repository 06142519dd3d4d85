"""Every compiled instance of the output-stage kernels, of the delayed form's forward pass and of the backward pass, against the oracle.

k_demit<W, K, HALF> (12 instances), k_emit<W, WIDE, EXT, JL> (12), k_dforward<512, 16 | 8, 4, SLOW> (4) and k_backlen<32 | 256, …> (6)
are picked per shard by the host: from the table's size, the output/input ratio, the constants per piece and kx_config.  With the
shipped programs and the other tests' inputs the planners land on a few of them; here kx_config steers them to each one, and each
case PROVES which instance ran from the lines the library prints under KX_DEBUG:

  [kx] emit (delayed form, K=…, … image … B)[, a lane = half a piece]: W=… stg=… jobs=… maxcnt=… … overflow=… of … pieces
  [kx] emit: layout=… next=… [kx] emit: W=… stg=… jobs=… maxcnt=… …                                  (jobs=0: the in-place sweep)
  [kx] forward (delayed form): ST=… SLOW=… image … B

and from the blob (byte classes, leaves, constants: test_instances.py, which also holds every precondition, checked without a
GPU).  `maxcnt` is predicted by the restated planner of test_instances.py from the same line's figures.  Every output — or
("fail", pos) — is compared byte for byte with the CPU oracle.  The switches that print nothing (KX_OFF_CMPX and KX_OFF_DIRECT on the
general engine, block_threads) are proven only by the configuration the engine accepted; whether a k_emit instance is the plain, the
inline or the general one, and which k_backlen instance ran, follows from test_instances.layout_kind, a restatement of parseStage
for small tables — the line names only the job-stride layout."""
import random
import re

import pytest
import test_instances as ti
from conftest import blob_of
from test_delayed_form import expect, many_classes_program
from test_dfrec8 import LENGTHS, PIECE, SEGMENTS, maxima_programs, with_context_at

from kleenexlang_amd import MatchError, Program, host, workloads

pytestmark = pytest.mark.gpu

_TAIL = r"W=(\d+) stg=(\d+) jobs=(\d+) maxcnt=(\d+) kmax=(\d+) kavg=(-?[\d.]+) olen=([\d.]+) overflow=(\d+) of (\d+) pieces"
_DEMIT = re.compile(r"\[kx\] emit \(delayed form, K=(\d+), (\d+) product states, image (\d+) B\)(, a lane = half a piece)?: " + _TAIL)
_EMIT = re.compile(r"\[kx\] emit: layout=(\S+) next=(.*?) \[kx\] emit: " + _TAIL)
_FORWARD = re.compile(r"\[kx\] forward \(delayed form\): ST=(\d+) SLOW=(\d+) image (\d+) B")
_TAIL_KEYS = ("W", "stg", "jobs", "maxcnt", "kmax", "kavg", "olen", "overflow", "pieces")


def _tail(groups):
    return {k: (float(v) if k in ("kavg", "olen") else int(v)) for k, v in zip(_TAIL_KEYS, groups)}


def demit_lines(err):
    return [dict(_tail(m.groups()[4:]), K=int(m.group(1)), image=int(m.group(3)), half=m.group(4) is not None) for m in _DEMIT.finditer(err)]


def emit_lines(err):
    return [dict(_tail(m.groups()[2:]), layout=m.group(1), next=m.group(2)) for m in _EMIT.finditer(err)]


def forward_lines(err):
    return [(int(m.group(1)), int(m.group(2))) for m in _FORWARD.finditer(err)]


@pytest.fixture
def log(monkeypatch, capfd):
    """run(program, data) -> (output or ("fail", pos), what the library printed)"""
    monkeypatch.setenv("KX_DEBUG", "1")

    def run(p, data):
        capfd.readouterr()
        try:
            got = p.run_host(data)
        except MatchError as e:
            got = ("fail", e.pos)
        return got, capfd.readouterr().err
    return run


def load(prog, env=None, **fields):
    """load-time fields go through the configuration the program is loaded with"""
    return Program(blob_of(prog), config=host.config_from_env(env or {}, **fields))


def predicted_maxcnt(line, data, want, emit_half):
    """the planner's maxcnt for a delayed-form run, from the figures of its own debug line (kavg is printed with two decimals: where
    that rounding decides, both neighbours count)"""
    tab = (line["image"] + 15) & ~15
    olen = 64.0 * len(want) / len(data)
    return {ti.plan_delayed(tab, line["W"], olen, ti.plan_kper(k, line["kmax"]), emit_half)[0]
            for k in ((line["kavg"],) if line["kavg"] < 0 else (line["kavg"] - 0.005, line["kavg"], line["kavg"] + 0.005))}


def predicted_general(line, data, want):
    """the general engine's (maxcnt, job-slot bytes) from the figures of its own debug line: a wave's LDS is what the line's staging and
    job slots add up to (the planner gives staging all that the slots leave)"""
    per_wave = line["stg"] + 16 + line["jobs"]
    assert per_wave % 256 == 0 and line["stg"] < 49152, line
    olen = 64.0 * len(want) / len(data)
    return {ti.plan_general(per_wave, olen, ti.plan_kper(k, line["kmax"], delayed=False), line["jobs"] == 0, line["layout"] == "job-stride")
            for k in ((line["kavg"],) if line["kavg"] < 0 else (line["kavg"] - 0.005, line["kavg"], line["kavg"] + 0.005))}


def sweep_delayed(log, prog, load_fields, run_fields, datas, segments, K, W, half, verify=None):
    """one program, loaded once: every input at every segment size on the delayed form, the instance proven for every accepted run"""
    blob = blob_of(prog)
    wants = [expect(blob, d) for d in datas]
    assert any(isinstance(w, bytes) and w for w in wants), "no accepted input: the case proves nothing"
    p = load(prog, **load_fields)
    try:
        for seg in segments:
            p.configure(segment_bytes=seg, **run_fields)
            for d, want in zip(datas, wants):
                got, err = log(p, d)
                assert got == want, (seg, len(d), err[-400:])
                if isinstance(want, bytes) and len(d):
                    assert p.stage_delayed_form(0) == 1, (seg, len(d), "the run left the delayed form", err[-400:])
                    lines = demit_lines(err)
                    assert len(lines) == 1 and not emit_lines(err), err[-400:]
                    ln = lines[0]
                    assert (ln["K"], ln["W"], ln["half"]) == (K, W, half), (seg, len(d), ln)
                    assert ln["pieces"] == (len(d) + PIECE - 1) // PIECE
                    assert ln["maxcnt"] in predicted_maxcnt(ln, d, want, run_fields.get("emit_half", 0)), (seg, len(d), ln)
                    if verify:
                        verify(ln, d, seg)
                p.reset_delayed_form(0)
    finally:
        p.close()


def sweep_general(log, prog, env, load_fields, run_fields, datas, segments, verify):
    """the same on the general engine (the stage has no delayed form, or KX_DF=0): verify(line, data, segment, run number)"""
    blob = blob_of(prog)
    wants = [expect(blob, d) for d in datas]
    assert any(isinstance(w, bytes) and w for w in wants), "no accepted input: the case proves nothing"
    p = load(prog, env, **load_fields)
    runs = 0
    try:
        for seg in segments:
            p.configure(segment_bytes=seg, **run_fields)
            for d, want in zip(datas, wants):
                got, err = log(p, d)
                assert got == want, (seg, len(d), err[-400:])
                assert p.stage_delayed_form(0) == 0 and not demit_lines(err)
                if isinstance(want, bytes) and len(d):
                    lines = emit_lines(err)
                    assert len(lines) == 1, err[-400:]
                    ln = lines[0]
                    assert ln["pieces"] == (len(d) + PIECE - 1) // PIECE
                    assert (ln["maxcnt"], ln["jobs"]) in predicted_general(ln, d, want), (seg, len(d), ln)
                    verify(ln, d, seg, runs)
                    runs += 1
    finally:
        p.close()
    assert runs


# ------------------------------------------------------------------------------------------- A. k_demit, all 12 instances
DEMIT_MODES = [(4, 1, False), (8, 1, False), (12, 1, False), (16, 1, False), (12, 2, True), (16, 2, True)]     # (emit_waves, emit_half, half pieces)


@pytest.mark.parametrize("W,emit_half,half", DEMIT_MODES, ids=["w4", "w8", "w12", "w16", "w12_half", "w16_half"])
@pytest.mark.parametrize("name,prog,pin,K,shape", ti.DEMIT_PROGRAMS, ids=[c[0] for c in ti.DEMIT_PROGRAMS])
def test_demit_instance(log, name, prog, pin, K, shape, W, emit_half, half):
    """k_demit<W, K, HALF> for W in 4, 8, 12, 16 whole pieces and 12, 16 half pieces, K in 1, 2 — on csv2json (K = 1 by itself, 2
    pinned), apache_log (2) and iso_datetime_to_json (1, 2 pinned).  emit_half is pinned both ways: iso_datetime_to_json takes half
    pieces by itself at 12 and 16 waves, the others never."""
    datas = [ti.exact_input(shape, n, 100 + n) for n in LENGTHS]
    sweep_delayed(log, prog, {"delay": pin}, {"emit_waves": W, "emit_half": emit_half}, datas, SEGMENTS, K, W, half)


# ------------------------------------------------------------------------------------------------ B. whole-piece rounds
ROUNDS_PROGRAMS = {"iso": ("iso_datetime_to_json", "datetime"), "long": (maxima_programs()["long"], "abcdefghijklmnopqrstuvwxyz")}


@pytest.mark.parametrize("name,W,emit_half", ti.ROUNDS_CASES, ids=["%s_w%d" % (c[0], c[1]) for c in ti.ROUNDS_CASES])
def test_whole_piece_rounds(log, name, W, emit_half):
    """A wave-iteration of whole pieces covered in R > 1 rounds (maxcnt < 64, first > 0): a round's output base is the wave's prefix
    sum read at its first lane.  Reachable only with emit_half = 1 at 12 waves or at 4 / 8 waves (test_instances.py: the planner's
    arithmetic; iso_datetime_to_json at 4 waves fits in one round and is no such case).  The lengths add 64 * maxcnt bytes and one
    piece less / more: a round that ends on, before and behind a lane boundary."""
    prog, shape = ROUNDS_PROGRAMS[name]
    blob = blob_of(prog)
    probe = ti.exact_input(shape, 4097, 3)
    p = load(prog)
    try:
        p.configure(emit_waves=W, emit_half=emit_half)
        got, err = log(p, probe)
        assert got == expect(blob, probe), err[-400:]
        M = demit_lines(err)[0]["maxcnt"]
    finally:
        p.close()
    assert M < 64, M
    lengths = LENGTHS + tuple(n for n in (64 * M - 64, 64 * M, 64 * M + 64) if n > 0)
    datas = [ti.exact_input(shape, n, 200 + n) for n in lengths]

    def verify(ln, d, seg):
        assert ln["maxcnt"] < 64, (seg, len(d), ln)

    sweep_delayed(log, prog, {}, {"emit_waves": W, "emit_half": emit_half}, datas, SEGMENTS, 1, W, False, verify)


BURSTS_PROGRAM = 'main := (/[a-m]/ "ab" | /[n-z]/)*\n'


def test_job_slots_overflow_at_16_waves(log):
    """Rounds whose constants outgrow their job slots copy them in place.  The slots are dimensioned by the AVERAGE constants per
    piece that the forward pass counted: an input of 8 KiB without a constant and then 4 KiB with one on every symbol, over and
    over, has wave-iterations of 4 096 constants against slots for about a third — overflow > 0, the output must still match.  In whole
    pieces and in half pieces (pinned: which of them the planner takes by itself depends on the lanes it sampled)."""
    r = random.Random(4)
    unit = bytes(r.choice(b"nopqrstuvwxyz") for _ in range(8192)) + bytes(r.choice(b"abcdefghijklm") for _ in range(4096))
    datas = [unit * 10, unit * 3 + unit[:4097]]
    seen = []

    def verify(ln, d, seg):
        assert ln["jobs"] > 0
        seen.append(ln["overflow"])

    for emit_half, half in ((1, False), (2, True)):
        seen.clear()
        sweep_delayed(log, BURSTS_PROGRAM, {}, {"emit_waves": 16, "emit_half": emit_half}, datas, SEGMENTS, 1, 16, half, verify)
        assert len(seen) == 6 and all(o > 0 for o in seen), (emit_half, seen)


def test_constant_on_every_step_at_16_waves(log):
    """`short`: 32 constants in each half of every piece, at 16 waves (the least LDS per wave): half pieces by itself.  Every piece
    holds as many constants as the average, so the slots suffice (overflow = 0 here: the planner adds a tenth to the average)."""
    r = random.Random(3)
    datas = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(n)) for n in LENGTHS]

    def verify(ln, d, seg):
        assert ln["overflow"] == 0 and ln["jobs"] > 0, (seg, len(d), ln)

    sweep_delayed(log, maxima_programs()["short"], {}, {"emit_waves": 16}, datas, SEGMENTS, 1, 16, True, verify)


# ------------------------------------------------------------------------------------------------------ C. all eight walks
WIDE_ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJ0123456789 "
WALKS = [  # (id, program, pinned delay, K, input shape, half pieces, more than 31 byte classes)
    ("2c_k1", "csv2json", 0, 1, "csv", False, False), ("1c_k1", "csv2json", 0, 1, "csv", True, False),
    ("2c_k2", "csv2json", 2, 2, "csv", False, False), ("1c_k2", "csv2json", 2, 2, "csv", True, False),
    ("2c_k1_iso", "iso_datetime_to_json", 0, 1, "datetime", False, False), ("1c_k1_iso", "iso_datetime_to_json", 0, 1, "datetime", True, False),
    ("2c_k2_iso", "iso_datetime_to_json", 2, 2, "datetime", False, False), ("1c_k2_iso", "iso_datetime_to_json", 2, 2, "datetime", True, False),
    ("2cw_k1", many_classes_program(2)[0], 0, 1, WIDE_ALPHABET, False, True), ("1cw_k1", many_classes_program(8)[0], 0, 1, WIDE_ALPHABET, True, True),
    ("2cw_k2", ti.wide_k2_program()[0], 2, 2, WIDE_ALPHABET, False, True), ("1cw_k2", ti.wide_k2_program(4, 8)[0], 2, 2, WIDE_ALPHABET, True, True)]


def fused_walk(ln, d, seg):
    """the fused walk runs where the round's jobs fit their slots: job slots at all, and — at the engine's own segment size, on an
    input of a whole piece or more — no round that overflowed them"""
    assert ln["jobs"] > 0, (seg, len(d), ln)
    if seg == 0 and len(d) >= PIECE:
        assert ln["overflow"] == 0, (len(d), ln)


@pytest.mark.parametrize("walk,prog,pin,K,shape,half,wide", WALKS, ids=[w[0] for w in WALKS])
def test_walk_sequence(log, walk, prog, pin, K, shape, half, wide):
    """The hand-scheduled sequences piece_dfwalk{2,1}c{,w}_k{1,2}: two chains (a whole piece) or one (half a piece), a class table of
    class * 8 or of indices (more than 31 byte classes), K of 1 or 2."""
    import kxp
    assert (kxp.parse(blob_of(prog))[0].nclasses > 31) == wide
    datas = [ti.exact_input(shape, n, 300 + n) for n in LENGTHS]
    sweep_delayed(log, prog, {"delay": pin}, {"emit_waves": 12, "emit_half": 2 if half else 1}, datas, SEGMENTS, K, 12, half, fused_walk)


def test_cmpx_switch_is_accepted_and_changes_nothing_in_the_delayed_form(log):
    """KX_OFF_CMPX selects the other store sequence of k_emit's constants phase (DevTables::short_consts).  The delayed form's table
    carries the same flag (DfDev::short_consts), but no kernel of the delayed form reads it: k_demit's constants phase has one store
    sequence.  One run with the switch set: the configuration is accepted and the bytes are the oracle's — no other device code ran.
    (The general engine's cases are in test_general_engine_switches.)"""
    datas = [ti.exact_input("datetime", n, 300 + n) for n in ti.ROUND_LENGTHS]
    sweep_delayed(log, "iso_datetime_to_json", {"disable": host.KX_OFF_CMPX}, {"emit_waves": 12, "emit_half": 1}, datas, SEGMENTS, 1, 12, False, fused_walk)


# ---------------------------------------------------------------------------------------- D. k_dforward, 8 staged records
def forward_sweep(log, prog, load_fields, datas, segments, stage, on_form=True):
    """every input on one program; every forward pass the library reports ran k_dforward<512, stage, 4, false> (on_form=False: or the
    slow instance behind it, where few enough lanes met an undecided context).  Returns (segment size, state, forward passes) of the
    accepted runs."""
    blob = blob_of(prog)
    info = ti.describe(blob, **load_fields)
    # kx_shard_forward: 16 staged records where 2 * (image + 512 * 16 * 8) <= 160 KiB, i.e. image <= 16 384 bytes; 8 otherwise
    assert ti.forward_stage(info.image_bytes) == stage and (info.image_bytes > 16384) == (stage == 8)
    wants = [expect(blob, d) for d in datas]
    p = load(prog, **load_fields)
    states = []
    try:
        for seg in segments:
            p.configure(segment_bytes=seg)
            for d, want in zip(datas, wants):
                got, err = log(p, d)
                assert got == want, (seg, len(d), err[-400:])
                fw = forward_lines(err)
                assert fw in ([(stage, 0)], [(stage, 0), (stage, 1)][:1 if on_form else 2]), (seg, len(d), fw)
                if isinstance(want, bytes):
                    states.append((seg, p.stage_delayed_form(0), fw))
                    if on_form:
                        assert states[-1][1] == 1 and demit_lines(err)[0]["image"] == info.image_bytes, (seg, len(d), err[-400:])
                p.reset_delayed_form(0)
    finally:
        p.close()
    return states


@pytest.mark.parametrize("fields", ti.FORWARD_8[:2], ids=["window5", "window9"])
def test_forward_8_records_plain_instance(log, fields):
    """apache_log with a pinned merge window: a table image of 21 / 31 KiB, K = 2, a narrow class table — 8 staged records per
    lane, half-line cooperative flushes (RPL == 1), on clean logs"""
    forward_sweep(log, "apache_log", fields, [ti.exact_input("apache_log", n, 100 + n) for n in LENGTHS], SEGMENTS, 8)


def test_forward_16_records_is_the_default(log):
    forward_sweep(log, "apache_log", {}, [ti.exact_input("apache_log", n, 100 + n) for n in ti.ROUND_LENGTHS], SEGMENTS, 16)


def test_forward_8_records_with_a_class_table_of_indices(log):
    """more than 31 byte classes, K = 2 and an image of 29 KiB"""
    prog = ti.wide_k2_program(8)[0]
    datas = [ti.exact_input(WIDE_ALPHABET, n, 7) for n in LENGTHS]
    forward_sweep(log, prog, {"delay": 2}, datas, SEGMENTS, 8)


def test_forward_8_records_when_the_form_is_given_up(log):
    """delay = 1 with a merge window of 9: 17 KiB, and every line holds a context that one symbol does not decide.  The shard falls back
    and the stage backs off (2) or gives the form up (3), as in test_engine_runs_the_delayed_form_and_agrees_with_the_general_engine —
    at the engine's own segment size always.  In segments of one piece few enough lanes may meet such a context for the stage to arm its
    slow path instead: a run that stays on the form (1) is one whose second forward pass ran the slow instance of 8 records.  Whichever
    way: the oracle's bytes at this image size."""
    datas = [ti.exact_input("apache_log", n, 100 + n) for n in LENGTHS]
    states = forward_sweep(log, "apache_log", ti.FORWARD_8[2], datas, SEGMENTS, 8, on_form=False)
    assert [st for seg, st, fw in states if seg == 0]
    for seg, st, fw in states:
        if seg == 0 or st != 1:
            assert st in (2, 3), states
        else:
            assert fw == [(8, 0), (8, 1)], states


HOLE_PIECES = (0, 7, 8, 15, 16, 31)      # the stretch's first piece, modulo 32: begins / ends a group of 8 records, begins the second half of one of 16


@pytest.mark.parametrize("fields", [{}] + list(ti.FORWARD_8[:2]), ids=["default_16", "window5", "window9"])
def test_forward_slow_instance(log, fields):
    """k_dforward<512, 8 | 16, 4, true>: an undecided context (an escaped quote) arms the slow path, the forward pass runs again on the
    slow instance and resolves the stretch in place (hole records).  The inputs of test_holes_on_and_next_to_a_base_word, and stretches
    whose first piece has index 0, 7, 8 (mod 16): a hole that begins a group of 8 records, ends one, and begins the second half of
    what would be a group of 16."""
    blob = blob_of("apache_log")
    stage = 8 if fields else 16
    assert ti.forward_stage(ti.describe(blob, **fields).image_bytes) == stage
    lines = workloads.generate("apache_log", 200 * 1024, 17).split(b"\n")[:-1]
    k = len(lines) // 2
    datas = [with_context_at(lines, k, w * PIECE + 20) for w in HOLE_PIECES] + \
            [with_context_at(lines, len(lines) - 1, 20), with_context_at(lines, len(lines) - 1, 31 * PIECE + 20)]
    wants = [expect(blob, d) for d in datas]
    assert not any(isinstance(w, tuple) for w in wants)
    p = load("apache_log", **fields)
    try:
        p.configure(segment_bytes=4096)      # (50 segments: a stage arms its slow path only where few lanes met such a context)
        for d, want in zip(datas, wants):
            got, err = log(p, d)
            assert got == want, (len(d), err[-600:])
            assert p.stage_delayed_form(0) == 1, "the shard fell back instead of resolving the stretch: " + err[-600:]
            assert "arms the slow path of its forward pass" in err
            m = re.search(r"the slow path resolved (\d+) input symbols in place", err)
            assert m and int(m.group(1)) > 0, err[-600:]
            assert forward_lines(err) == [(stage, 0), (stage, 1)], err[-600:]
            p.reset_delayed_form(0)          # (the stage would stay on the slow instance: every input arms it afresh)
        # an armed stage stays on the slow instance, on clean input too
        got, err = log(p, datas[0])
        assert got == wants[0] and forward_lines(err) == [(stage, 0), (stage, 1)], err[-600:]
        got, err = log(p, b"\n".join(lines) + b"\n")
        assert got == expect(blob, b"\n".join(lines) + b"\n") and forward_lines(err) == [(stage, 1)], err[-600:]
    finally:
        p.close()


# ---------------------------------------------------------------------------- E. the second trip of the persistent loop
def second_trip_length(W, half):
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return ncu, ncu * W * (2048 if half else 4096) + 3 * 4096 + 1


@pytest.mark.parametrize("prog,shape,K,W,emit_half,half", [("csv2json", "csv", 1, 4, 0, False), ("apache_log", "apache_log", 2, 8, 0, False),
                                                          ("iso_datetime_to_json", "datetime", 1, 16, 0, True), ("apache_log", "apache_log", 2, 12, 0, False)],
                         ids=["csv2json_w4", "apache_log_w8", "iso_w16_half", "apache_log_w12_partial_last_piece"])
def test_demit_second_trip(log, prog, shape, K, W, emit_half, half):
    """`it += gridDim.x * WAVES` and the hand-over of the prefetched operands (cur = nx): an input of CUs * W wave-iterations and
    three more, so that a few waves take a second iteration and most do not.  Its last piece is one byte: that lane writes straight
    to global memory, and the input's last iteration ends on the `!taken` path (with nothing behind it: the case below has an
    iteration that ends so and is followed by another of the same wave)."""
    ncu, n = second_trip_length(W, half)
    data = ti.tiled_input(shape, n, 11)
    assert len(data) == n and n % PIECE == 1

    def verify(ln, d, seg):
        nwi = ((ln["pieces"] * (2 if half else 1)) + 63) // 64
        assert ncu * W < nwi < 2 * ncu * W, (ncu, W, nwi)

    sweep_delayed(log, prog, {}, {"emit_waves": W, "emit_half": emit_half}, [data], (0,), K, W, half, verify)


def test_demit_second_trip_after_a_directly_written_last_lane(log):
    """`if (!taken) cur = nx` with a next iteration to hand over to: the first wave-iteration's lane 63 holds a piece that the forward
    pass resolved on its slow path (a hole: an escaped quote at byte 63 * 64 + 20).  Its lane replays it straight into the output, the
    round before it ends at lane 62 and takes nothing over — and wave 0 of workgroup 0 is one of the four that have a second
    iteration."""
    W = 12
    blob = blob_of("apache_log")
    ncu, n = second_trip_length(W, False)
    lines = ti.tiled_input("apache_log", n, 13).split(b"\n")[:-1]
    at, k = 0, 0
    while at + lines[k].index(b" HTTP/") <= 31 * PIECE + 20:      # the first line whose context lies behind byte 2004: stretched up to 4052
        at += len(lines[k]) + 1
        k += 1
    data = with_context_at(lines, k, 31 * PIECE + 20)
    assert data.index(b'\\"') == 63 * PIECE + 20 and data.count(b'\\"') == 1
    want = expect(blob, data)
    assert isinstance(want, bytes)
    p = load("apache_log")
    try:
        p.configure(emit_waves=W)
        got, err = log(p, data)
        assert got == want, err[-600:]
        assert p.stage_delayed_form(0) == 1 and "arms the slow path of its forward pass" in err, err[-600:]
        m = re.search(r"the slow path resolved (\d+) input symbols in place", err)
        assert m and int(m.group(1)) > 0, err[-600:]
        ln, = demit_lines(err)
        assert (ln["K"], ln["W"], ln["half"], ln["maxcnt"]) == (2, W, False, 64), ln      # (one round for lanes 0 to 62, then the hole)
        assert ncu * W < (ln["pieces"] + 63) // 64 < 2 * ncu * W, (ncu, ln)
    finally:
        p.close()


@pytest.mark.parametrize("W", [4, 8])
def test_emit_second_trip(log, W):
    """the same for the general engine's k_emit (KX_DF=0), on apache_log"""
    ncu, n = second_trip_length(W, False)
    data = ti.tiled_input("apache_log", n, 12)

    def verify(ln, d, seg, run):
        assert ln["W"] == W and ncu * W < (ln["pieces"] + 63) // 64 < 2 * ncu * W, ln

    sweep_general(log, "apache_log", {"KX_DF": "0"}, {}, {"emit_waves": W}, [data], (0,), verify)


# -------------------------------------------------------------------------- F. the general engine: k_emit 3 x 4, switches
GENERAL_SEGMENTS = (64, 4096)
LAYOUTS = {  # case: (program, load-time fields, input shape, the line's layout, layout kind)
    "plain": ("apache_log", {"job_stride": 1}, "apache_log", "vote-and-rank", "plain"),
    "inline": (ti.INLINE_PROGRAM, {}, "abcdefgh,\n", "vote-and-rank", "inline"),
    "general": (ti.WIDE_ENTRY_PROGRAM, {}, "abc", "vote-and-rank", "general"),                                   # (constants of 127 bytes and more)
    "general_classes": (ti.CLASSES_PROGRAM, {}, bytes(range(32, 127)).decode(), "vote-and-rank", "general"),     # (more than 64 byte classes)
    "job-stride": ("iso_datetime_to_json", {"job_stride": 2}, "datetime", "job-stride", "job-stride")}
# (the table of the program of 96 byte classes leaves room for 8 waves at the most: the general instance of 12 runs on the other)
EMIT_INSTANCES = [(kind, W) for kind in LAYOUTS for W in (4, 8, 12) if (kind, W) != ("general_classes", 12)]


def rejected_input(blob, shape, seed):
    """an input whose byte 100 000 the program does not take there (a NUL, a line end or FF: the first that the oracle rejects)"""
    d = bytearray(ti.exact_input(shape, 100000 + 4097, seed))
    for bad in (0, 10, 255):
        d[100000] = bad
        if isinstance(expect(blob, bytes(d)), tuple):
            return bytes(d)
    raise AssertionError("the program takes every byte tried at 100 000")


@pytest.mark.parametrize("kind,W", EMIT_INSTANCES, ids=["%s_w%d" % c for c in EMIT_INSTANCES])
def test_emit_instance(log, kind, W):
    """k_emit<W, WIDE, EXT, JL> for W in 4, 8, 12 and the four layout kinds: plain, inline constants, general (wide entries: constants of
    127 bytes and more; and more than 64 byte classes), job-stride (pinned: on a first shard the heuristic never gives it).  The kind
    follows from the blob (test_instances.layout_kind), W and the layout from the line; k_backlen runs its 32-leaf instance of the same
    kind (the program of 96 byte classes, which has 96 leaves: the 256-leaf one).  One rejected input per case: the position is the
    oracle's."""
    prog, fields, shape, layout, family = LAYOUTS[kind]
    blob = blob_of(prog)
    assert ti.layout_kind(blob, fields.get("inline_consts", 0), fields.get("job_stride", 0)) == family
    assert (ti.layout_facts(blob)["Lm"] <= 32) == (kind != "general_classes")
    datas = [ti.exact_input(shape, n, 400 + n) for n in ti.GENERAL_LENGTHS] + [rejected_input(blob, shape, 5)]

    def verify(ln, d, seg, run):
        assert (ln["W"], ln["layout"]) == (W, layout), (seg, len(d), ln)
        assert ln["next"] == "(fixed)"

    sweep_general(log, prog, {"KX_DF": "0"}, fields, {"emit_waves": W}, datas, GENERAL_SEGMENTS, verify)


def test_job_stride_pinned_off_stays_off(log):
    """job_stride = 1 on iso_datetime_to_json (about 13 constants per piece: by itself the stage would change to the job-stride layout
    for its second shard): vote-and-rank over four runs on one Program"""
    data = ti.exact_input("datetime", 70000, 2)
    seen = []

    def verify(ln, d, seg, run):
        assert ln["kavg"] >= 12.0, "the heuristic would not have changed the layout: the case proves nothing"
        seen.append((ln["layout"], ln["next"]))

    sweep_general(log, "iso_datetime_to_json", {"KX_DF": "0"}, {"job_stride": 1}, {}, [data, data], GENERAL_SEGMENTS, verify)
    assert seen == [("vote-and-rank", "(fixed)")] * 4, seen


@pytest.mark.parametrize("prog,shape,inplace,fields", [("apache_log", "apache_log", 2, {"job_stride": 1}), (ti.INLINE_PROGRAM, "abcdefgh,\n", 1, {})],
                         ids=["apache_log_on", "inline_off"])
def test_emit_inplace_pinned(log, prog, shape, inplace, fields):
    """emit_inplace = 2: the sweeping lanes copy every constant in place, no job slots (jobs=0); emit_inplace = 1: job slots even
    where the constants are short"""
    datas = [ti.exact_input(shape, n, 500 + n) for n in ti.GENERAL_LENGTHS]

    def verify(ln, d, seg, run):
        assert (ln["jobs"] == 0) == (inplace == 2), (seg, len(d), ln)

    sweep_general(log, prog, {"KX_DF": "0"}, fields, {"emit_inplace": inplace}, datas, GENERAL_SEGMENTS, verify)


@pytest.mark.parametrize("prog,shape,bit", [("apache_log", "apache_log", host.KX_OFF_CMPX), (ti.INLINE_PROGRAM, "abcdefgh,\n", host.KX_OFF_CMPX),
                                            ("apache_log", "apache_log", host.KX_OFF_DIRECT)], ids=["cmpx_apache_log", "cmpx_inline", "direct_apache_log"])
def test_general_engine_switches(log, prog, shape, bit):
    """KX_OFF_CMPX on stages whose constants are at most 16 bytes (the other store sequence of the constants phase) and KX_OFF_DIRECT
    (constants addressed through their descriptors) — the engine prints nothing about either: the proof is the configuration it took"""
    assert ti.max_constant(blob_of(prog)) <= 16
    datas = [ti.exact_input(shape, n, 600 + n) for n in ti.GENERAL_LENGTHS] + [rejected_input(blob_of(prog), shape, 6)]

    def verify(ln, d, seg, run):
        assert ln["jobs"] > 0 or prog != "apache_log"

    sweep_general(log, prog, {"KX_DF": "0"}, {"disable": bit, "job_stride": 1}, {}, datas, GENERAL_SEGMENTS, verify)


@pytest.mark.parametrize("bt", [64, 1024])
@pytest.mark.parametrize("prog,shape,K", [("apache_log", "apache_log", 2), ("csv2json", "csv", 1)])
def test_block_threads(log, prog, shape, K, bt):
    """workgroups of 64 and of 1024 lanes for every kernel that takes the configured size, in both engines"""
    datas = [ti.exact_input(shape, n, 700 + n) for n in ti.GENERAL_LENGTHS]
    sweep_delayed(log, prog, {}, {"block_threads": bt, "emit_half": 1}, datas, GENERAL_SEGMENTS, K, 12, False)
    sweep_general(log, prog, {"KX_DF": "0"}, {}, {"block_threads": bt}, datas, GENERAL_SEGMENTS, lambda ln, d, seg, run: None)


BACKLEN_256 = {  # k_backlen<256, …>: (program, fields, inputs, layout on the line, layout kind)
    "plain": (ti.LEAVES_PROGRAM, {"job_stride": 1}, "vote-and-rank"),
    "job-stride": (ti.LEAVES_PROGRAM, {"job_stride": 2}, "job-stride"),
    "general": (ti.CLASSES_PROGRAM, {}, "vote-and-rank")}


@pytest.mark.parametrize("kind", list(BACKLEN_256))
def test_backlen_more_than_32_leaves(log, kind):
    """k_backlen's 256-leaf instances: 34 simultaneous paths in the plain and in the job-stride layout, 96 leaves in the general one"""
    prog, fields, layout = BACKLEN_256[kind]
    blob = blob_of(prog)
    assert ti.layout_facts(blob)["Lm"] > 32 and ti.layout_kind(blob, 0, fields.get("job_stride", 0)) == kind
    if prog == ti.LEAVES_PROGRAM:
        datas = [b"a" * k + b"\n" for k in (32, 40, 63, 64, 31, 65)]
        assert [isinstance(expect(blob, d), tuple) for d in datas] == [False] * 4 + [True] * 2
    else:
        datas = [ti.exact_input(bytes(range(32, 127)).decode(), n, 8) for n in ti.GENERAL_LENGTHS]

    def verify(ln, d, seg, run):
        assert ln["layout"] == layout, ln

    sweep_general(log, prog, {"KX_DF": "0"}, fields, {}, datas, GENERAL_SEGMENTS, verify)
