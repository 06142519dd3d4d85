"""What the GPU cases of test_batch_instances_gpu.py rest on, checked without a GPU.

runBatch (kx_batch_host.inc) launches one of twelve kernel instances per stage — k_bforward<WIDE[, BFrame]>, k_bback<WIDE[, BFrame]>,
k_bemit<WIDE>, k_bemit_fr<WIDE, BFrame> — on whichever table image chooseLayout (kx_stage.h) gave the stage.  The batch kernels print no
line of their own: the instance of a stage follows from two conditions of runBatch alone, `wide = S.general` and
`framed = st == 0 && trim != 0` (batch_instances below), and `general` with every layout flag is what kx_stage_describe_cfg reports
for the configuration the Program is loaded with.  This file holds

  CASES       one program and configuration per layout (the table of the GPU file), with the layout flags asserted here;
  bodies_of   the documents the GPU file runs, with the assertions that they reach the layout's own code: a case whose documents
              never touch a 300-byte constant, a byte class beyond 63 or a translated symbol passes vacuously on the GPU and fails HERE;
  slot_ranges the workspace arithmetic of kx_batch.inc's header comment (checkpoint and piece slots per document, no scan), restated
              and held to its three claims on every offset vector the GPU file uses and on random ones."""
import collections
import functools
import random

import numpy as np
import pytest
import kxp
from conftest import blob_of
from test_instances import CLASSES_PROGRAM, INLINE_PROGRAM, LEAVES_PROGRAM, WIDE_ENTRY_PROGRAM, layout_facts

from kleenexlang_amd import host
from oracle import oracle

LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193)   # granule, checkpoint and piece borders, three pieces
LEADS = (1, 7, 16)
# (trim, last_whole, suffix): no frame; a trim; the widest trim and suffix with the last range whole; the unframed kernels plus k_bsuffix
FRAMES = ((0, False, b""), (1, False, b""), (8, True, b"12345678"), (0, False, b"\r\n;"))
ROUTE_MAX = 100                                       # batch_doc_max of the routed round: longer documents take batchRouteOne
ROUTE_MAX_SHORT = 48                                  # … for a language whose longest document has 65 bytes (LEAVES_PROGRAM)
XLAT_REGEX = "(([^,\\n]*),([^,\\n]*)\\n)*"            # the coder of a two-field row: ONE table on every copying entry

CLASS_RULE = CLASSES_PROGRAM[len("main := "):]        # (/\x21/ "33;" | … | ~/ /)*
# a narrow stage that passes DEL (which the class rule refuses) and refuses \n, in front of the class rule; and the class rule in front
# of a narrow stage that refuses { } ~ (which the class rule copies) — so both orders have rejections at both stages
TWO_WIDE_LAST = "start: a >> b\na := (/[\\x20-\\x7f]/ | ~/\\t/ \" \")*\nb := " + CLASS_RULE
TWO_WIDE_FIRST = "start: a >> b\na := " + CLASS_RULE + "b := (/[\\x21-\\x7a]/ | ~/\\|/ \"/\")*\n"
PRINTABLE = bytes(range(33, 127)) + b"   "


# ---------------------------------------------------------------------------------------------------------------- the oracle
def want(blob, doc, cache={}):
    """the oracle on the document alone: its bytes, or (fail_pos, fail_stage)"""
    k = (blob, doc)
    if k not in cache:
        try:
            cache[k] = oracle.run(blob, doc)
        except oracle.OracleMatchError as e:
            cache[k] = (e.pos, e.stage)
    return cache[k]


# ------------------------------------------------------------------------------------------------------------ accepted bodies
def over(alphabet):
    return lambda L, r: bytes(r.choice(alphabet) for _ in range(L))


def _quoted(k, r):
    out = bytearray()
    while len(out) < k:
        if k - len(out) >= 2 and r.random() < 0.1:
            out += b'\\"'
        else:
            out.append(r.choice(b"abcXYZ /.-_?=1"))
    return bytes(out)


def _apache_line(n, r):
    """one combined-log line of exactly n >= 29 bytes: the spare bytes spread over the eight fields that stretch"""
    x = [0] * 8
    for _ in range(n - 29):
        x[r.randrange(8)] += 1
    digits = lambda k: bytes(r.choice(b"0123456789") for _ in range(k))   # noqa: E731
    word = lambda k: bytes(r.choice(b"abcxyz:/+") for _ in range(k))      # noqa: E731
    line = (digits(1 + x[0]) + b".2.3.4 - " + word(1 + x[1]) + b" [" + word(1 + x[2]) + b'] "' + _quoted(x[3], r) + b'" ' + digits(1 + x[4]) + b" "
            + digits(1 + x[5]) + b' "' + _quoted(x[6], r) + b'" "' + _quoted(x[7], r) + b'"\n')
    assert len(line) == n
    return line


def _lines(L, r, shortest, line):
    """L bytes of whole lines, each of `shortest` bytes and more"""
    if L == 0:
        return b""
    if L < shortest:
        return None
    out = []
    while L:
        n = L if L < 2 * shortest or r.randrange(2) else r.randrange(shortest, L - shortest + 1)
        out.append(line(n, r))
        L -= n
    return b"".join(out)


def apache_body(L, r):
    return _lines(L, r, 29, _apache_line)


def _iso_line(n, r):
    """an xs:dateTime line of exactly n >= 21 bytes: 21 with the zone Z, 26 with an offset, the year stretched by the rest"""
    zone = b"Z" if n < 26 or r.randrange(2) else b"+%02d:%02d" % (r.randrange(24), r.randrange(60))
    x = n - 20 - len(zone)
    year = (bytes([r.choice(b"123456789")]) + bytes(r.choice(b"0123456789") for _ in range(x - 1)) if x else b"") + b"%04d" % r.randrange(10000)
    line = year + b"-%02d-%02dT%02d:%02d:%02d" % (r.randrange(1, 13), r.randrange(1, 29), r.randrange(24), r.randrange(60), r.randrange(60)) + zone + b"\n"
    assert len(line) == n
    return line


def iso_body(L, r):
    return _lines(L, r, 21, _iso_line) if L else None          # (stamps is a plus: no empty document)


def leaves_body(L, r):
    return b"a" * (L - 1) + b"\n" if 33 <= L <= 65 else None   # a{32..64}\n


def _row(n, r):
    k = r.randrange(n - 1)
    field = lambda m: bytes(r.choice(b"abcdefXYZ 0123456789;.\t\xe9") for _ in range(m))   # noqa: E731
    return field(k) + b"," + field(n - 2 - k) + b"\n"


def rows_body(L, r):
    return _lines(L, r, 2, _row)


# ------------------------------------------------------------------------------------------------------------------ the cases
# name; program (shipped name, source, or regex); kx_config fields; accepted body of a length (or None); candidates for the refused
# byte, tried in order; 8 bytes that are refused behind every accepted body (what a trim cuts off); lengths beside LENGTHS for a language
# that has few of them; WIDE per stage; whether a body cut before its end is rejected there (a non-final prefix)
Case = collections.namedtuple("Case", "name prog cfg body reject junk extra wide cut")


def _cases():
    big = {"force": host.KX_FORCE_BIG}
    plain = {"job_stride": 1, "inline_consts": 1}
    apache = ("apache_log", apache_body, b"\n\"x", b"\n" * 8, (29, 30, 47, 48, 49, 95, 96, 97))
    wide_e = (WIDE_ENTRY_PROGRAM, over(b"abc"), b"z", b"z" * 8, ())
    classes = (CLASSES_PROGRAM, over(PRINTABLE), b"\n", b"\n" * 8, ())
    xlat = ("re:" + XLAT_REGEX, rows_body, b"\n,", b"\n" * 8, (2, 3))
    leaves = (LEAVES_PROGRAM, leaves_body, b"b", b"b" * 8, (40, 47, 48, 49, 50))
    t = [
        ("plain_direct", apache, plain, (False,), True),
        ("plain_nodirect", apache, dict(plain, disable=host.KX_OFF_DIRECT), (False,), True),
        ("inline", (INLINE_PROGRAM, over(b"abcdefgh,\n"), b"z", b"z" * 8, ()), {}, (False,), False),
        ("inline_pinned", apache, {"inline_consts": 2}, (False,), True),
        ("job_stride", ("iso_datetime_to_json", iso_body, b"x\n", b"\n" * 8, (21, 26, 42, 47, 48, 52)), {"job_stride": 2}, (False,), True),
        ("leaves_js1", leaves, {"job_stride": 1}, (False,), True),
        ("leaves_js2", leaves, {"job_stride": 2}, (False,), True),
        ("wide_entries", wide_e, {}, (True,), False),
        ("classes", classes, {}, (True,), False),
        ("xlat", xlat, {}, (False,), True),
        ("tblmode", xlat, {"force": host.KX_FORCE_TBLMODE}, (True,), True),
        ("big_plain_direct", apache, dict(plain, **big), (True,), True),
        ("big_wide_entries", wide_e, big, (True,), False),
        ("big_classes", classes, big, (True,), False),
        ("big_xlat", xlat, big, (True,), True),
        ("two_stage_wide_last", (TWO_WIDE_LAST, over(PRINTABLE + b"\t\t"), b"\n\x7f", b"\n" * 8, ()), {}, (False, True), False),
        ("two_stage_wide_first", (TWO_WIDE_FIRST, over(bytes(range(33, 123)) + b"   ||"), b"\n{", b"\n" * 8, ()), {}, (True, False), False),
    ]
    return [Case(name, p[0], cfg, p[1], p[2], p[3], p[4], wide, cut) for name, p, cfg, wide, cut in t]


CASES = _cases()
CASE = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def blob(name):
    prog = CASE[name].prog
    return host.compile_regex(prog[3:]) if prog.startswith("re:") else blob_of(prog)


def config(name, **more):
    """the kx_config the case's Program is loaded with, and stage_describe is asked about"""
    return host.config_from_env({}, **dict(CASE[name].cfg, **more))


def describe(name, stage=0):
    return host.stage_describe(blob(name), stage, cfg=config(name), with_image=False)[0]


def instance_names(wide, framed):
    w = "true" if wide else "false"
    if framed:
        return ("k_bforward<%s, BFrame>" % w, "k_bback<%s, BFrame>" % w, "k_bemit_fr<%s, BFrame>" % w)
    return ("k_bforward<%s>" % w, "k_bback<%s>" % w, "k_bemit<%s>" % w)


def batch_instances(info, stage, trim):
    """The three kernel instances runBatch launches for a stage, from what stage_describe says of it and the call's trim: WIDE is
    Stage::general, the framed instances run exactly for stage 0 of a call with trim != 0."""
    return instance_names(bool(info.general), stage == 0 and trim != 0)


ALL_INSTANCES = {k for wide in (False, True) for framed in (False, True) for k in instance_names(wide, framed)}


def test_batch_instances_is_runbatchs_choice():
    assert len(ALL_INSTANCES) == 12
    got = set()
    for name in ("plain_direct", "classes", "two_stage_wide_last", "two_stage_wide_first"):
        for st in range(len(CASE[name].wide)):
            for trim in (0, 1):
                got |= set(batch_instances(describe(name, st), st, trim))
    assert got == ALL_INSTANCES
    assert batch_instances(describe("two_stage_wide_last", 1), 1, 8) == ("k_bforward<true>", "k_bback<true>", "k_bemit<true>")   # (a later stage: never framed)
    assert batch_instances(describe("classes"), 0, 2) == ("k_bforward<true, BFrame>", "k_bback<true, BFrame>", "k_bemit_fr<true, BFrame>")
    # every case of the matrix runs with and without a trim: the single-stage narrow cases cover the six <false…> instances, the
    # single-stage wide ones the six <true…>; the pipelines add the unframed instances of a later stage
    for name in NAMES:
        assert {k for st in range(len(CASE[name].wide)) for t in (0, 1) for k in batch_instances(describe(name, st), st, t)} == \
               {k for st, w in enumerate(CASE[name].wide) for t in (0, 1) for k in instance_names(w, st == 0 and t)}, name


# ------------------------------------------------------------------------------------------------------------- layout flags
def _flags(info):
    return {"general": info.general, "big": info.big, "inl": info.t.inl, "jl": info.t.jl, "direct": info.t.direct, "xlat": int(info.t.xlat != 0),
            "tblmode": info.t.tblmode}


LAYOUT = {
    "plain_direct": {"general": 0, "big": 0, "inl": 0, "jl": 0, "direct": 1, "xlat": 0, "tblmode": 0},
    "plain_nodirect": {"general": 0, "big": 0, "inl": 0, "jl": 0, "direct": 0, "xlat": 0, "tblmode": 0},
    "inline": {"general": 0, "big": 0, "inl": 1},
    "inline_pinned": {"general": 0, "big": 0, "inl": 1},
    "job_stride": {"general": 0, "big": 0, "inl": 0, "jl": 1},
    "leaves_js1": {"general": 0, "big": 0, "jl": 0},
    "leaves_js2": {"general": 0, "big": 0, "jl": 1},
    "wide_entries": {"general": 1, "big": 0, "tblmode": 0},
    "classes": {"general": 1, "big": 0, "tblmode": 0},
    "xlat": {"xlat": 1, "tblmode": 0, "big": 0},
    "tblmode": {"tblmode": 1, "general": 1, "xlat": 0, "big": 0},
    "big_plain_direct": {"big": 1, "general": 1, "inl": 0, "jl": 0, "direct": 0},
    "big_wide_entries": {"big": 1, "general": 1, "inl": 0, "jl": 0, "direct": 0},
    "big_classes": {"big": 1, "general": 1, "inl": 0, "jl": 0, "direct": 0},
    "big_xlat": {"big": 1, "general": 1, "inl": 0, "jl": 0, "direct": 0, "xlat": 1},
    "two_stage_wide_last": {"general": 0, "big": 0},
    "two_stage_wide_first": {"general": 1, "big": 0},
}


@pytest.mark.parametrize("name", NAMES)
def test_layout_of_the_case(name):
    """the row of the GPU file's table: what the loader builds for the case's program under the case's configuration"""
    c = CASE[name]
    info = describe(name)
    got = _flags(info)
    assert {k: got[k] for k in LAYOUT[name]} == LAYOUT[name], (name, got)
    for st, wide in enumerate(c.wide):
        assert bool(describe(name, st).general) == wide, (name, st)
    assert len(kxp.parse(blob(name))) == len(c.wide)
    facts = layout_facts(blob(name)) if kxp.parse(blob(name))[0].tables is None else None     # (layout_facts reads no table field)
    if name.startswith("leaves"):
        assert info.t.maxleaves > 32
    if name in ("wide_entries", "big_wide_entries"):
        assert info.t.nclasses <= 64 and facts["widest"] >= 127
    if name in ("classes", "big_classes"):
        assert info.t.nclasses > 64 and info.t.cshift != 0
    if name == "two_stage_wide_last":
        assert describe(name, 1).t.nclasses > 64
    if name == "inline_pinned":                       # pinned against the loader's own choice, with entries that carry the 0x8000 flag
        assert facts["longer"] > facts["one"] > 0
        assert host.stage_describe(blob(name), 0, cfg=host.config_from_env({}), with_image=False)[0].t.inl == 0
    if name == "inline":
        assert facts["one"] > 0 and facts["longer"] > 0


# ------------------------------------------------------------------------------------------------------------- the documents
@functools.lru_cache(maxsize=None)
def accepted_bodies(name):
    """three bodies of every length the language has (LENGTHS and the case's own), in the order they are made"""
    c = CASE[name]
    r = random.Random(len(name) * 7 + 1)
    out = []
    for rep in range(3):
        for L in LENGTHS + c.extra:
            b = c.body(L, r)
            if b is not None:
                out.append(b)
    return tuple(out)


def rejected_variants(name, body):
    """`body` with a refused byte at position 0, at 31 or 32, at 63 or 64 and at its last byte, and cut before its last byte where
    the language has non-final prefixes.  The refused byte is the first of the case's candidates with which the ORACLE rejects the
    document at that very position; else the first with which it rejects it at all.  (A pipeline's candidates are one byte per stage:
    there the first that rejects the document, the candidates taking turns.)"""
    c, bl = CASE[name], blob(name)
    out = []
    n = len(body)
    alt = (n >> 2) & 1
    for k, p in enumerate(sorted({0, 31 + alt, 63 + alt, n - 1})):
        if not 0 <= p < n:
            continue
        best = None
        turn = (k + n) % len(c.reject) if len(c.wide) > 1 else 0     # (a pipeline: the stages' refused bytes take turns)
        for ch in c.reject[turn:] + c.reject[:turn]:
            v = body[:p] + bytes([ch]) + body[p + 1:]
            w = want(bl, v)
            if v != body and isinstance(w, tuple):
                if w[0] == p or len(c.wide) > 1:
                    best = v
                    break
                best = best or v
        if best:
            out.append(best)
    if c.cut and n and isinstance(want(bl, body[:-1]), tuple):
        out.append(body[:-1])
    return out


@functools.lru_cache(maxsize=None)
def bodies_of(name):
    """The documents of the case's matrix: the accepted bodies, the rejected variants of every fourth, five empty ones (where the
    language has no empty document: five of its shortest) — shuffled, and behind them two more of those side by side and an accepted
    body of 64 bytes or the nearest the language has (with last_whole the last range keeps its junk)."""
    c = CASE[name]
    r = random.Random(len(name) * 13 + 5)
    acc = list(accepted_bodies(name))
    docs = list(acc)
    for b in acc[::4]:
        docs += rejected_variants(name, b)
    short = [b for b in (c.body(L, r) for L in sorted(c.extra + LENGTHS)) if b is not None]     # (the language's shortest documents first)
    fill = [b""] * 7 if c.body(0, r) is not None else short[:7]                                   # no empty document: its shortest ones instead
    docs += fill[:5] + [next(b for L in (65, 64, 50) for b in [c.body(L, r)] if b is not None)]
    r.shuffle(docs)
    return tuple(docs + fill[5:] + [next(b for L in (64, 63, 50) for b in [c.body(L, r)] if b is not None)])


FIRST_STAGE = {"two_stage_wide_last": TWO_WIDE_LAST.split("\n")[1].replace("a := ", "main := ") + "\n", "two_stage_wide_first": CLASSES_PROGRAM}


def routed_expected(name, docs, doc_max):
    """kx_batch_stats::docs_routed of a run with batch_doc_max = doc_max: per stage, the documents longer than that which no earlier
    stage rejected (a later stage's documents are the outputs of the stage before it: the oracle on that stage alone)"""
    n = sum(len(d) > doc_max for d in docs)
    if name in FIRST_STAGE:
        mid = [want(blob_of(FIRST_STAGE[name]), d) for d in docs]
        n += sum(isinstance(w, bytes) and len(w) > doc_max for w in mid)
    return n


def route_max(name):
    return ROUTE_MAX if max(map(len, accepted_bodies(name))) > ROUTE_MAX else ROUTE_MAX_SHORT


def pack(name, docs, trim):
    """every document followed by `trim` bytes of the case's junk: (data, offsets)"""
    return host.pack_batch([d + CASE[name].junk[:trim] for d in docs])


@pytest.mark.parametrize("name", NAMES)
def test_documents_reach_the_layouts_own_code(name):
    c, bl = CASE[name], blob(name)
    docs = bodies_of(name)
    acc = accepted_bodies(name)
    wants = [want(bl, d) for d in docs]
    assert all(isinstance(want(bl, b), bytes) for b in acc), (name, next(b for b in acc if not isinstance(want(bl, b), bytes)))
    naccepted = sum(isinstance(w, bytes) for w in wants)
    assert 2 * naccepted >= len(docs) + 2 and len(docs) - naccepted >= 10, (name, naccepted, len(docs))     # (+ 2: with last_whole the last document is rejected)
    # every length the language has, three of each; the lengths it lacks are lacking from the LANGUAGE (the maker says so, the oracle agrees on some)
    have = {L for L in LENGTHS if c.body(L, random.Random(L)) is not None}
    assert {len(b) for b in acc} >= have and all(sum(len(b) == L for b in acc) == 3 for L in have), name
    assert len(have | set(c.extra)) >= 8 and max(len(b) for b in acc) >= 65, (name, sorted(have))
    # what a trim cuts off is refused behind every accepted body: a kernel that ignores the trim rejects the document
    for b in acc:
        for t in (1, 2, 8):
            assert isinstance(want(bl, b + c.junk[:t]), tuple), (name, b, t)
    # rejections at the start, around both checkpoints of a piece, around a piece border and at (or behind) the last byte
    fails = {w[0] for w in wants if isinstance(w, tuple)}
    lens = {len(d) for d, w in zip(docs, wants) if isinstance(w, tuple)}
    assert 0 in fails and fails & {31, 32} and (fails & {63, 64} or max(len(b) for b in acc) <= 65), (name, sorted(fails))
    assert any(isinstance(w, tuple) and w[0] >= len(d) - 1 and len(d) > 65 for d, w in zip(docs, wants)) or max(lens) <= 65, name
    if c.cut:
        assert any(isinstance(w, tuple) and w[0] == len(d) for d, w in zip(docs, wants)), (name, "no document ends in a non-final state")
    stages = {w[1] for w in wants if isinstance(w, tuple)}
    assert stages == set(range(len(c.wide))), (name, stages)
    outs = [w for w in wants if isinstance(w, bytes)]
    if name in ("wide_entries", "big_wide_entries"):
        assert any(b"x" * 300 in o for o in outs) and any(b"<" + b"y" * 130 + b">" in o for o in outs)
        assert any(len(want(bl, d[k:k + 64])) > 8192 for d, w in zip(docs, wants) if isinstance(w, bytes) for k in range(0, len(d), 64)), name
    if name == "inline":
        joined = b"".join(d for d, w in zip(docs, wants) if isinstance(w, bytes))
        assert set(joined) >= set(b"abcdefgh,\n") and any(b"<end of line>\n" in o for o in outs) and any(b"a1" in o for o in outs)
    if name == "inline_pinned":
        assert sum(b'"host":"' in o and b'",' in o for o in outs) >= 30
    if name in ("classes", "big_classes", "two_stage_wide_last", "two_stage_wide_first"):
        st = kxp.parse(bl)[c.wide.index(True)]
        used = {int(st.cls[x]) for d, w in zip(docs, wants) if isinstance(w, bytes) for x in d.replace(b"\t", b" ")}   # (stage 0 of wide_last: tab to blank)
        assert max(used) >= 64 and len(used) > 64, (name, len(used))
    if name in ("xlat", "tblmode", "big_xlat"):
        st = kxp.parse(bl)[0]
        assert st.tables is not None and len(st.tables) == 1
        moved = {x for d, w in zip(docs, wants) if isinstance(w, bytes) for x in d if x not in b",\n" and int(st.tables[0][x]) != x}
        assert len(moved) >= 10, (name, moved)
        assert want(bl, b"ab,\xe9\n")[-3:] != b"ab\xe9" and bytes([int(st.tables[0][0xe9])]) in want(bl, b"ab,\xe9\n")
    if len(c.wide) == 2:
        assert sum(isinstance(w, tuple) and w[1] == 0 for w in wants) >= 5 and sum(isinstance(w, tuple) and w[1] == 1 for w in wants) >= 5, name


# ----------------------------------------------------------------------------------------- generated programs (part c)
# Every fourth seed of randprog.program_wide, and seed 109.  `general` (the WIDE instances) is not "more than 31 byte classes" (that is
# the delayed form's wide walk): it takes more than 64 classes, an entry of 127 bytes and more, per-entry tables or BIG.
# program_wide has at most 45 classes and constants of at most 40 bytes, so a generated stage is general only where its tables
# outgrow LDS addressing (BIG): of seeds 0-119 that is the first (and only) stage of seeds 31 and 109 — no multiple of 4, and no
# two-stage program on any stride: the second stage, `tidy`, has three classes and a handful of states on every seed.  So the stride
# stays and seed 109 is added (seed 31 takes 20 s to compile); and every two-stage program of the run runs once more with
# KX_FORCE_BIG, which makes both of its stages general: that is the generated population with a general LATER stage (offsets from the
# workspace, BM_SKIP documents from the stage before).  The hand-written two_stage_wide_last case has one by itself.
WIDE_BIG_SEEDS = (109,)
WIDE_SEEDS = tuple(range(0, 120, 4)) + WIDE_BIG_SEEDS
WIDE_PARTS = 3


def wide_generals(seed, **fields):
    """`general` of every stage of program_wide(seed) as the loader builds it under the configuration, or None (no such program)"""
    import test_random_inputs as tr
    src = tr.source("wide", seed)
    if src is None:
        return None
    bl = blob_of(src, 3)
    cfg = host.config_from_env({}, **fields)
    return [host.stage_describe(bl, st, cfg=cfg, with_image=False)[0].general for st in range(len(kxp.parse(bl)))]


def test_generated_wide_programs_with_a_general_stage():
    g = {seed: wide_generals(seed) for seed in WIDE_SEEDS}
    assert all(v is not None for v in g.values())
    assert [s for s, v in g.items() if v[0]] == list(WIDE_BIG_SEEDS) and not any(v[1] for v in g.values() if len(v) > 1)
    two = [s for s, v in g.items() if len(v) > 1]
    assert len(two) >= 8 and all(len(two[k::WIDE_PARTS]) >= 2 for k in range(WIDE_PARTS))
    for s in two:
        assert wide_generals(s, force=host.KX_FORCE_BIG) == [1, 1], s
    for k in range(WIDE_PARTS):
        assert len(WIDE_SEEDS[k::WIDE_PARTS]) >= 10


# ------------------------------------------------------------------------------------------------- the other parts' documents
def pool_of(name):
    """about 40 distinct bodies of 0 to 5 bytes for the grid-stride and scan-edge runs: accepted, rejected and empty ones.
    wide_entries: the bodies with `a` (300 output bytes) or `c` (132) are drawn a sixteenth as often as the others (pool_draw), so that
    half a million documents stay well under 64 MB of output."""
    r = random.Random(len(name))
    alphabet, reject = {"classes": (PRINTABLE, b"\n\x00"), "wide_entries": (b"bbbbbbcca", b"z")}[name]
    pool = {b""}
    while len(pool) < 30:
        pool.add(bytes(r.choice(alphabet) for _ in range(r.randrange(1, 6))))
    while len(pool) < 40:
        b = bytearray(r.choice(alphabet) for _ in range(r.randrange(1, 6)))
        b[r.randrange(len(b))] = r.choice(reject)
        pool.add(bytes(b))
    return sorted(pool)


def pool_draw(name, ndocs, seed=0):
    """(pool, indices): ndocs documents drawn from the pool, empty ones side by side somewhere"""
    pool = pool_of(name)
    weight = np.array([1.0 if name == "wide_entries" and (b"a" in b or b"c" in b) else 16.0 for b in pool])    # (the long constants: drawn less often)
    idx = np.random.RandomState(seed + ndocs % 1000).choice(len(pool), size=ndocs, p=weight / weight.sum())
    idx[ndocs // 2:ndocs // 2 + 3] = pool.index(b"")
    return pool, idx


def pool_arrays(name, ndocs, trim, junk, suffix, seed=0):
    """The packed batch and what the oracle says of it, built with numpy: (data, offsets, expected output, expected output offsets,
    status, fail_pos).  The oracle runs once per distinct body."""
    pool, idx = pool_draw(name, ndocs, seed)
    bl = blob(name)
    wants = [want(bl, b) for b in pool]
    parts = [np.frombuffer(b + junk[:trim], dtype=np.uint8) for b in pool]
    outs = [np.frombuffer(w + suffix, dtype=np.uint8) if isinstance(w, bytes) else np.zeros(0, np.uint8) for w in wants]

    def gather(pieces):
        lens = np.array([len(p) for p in pieces], dtype=np.int64)
        starts = np.concatenate(([0], np.cumsum(lens)))[:-1]
        flat = np.concatenate(pieces) if lens.sum() else np.zeros(0, np.uint8)
        n = lens[idx]
        off = np.concatenate(([0], np.cumsum(n)))
        src = np.repeat(starts[idx] - off[:-1], n) + np.arange(off[-1])
        return flat[src].tobytes(), off
    data, off = gather(parts)
    out, ooff = gather(outs)
    status = np.array([int(isinstance(w, tuple)) for w in wants], dtype=np.int64)[idx]
    fpos = np.array([w[0] if isinstance(w, tuple) else 0 for w in wants], dtype=np.int64)[idx]
    return data, off, out, ooff, status, fpos


MI355X_CUS = 256
SCAN_EDGES = (1023, 1024, 1025, 2049)


def second_trip_docs(ncu):
    """one document more than two trips' worth of the grid-stride loops: bgrid = ncu * 4 workgroups of BATCH_BT = 512 lanes"""
    return ncu * 4 * 512 + 1025


def test_pools_hold_accepted_rejected_and_empty_documents():
    for name in ("classes", "wide_entries"):
        pool = pool_of(name)
        wants = [want(blob(name), b) for b in pool]
        assert len(pool) == 40 and b"" in pool and max(map(len, pool)) == 5
        assert sum(isinstance(w, bytes) for w in wants) == 30 and sum(isinstance(w, tuple) for w in wants) == 10
        fails = {w[0] for w in wants if isinstance(w, tuple)}
        assert 0 in fails and len(fails) >= 3, fails
        junk = CASE[name].junk
        data, off, out, ooff, status, fpos = pool_arrays(name, 5000, 1, junk, b"\n")
        _, idx = pool_draw(name, 5000)
        assert data == b"".join(pool[i] + junk[:1] for i in idx) and off[-1] == len(data)
        assert out == b"".join(wants[i] + b"\n" for i in idx if isinstance(wants[i], bytes)) and ooff[-1] == len(out)
        assert status.tolist() == [int(isinstance(wants[i], tuple)) for i in idx] and 2 * status.sum() < len(idx)
    # the output of the second-trip run on wide_entries stays under 64 MB on an MI355X
    pool, idx = pool_draw("wide_entries", second_trip_docs(MI355X_CUS))
    lens = np.array([len(w) if isinstance(w, bytes) else 0 for w in (want(blob("wide_entries"), b) for b in pool)])
    assert 4 << 20 < lens[idx].sum() < 48 << 20
    assert any(b"a" in b for b in pool) and any(b"c" in b for b in pool)
    st = kxp.parse(blob("classes"))[0]
    assert max(int(st.cls[x]) for b in pool_of("classes") for x in b) >= 64


def end_bodies(name, last):
    """Part e: a few documents and a LAST one of `last` bytes (both languages have every length)"""
    c = CASE[name]
    r = random.Random(last)
    return [c.body(33, r), c.body(64, r), b"", c.body(17, r), c.body(last, r)]


END_LEAD = 3
END_CASES = {"inline": (1, 16, 17, 64), "wide_entries": (1, 16, 17, 64)}       # one narrow and one wide case: last bodies of these lengths


def end_batch(name, last, trim):
    """(data, offsets) of end_bodies behind one more accepted document, as long as it takes for the last document to start at residue
    15 of a 16-byte granule when the batch lies END_LEAD bytes into a buffer that ends with it"""
    docs = end_bodies(name, last)
    _, offs = pack(name, docs, trim)
    fill = (15 - (END_LEAD + offs[-2] + trim)) % 16
    return pack(name, [CASE[name].body(fill, random.Random(fill))] + docs, trim)


def test_buffer_end_batches_put_the_last_document_at_residue_15():
    for name, lasts in END_CASES.items():
        for last in lasts:
            for trim in (0, 1):
                data, offs = end_batch(name, last, trim)
                assert (END_LEAD + offs[-2]) % 16 == 15 and offs[-1] - offs[-2] == last + trim and offs[-1] == len(data)
                assert isinstance(want(blob(name), data[offs[-2]:offs[-1] - trim]), bytes)


# ---------------------------------------------------------------------------------------------------------- slot arithmetic
def slot_ranges(off, trim=0, last_whole=False):
    """kx_batch.inc's header comment, restated.  Document i with relative start r = off[i] - off[0] and a range of n_i bytes owns
    checkpoint slots [r/32 + i, r/32 + i + n_i/32] (bchk_base) and piece slots [r/64 + i, (r + n_i)/64 + i + 1) (bpiece_base of i and of
    i + 1).  -> dict of arrays: the ranges, the highest checkpoint slot and the piece slots that a document of the TRIMMED length writes
    (k_bforward: one checkpoint per 32 symbols begun, k_bback: one record per 64), and the sizes runBatch gives the two buffers."""
    off = np.asarray(off, dtype=np.int64)
    nd = len(off) - 1
    i = np.arange(nd, dtype=np.int64)
    r, n = off[:-1] - off[0], np.diff(off)
    cut = np.full(nd, trim, dtype=np.int64)
    if last_whole and nd:
        cut[-1] = 0
    m = n - cut
    assert (n >= 0).all() and (m >= 0).all()
    last_piece = np.maximum(m - 1, 0) // 64
    chk_top = np.where(m > 0, 2 * last_piece + (m - 64 * last_piece >= 32), -1)     # relative to the document's first slot
    total = int(off[-1] - off[0])
    return {"chk_lo": r // 32 + i, "chk_hi": r // 32 + i + n // 32, "pc_lo": r // 64 + i, "pc_hi": (r + n) // 64 + i + 1,
            "chk_top": chk_top, "pieces": (m + 63) // 64, "nchk": (total >> 5) + nd + 2, "nslots": (total >> 6) + nd}


def assert_slots(off, trim=0, last_whole=False):
    s = slot_ranges(off, trim, last_whole)
    assert (s["chk_hi"][:-1] < s["chk_lo"][1:]).all() and (s["pc_hi"][:-1] <= s["pc_lo"][1:]).all(), "consecutive documents' ranges overlap"
    if len(s["chk_lo"]):
        assert s["chk_hi"].max() < s["nchk"] and s["pc_hi"].max() <= s["nslots"], "a range beyond the buffer runBatch sizes"
        assert s["pc_hi"][-1] == s["nslots"]                  # (k_bback marks every slot below nslots: the ranges tile [0, nslots))
        assert s["pc_lo"][0] == 0 and (s["pc_hi"][:-1] == s["pc_lo"][1:]).all()
    assert (s["chk_lo"] + s["chk_top"] <= s["chk_hi"]).all() and (s["pc_lo"] + s["pieces"] <= s["pc_hi"]).all(), "a document needs more than its range"
    return s


def test_slot_ranges_on_a_worked_example():
    # two documents of 64 + 1 bytes at a piece-aligned start: each range holds two piece slots, the trimmed documents need one
    s = assert_slots([0, 65, 130], trim=1)
    assert s["pc_lo"].tolist() == [0, 2] and s["pc_hi"].tolist() == [2, 4] and s["pieces"].tolist() == [1, 1]
    assert s["chk_lo"].tolist() == [0, 3] and s["chk_hi"].tolist() == [2, 5] and s["chk_top"].tolist() == [1, 1]
    assert assert_slots([0, 65, 130], trim=1, last_whole=True)["pieces"].tolist() == [1, 2]
    assert assert_slots([5, 5, 5, 5])["pc_hi"].tolist() == [1, 2, 3]
    with pytest.raises(AssertionError):
        assert_slots([0, 65, 130], trim=66)


def gpu_offset_vectors():
    """every (offsets, trim, last_whole) the GPU file hands the engine (the leads shift every offset alike: r is relative)"""
    for name in NAMES:
        docs = bodies_of(name)
        for trim, last_whole, _ in FRAMES + ((2, False, b""),):
            _, offs = pack(name, docs, trim)
            for lead in LEADS:
                yield [o + lead for o in offs], trim, last_whole
        _, offs = pack(name, accepted_bodies(name), 2)
        yield offs, 2, False
    for name, trim in (("classes", 1), ("wide_entries", 0)):
        for nd in SCAN_EDGES + (second_trip_docs(MI355X_CUS), second_trip_docs(304)):
            yield pool_arrays(name, nd, trim, CASE[name].junk, b"")[1], trim, False
    for name, lasts in END_CASES.items():
        for last in lasts:
            for trim in (0, 1):
                yield [o + END_LEAD for o in end_batch(name, last, trim)[1]], trim, False


def test_slot_ranges_of_every_batch_the_gpu_file_runs():
    count = 0
    for off, trim, last_whole in gpu_offset_vectors():
        assert_slots(off, trim, last_whole)
        count += 1
    assert count > 250


def test_slot_ranges_of_random_batches():
    r = random.Random(11)
    for k in range(4000):
        trim = r.choice((0, 0, 1, 2, 8))
        nd = r.choice((1, 2, 3, 17, 200))
        lens = [r.choice((0, 0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129)) if r.random() < 0.6 else r.randrange(0, 700) for _ in range(nd)]
        last_whole = trim > 0 and r.random() < 0.3
        off = [r.choice((0, 1, 7, 16, 63, 64, 1 << 33))]
        for j, n in enumerate(lens):
            off.append(off[-1] + n + (0 if last_whole and j == nd - 1 else trim))
        s = assert_slots(off, trim, last_whole)
        # exact where it matters: a document of n bytes at a piece-aligned start needs all of its ceil(n / 64) slots
        for j in range(nd):
            if (off[j] - off[0]) % 64 == 0 and trim == 0:
                assert s["pieces"][j] == (lens[j] + 63) // 64 and s["pc_hi"][j] - s["pc_lo"][j] == lens[j] // 64 + 1
