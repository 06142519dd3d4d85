"""The case table of test_run_device_gpu.py and what it rests on, checked without a GPU.

kx_run_device is the device-to-device entry of the single-document engine, the call bench.py times.  The GPU file runs it into a
caller's buffer of exactly the result's length between guards and asks what the call did to memory it does not own: a store behind
`*out_len`, a byte it forgot, a read behind `n`.  Which kernel writes the output depends on the program and on kx_config: a ROUTE here
is one program under one configuration, and a route keeps ONE Program for all of its inputs.  Which bytes a wrong store would hit
depends on the input: whether the result ends on a 16-byte boundary (the flushes of k_demit and k_emit store 16 bytes at a time, heads
and tails bytewise), whether the last piece is partial, whether the result is empty or shorter than one store.  This file builds the
routes and their inputs from the oracle alone and asserts that they are what they claim:

  * every route's layout flags (kx_stage_describe_cfg), all of them, and whether, and at which delay, its first stage runs on the
    delayed form; for the pipelines the same of every later stage;
  * per route, the accepted inputs' result lengths cover every residue modulo 16 that the language has (all 16, except the coder of
    [a-d]*: two code bytes per symbol and one at the end, an odd length always: its 8 odd residues);
  * over the table as a whole, results of 0 and of every length from 1 to 15 bytes;
  * three size groups per route: under 64 bytes (one partial piece; where the language has no such input beside the empty one, its
    shortest), around 4 KiB (one wave-iteration of 64 pieces; n % 64 of 0, 1 and 63 for every table, within 1 KiB of 4 KiB: the last
    line is stretched to fit where lines vary) and around 40 KiB (several workgroups);
  * the hole routes' larger inputs hold an escaped quote in their first 4 KiB and behind it;
  * every route has rejected variants (oracle.OracleMatchError): damaged at byte 0, damaged inside the last piece and, where the
    language has lines, cut in mid-line; one pipeline's are rejected by a later stage;
  * every table has a byte other than 0 that its program rejects (the junk around the input: valid, rejected and zeros differ)."""
import collections
import functools
import random

import pytest
import test_instances as ti
from conftest import blob_of
from test_register_actions import PROGRAMS

from kleenexlang_amd import host, workloads
from oracle import oracle

PIECE = 64
# (test_multi_stage_pipeline_on_device's program: three stages, the last one reads the stage buffer)
THREE_STAGES = 'start: p >> a >> b\np := (~/abc/ "a")*\na := (/./ "b")*\nb := (/ab/ "c" | ~/[^ab]/ "lol")*\n'
# a pipeline whose SECOND stage can reject what the first accepts (a "z", or a lone "y")
LATE_REJECT = 'start: p >> q\np := (~/x/ "yy" | /[^x]/)*\nq := (~/yy/ "z" | /[a-w]/ | /\\n/)*\n'
# the result's first two bytes are written before any input (k_emit's init copy), and an input of x's appends nothing to them
INIT_ONLY = 'main := "<<" (~/x/ | /y/ "!!")*\n'
CODER = "re:[a-d]*"

Route = collections.namedtuple("Route", "name prog fields seg table delay flags")
GENERAL = {"delayed_form": 1}                                    # (KX_DF=0)


def _routes():
    plain = {"general": 0, "big": 0, "inl": 0, "jl": 0, "direct": 1, "xlat": 0, "tblmode": 0}      # (every flag _flags() reads)
    t = []
    # the delayed form and the general engine on the three workloads, each at segment_bytes 64 and 0 (the engine's own choice)
    for seg in (0, 64):
        s = "_seg64" if seg else ""
        t += [("df_k2" + s, "apache_log", {}, seg, "apache_log", 2, plain),
              ("df_k1" + s, "csv2json", {}, seg, "csv", 1, plain),
              ("df_iso" + s, "iso_datetime_to_json", {}, seg, "datetime", 1, plain),
              ("gen_apache" + s, "apache_log", GENERAL, seg, "apache_log", 0, plain),
              ("gen_csv" + s, "csv2json", GENERAL, seg, "csv", 0, plain),
              ("gen_iso" + s, "iso_datetime_to_json", GENERAL, seg, "datetime", 0, plain)]
    t += [
        # k_demit's other instances: a lane takes half a piece (W = 12 and 16), rounds of whole pieces (test_instances.ROUNDS_CASES:
        # 8 waves by itself, 12 with half pieces off; at 4 waves 64 pieces of it fit one round)
        ("df_half_w12", "iso_datetime_to_json", {"emit_waves": 12, "emit_half": 2}, 0, "datetime", 1, plain),
        ("df_rounds_w4", "iso_datetime_to_json", {"emit_waves": 4}, 0, "datetime", 1, plain),
        ("df_rounds_w8", "iso_datetime_to_json", {"emit_waves": 8}, 0, "datetime", 1, plain),
        ("df_rounds_w12", "iso_datetime_to_json", {"emit_waves": 12, "emit_half": 1}, 0, "datetime", 1, plain),
        ("df_half_w16", "apache_log", {"emit_waves": 16, "emit_half": 2}, 0, "apache_log", 2, plain),
        # the general engine's layouts
        # (thousand_sep has a delayed form that its inputs leave in every segment: the engine gives the form up by itself, delay -1 here)
        ("gen_never_delayed", "thousand_sep", {}, 0, "numbers", -1, dict(plain, inl=1, direct=0)),
        ("gen_inline", ti.INLINE_PROGRAM, GENERAL, 0, "inline", 0, dict(plain, inl=1, direct=0)),
        ("gen_wide_entries", ti.WIDE_ENTRY_PROGRAM, GENERAL, 0, "wide", 0, dict(plain, general=1, direct=0)),
        ("gen_job_stride", "apache_log", dict(GENERAL, job_stride=2), 0, "apache_log", 0, dict(plain, jl=1, direct=0)),
        ("gen_big", "apache_log", dict(GENERAL, force=host.KX_FORCE_BIG), 0, "apache_log", 0, dict(plain, general=1, big=1, direct=0)),
        ("gen_init_only", INIT_ONLY, GENERAL, 0, "init", 0, dict(plain, direct=1)),
        # a coder's symbol table: translated per piece, and with a table id per entry
        ("xlat", CODER, GENERAL, 0, "coder", 0, dict(plain, inl=1, xlat=1, direct=0)),
        ("tblmode", CODER, dict(GENERAL, force=host.KX_FORCE_TBLMODE), 0, "coder", 0, dict(plain, general=1, tblmode=1, direct=0)),
        # pipelines; a last stage with register actions (its result reaches d_out through k_copy_bytes)
        # (the first stage of each has a delayed form of its own, K = 1; the later stages' layouts: LATER_STAGES)
        ("three_stages", THREE_STAGES, {}, 0, "abc", 1, dict(plain, inl=1, direct=0)),
        ("late_reject", LATE_REJECT, {}, 0, "late", 1, dict(plain, direct=1)),
        ("actions", PROGRAMS["swap_fields"], {}, 0, "swap", 1, dict(plain, direct=1)),
        # escaped quotes: k_dforward's slow path replays the stretch (hole lanes write into `out`); with the slow path off the shard
        # falls back to the general engine, every time (df_backoff = 1: no shard skips the form)
        ("holes_slow", "apache_log", {"df_backoff": 1}, 64, "holes", 2, plain),
        ("holes_fall_back", "apache_log", {"disable": host.KX_OFF_SLOW, "df_backoff": 1}, 64, "holes", 2, plain),
    ]
    return [Route(*r) for r in t]


ROUTES = _routes()
# the stages behind the first one: (layout flags, has a delayed form); the last of them writes d_out
_INLINE = {"general": 0, "big": 0, "inl": 1, "jl": 0, "direct": 0, "xlat": 0, "tblmode": 0}
LATER_STAGES = {"three_stages": [(_INLINE, 1), (_INLINE, 1)], "late_reject": [(_INLINE, 1)]}
ROUTE = {r.name: r for r in ROUTES}
NAMES = [r.name for r in ROUTES]
# the language of each input table: residues of the result's length modulo 16 it can give; whether it has lines (a cut rejects)
ODD = frozenset(range(1, 16, 2))
ALL16 = frozenset(range(16))
TABLES = {"apache_log": (ALL16, True), "csv": (ALL16, True), "datetime": (ALL16, True), "numbers": (ALL16, True), "inline": (ALL16, False),
          "wide": (ALL16, False), "init": (ALL16, False), "coder": (ODD, False), "abc": (ALL16, True), "late": (ALL16, False),
          "swap": (ALL16, True), "holes": (ALL16, True)}
TABLE_PROGRAM = {}
for _r in ROUTES:
    assert TABLE_PROGRAM.setdefault(_r.table, _r.prog) == _r.prog      # (a table belongs to one program: its results are shared)


@functools.lru_cache(maxsize=None)
def blob(prog):
    return host.compile_regex(prog[3:]) if prog.startswith("re:") else blob_of(prog)


def config(route):
    """the kx_config the route's Program is loaded with (nothing from the environment), and the describe calls are asked about"""
    return host.config_from_env({}, **route.fields)


def expect(prog, data):
    """the oracle's bytes, or ("fail", position, stage)"""
    try:
        return oracle.run(blob(prog), data)
    except oracle.OracleMatchError as e:
        return ("fail", e.pos, e.stage)


# ----------------------------------------------------------------------------------------------------------------- the routes
def _flags(info):
    return {"general": info.general, "big": info.big, "inl": info.t.inl, "jl": info.t.jl, "direct": info.t.direct, "xlat": int(info.t.xlat != 0),
            "tblmode": info.t.tblmode}


def last_stage(route):
    import kxp
    return len(kxp.parse(blob(route.prog))) - 1


@pytest.mark.parametrize("name", NAMES)
def test_layout_and_engine_of_the_route(name):
    r = ROUTE[name]
    info = host.stage_describe(blob(r.prog), 0, cfg=config(r), with_image=False)[0]
    got = _flags(info)
    assert {k: got[k] for k in r.flags} == r.flags, (name, got)
    d = host.df_describe(blob(r.prog), cfg=config(r), with_image=False)[0]
    if r.delay is not None:
        assert bool(info.has_df) == bool(r.delay), (name, info.has_df, d.reason)
        if r.delay > 0:
            assert d.available == 1 and d.delay == r.delay, (name, d.delay, d.reason)
    if name == "gen_never_delayed":      # by the engine's own judgement at run time, not by a switch: a digit may begin a group of three or not
        assert r.fields == {} and d.available == 1 and d.escapes > 0 and d.escapes_start > 0
    if name.startswith("holes"):
        assert d.escapes_start > 0, "apache_log has lost its undecided contexts: the hole routes prove nothing"
        sl = host.stage_describe(blob(r.prog), 0, cfg=config(r), with_image=False)[0].d.sl_on
        assert bool(sl) == (name == "holes_slow")
    if name == "gen_wide_entries":
        assert ti.layout_facts(blob(r.prog))["widest"] >= 127
    if name == "gen_init_only":
        assert expect(r.prog, b"") == b"<<" == expect(r.prog, b"xxx") and info.has_df == 0
    nst = last_stage(r) + 1
    assert nst == {"three_stages": 3, "late_reject": 2}.get(name, 1)
    later = [host.stage_describe(blob(r.prog), st, cfg=config(r), with_image=False)[0] for st in range(1, nst)]
    assert [(_flags(i), int(i.has_df)) for i in later] == LATER_STAGES.get(name, []), (name, [(_flags(i), i.has_df) for i in later])
    acts = [host.stage_describe(blob(r.prog), st, cfg=config(r), with_image=False)[0].actions for st in range(nst)]
    assert [bool(a) for a in acts] == [name == "actions"] * nst, (name, acts)


def test_every_output_kernel_family_has_a_route():
    kinds = collections.Counter()
    for r in ROUTES:
        info = host.stage_describe(blob(r.prog), 0, cfg=config(r), with_image=False)[0]
        kinds["delayed K=%d" % r.delay if r.delay and r.delay > 0 else "big" if info.big else "job-stride" if info.t.jl else "general" if info.general else
              "ext" if info.t.inl or info.t.xlat else "plain"] += 1
    assert set(kinds) >= {"delayed K=1", "delayed K=2", "plain", "ext", "general", "job-stride", "big"}, kinds
    pairs = [n for n in NAMES if n.endswith("_seg64")]
    assert len(pairs) == 6 and all(ROUTE[n].seg == 64 and ROUTE[n[:-6]].seg == 0 and ROUTE[n[:-6]].fields == ROUTE[n].fields for n in pairs)


# ----------------------------------------------------------------------------------------------------------------- the inputs
HOLE = b'\\"   5x HTTP/'


def _units(table):
    """the table's language as a list of pieces of input any prefix of which (joined) the program accepts"""
    r = random.Random(20240 + sorted(TABLES).index(table))
    if table in ("apache_log", "csv", "datetime", "numbers"):
        return [ln + b"\n" for ln in workloads.generate(table, 56 * 1024, 61).split(b"\n")[:-1]]
    if table == "holes":
        lines = [ln + b"\n" for ln in workloads.generate("apache_log", 56 * 1024, 62).split(b"\n")[:-1]]
        at, marks = 0, []
        for i, ln in enumerate(lines):          # an escaped quote in the request field: early (within the first 4 KiB), and every 5 KiB or so
            if at + len(ln) < 2048 and not marks or marks and at > marks[-1] + 5 * 1024:
                assert b" HTTP/" in ln
                lines[i] = ln.replace(b" HTTP/", HOLE, 1)
                marks.append(at)
            at += len(ln)
        return lines
    if table == "swap":
        return [bytes(r.choice(b"abcxyz") for _ in range(r.randint(0, 9))) + b"," + str(r.randint(0, 10 ** r.randint(1, 8))).encode() + b"\n"
                for _ in range(5000)]
    if table == "abc":
        return [b"abc"] * 16000
    alphabet = {"inline": b"abcdefgh,\n", "wide": b"bbbbbbbbbbbbbbbbbbbbbbbbbbbbbbac", "init": b"xxxy", "coder": b"abcd", "late": b"xab\nxw"}[table]
    return [bytes([r.choice(alphabet)]) for _ in range(46 * 1024)]


def _tiny(table):
    """inputs beside the prefixes: results of a few bytes"""
    if table == "inline":
        return [b"," * k for k in range(1, 16)]           # (a comma becomes one byte: results of 1 … 15 bytes)
    if table == "init":
        return [b"x" * 70, b"x" * 4096, b"x" * 5000 + b"y"]   # (nothing but the init copy's two bytes; one byte from the last piece)
    if table == "coder":
        return [b"abcd"[:k] for k in range(1, 5)]
    if table == "csv":
        return [ti.exact_input("csv", n, 3) for n in (14, 20, 63)]     # (the shortest row there is, and stretched ones)
    if table == "wide":
        return [b"b" * k for k in (1, 7, 15)] + [b"a", b"c" * 64 + b"a" * 64]
    return []


def _edge_sizes(table):
    """the three lengths around 4 KiB: n % 64 of 0 (a whole last piece), 1 and 63; the nearest to 4096 that the language has"""
    unit = 3 if table == "abc" else 1                  # ("abc" over and over: multiples of 3 alone)
    return [min((n for n in range(3072, 5121) if n % PIECE == r and n % unit == 0), key=lambda n: abs(n - 4096)) for r in (0, 1, 63)]


def _exact(table, n, whole, ends):
    """an accepted input of exactly n bytes (around 4 KiB): whole lines, the last of them stretched to fit where lines vary"""
    if table in ("apache_log", "csv", "datetime"):
        return ti.exact_input(table, n, 7)
    if table == "holes":                               # (a log of 7 bytes fewer, and the escaped quote into its first line)
        d = ti.exact_input("apache_log", n - (len(HOLE) - len(b" HTTP/")), 7)
        assert b" HTTP/" in d[:d.index(b"\n")]
        return d.replace(b" HTTP/", HOLE, 1)
    if n in ends:                                      # (units of one byte, or of three)
        return whole[:n]
    r = random.Random(n)
    e = max(e for e in ends if e <= n - 3)             # whole lines, then one line of the n - e bytes that are left
    if table == "numbers":                             # (1 to 1000 digits, as workloads.numbers_line has them)
        assert n - e <= 1001
        return whole[:e] + bytes(r.choice(b"0123456789") for _ in range(n - e - 1)) + b"\n"
    assert table == "swap"
    return whole[:e] + bytes(r.choice(b"abcxyz") for _ in range(n - e - 3)) + b",7\n"


Input = collections.namedtuple("Input", "group data want")      # group: "small", "4k", "40k" or "reject"; want: bytes or ("fail", pos, stage)


def _damage(prog, data, positions):
    """`data` with one byte replaced so that the oracle rejects it: the first (position, byte) that does"""
    for pos in positions:
        for b in (0, 0xFF, ord("z"), ord("\n"), ord('"')):
            if data[pos] != b:
                bad = data[:pos] + bytes([b]) + data[pos + 1:]
                if isinstance(expect(prog, bad), tuple):
                    return bad
    return None


@functools.lru_cache(maxsize=None)
def inputs(table):
    """the table's inputs, accepted ones first; built from the oracle alone"""
    prog = TABLE_PROGRAM[table]
    units = _units(table)
    ends = [0]
    for u in units:
        ends.append(ends[-1] + len(u))
    whole = b"".join(units)
    out, seen, res = [], set(), set()

    def add(group, data):
        if data in seen:
            return None
        want = expect(prog, data)
        assert isinstance(want, bytes), (table, group, len(data), want)
        seen.add(data)
        res.add(len(want) % 16)
        out.append(Input(group, data, want))
        return want

    # under 64 bytes: the empty input, every prefix below 64 bytes up to four of them, else the shortest there is
    if isinstance(expect(prog, b""), bytes):
        add("small", b"")
    else:                                       # (csv2json wants its header line: the empty input is a rejected one)
        seen.add(b"")
        out.append(Input("reject", b"", expect(prog, b"")))
    for e in [e for e in ends[1:] if e < PIECE][:4]:
        add("small", whole[:e])
    for d in _tiny(table):
        add("small" if len(d) < PIECE else "4k", d)
    if not any(i.data for i in out if i.group == "small"):
        add("small", min(units, key=len))          # (a log line has 81 bytes and more)
    # around 4 KiB: n % 64 of 0, 1 and 63, then prefixes, those nearest to 4 KiB first, until the residues are covered (at most 32 KiB)
    for n in _edge_sizes(table):
        data = _exact(table, n, whole, ends)
        assert len(data) == n, (table, n, len(data))
        add("4k", data)
    for e in sorted((e for e in ends if 1024 <= e <= 32 * 1024), key=lambda e: abs(e - 4096)):
        if res >= TABLES[table][0]:
            break
        data = whole[:e]
        if data not in seen and len(expect(prog, data)) % 16 not in res:
            add("4k", data)
    # around 40 KiB
    for lo in (36 * 1024, 40 * 1024 + 1, 44 * 1024):
        add("40k", whole[:next(e for e in ends if e >= lo)])
    # rejected variants of one input per group
    bases = [next(i for i in reversed(out) if i.group == g and len(i.data) > 0) for g in ("small", "4k", "40k")]
    for b in bases:
        n = len(b.data)
        last = (n - 1) // PIECE * PIECE
        variants = [_damage(prog, b.data, [0]), _damage(prog, b.data, [p for p in range(n - 1, max(last, 1) - 1, -1)])]
        if TABLES[table][1]:
            variants.append(next((b.data[:n - k] for k in range(1, min(n, 40)) if isinstance(expect(prog, b.data[:n - k]), tuple)), None))
        for v in variants:
            if v is not None and v not in seen:
                seen.add(v)
                out.append(Input("reject", v, expect(prog, v)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rejected_byte(table):
    """a byte other than 0 that the program rejects where it stands: alone (at position 0), over and over, and behind an accepted input"""
    prog = TABLE_PROGRAM[table]
    acc = next(i.data for i in inputs(table) if i.group == "small" and i.data)
    for b in (0xFF, 0x80, ord("z"), ord('"'), 1):
        f = bytes([b])
        got = [expect(prog, d) for d in (f, f * PIECE, acc + f, acc + f * PIECE)]
        if all(isinstance(g, tuple) for g in got) and got[0][1] == 0 and got[2][1] >= len(acc):
            return f
    return None


def order(table, seed):
    """the table's inputs in a shuffled order, a rejected one after every few accepted ones"""
    acc = [i for i in inputs(table) if i.group != "reject"]
    rej = [i for i in inputs(table) if i.group == "reject"]
    r = random.Random(seed)
    r.shuffle(acc)
    r.shuffle(rej)
    step = max(1, len(acc) // max(1, len(rej)))
    out = []
    for k, a in enumerate(acc):
        out.append(a)
        if k % step == step - 1 and rej:
            out.append(rej.pop())
    return out + rej


@pytest.mark.parametrize("table", sorted(TABLES))
def test_populations_of_the_table(table):
    ins = inputs(table)
    acc = [i for i in ins if i.group != "reject"]
    residues, lines = TABLES[table]
    assert {len(i.want) % 16 for i in acc} == set(residues), (table, sorted({len(i.want) % 16 for i in acc}))
    groups = collections.Counter(i.group for i in ins)
    assert groups["small"] >= 2 and groups["4k"] >= 3 and groups["40k"] == 3, groups
    assert all(len(i.data) < PIECE or len(i.data) == min(len(j.data) for j in acc if j.data) for i in acc if i.group == "small")
    assert all(1024 <= len(i.data) <= 32 * 1024 or table in ("wide", "init") for i in acc if i.group == "4k")
    assert sum(3 * 1024 <= len(i.data) <= 5 * 1024 for i in acc if i.group == "4k") >= 3
    assert all(36 * 1024 <= len(i.data) <= 46 * 1024 for i in acc if i.group == "40k")
    # a whole last piece, one byte into the next and one byte short of it, each within 1 KiB of 4 KiB: every language here has all three
    assert {0, 1, 63} <= {len(i.data) % PIECE for i in acc if i.group == "4k" and 3072 <= len(i.data) <= 5120}, table
    # rejected variants: at byte 0, inside the last piece (the oracle stops there, or before), cut in mid-line
    rej = [i for i in ins if i.group == "reject"]
    assert all(isinstance(i.want, tuple) and i.want[0] == "fail" for i in rej)
    assert any(i.want[1] == 0 for i in rej), table
    if table != "late":       # (a later stage's position counts that stage's input)
        assert any(len(i.data) > 1024 and i.want[1] // PIECE == (len(i.data) - 1) // PIECE for i in rej), table
    if lines:
        assert any(i.want[1] == len(i.data) and i.data == j.data[:len(i.data)] for i in rej for j in acc if len(j.data) > len(i.data)), table
    assert len(rej) >= (8 if lines else 5), (table, len(rej))
    if table == "late":
        assert any(i.want[2] == 1 for i in rej) and any(i.want[2] == 1 and len(i.data) > 36 * 1024 for i in rej)
    else:
        assert all(i.want[2] == 0 for i in rej)
    if table == "holes":
        for i in acc:
            if len(i.data) > 12 * 1024:
                assert HOLE[:2] in i.data[:4096] and HOLE[:2] in i.data[4096:], len(i.data)
            elif len(i.data) >= 2048:
                assert HOLE[:2] in i.data
        assert sum(i.data.count(HOLE[:2]) for i in acc if i.group == "40k") >= 9
    # the junk around the input: a rejected byte that is not the zero filling, nor the first byte of the filling that goes on validly
    bad = rejected_byte(table)
    assert bad is not None and bad != b"\0" and bad != next(i.data for i in acc if i.group == "40k")[:1], (table, bad)
    if table == "coder":                                   # two code bytes per symbol and one for the end: never an even length
        assert all(len(i.want) == 2 * len(i.data) + 1 for i in acc)
    for seed in (1, 2):
        o = order(table, seed)
        assert sorted(o) == sorted(ins)
        first_rej = next(k for k, i in enumerate(o) if i.group == "reject")
        assert any(i.group != "reject" for i in o[first_rej:]), "no accepted input runs after a rejected one"
    assert order(table, 1) != order(table, 2)


def test_results_of_0_and_of_1_to_15_bytes_occur():
    lens = {len(i.want) for t in TABLES for i in inputs(t) if i.group != "reject"}
    assert set(range(16)) <= lens, sorted(set(range(16)) - lens)


def test_every_route_has_its_table():
    assert {r.table for r in ROUTES} == set(TABLES)
    for r in ROUTES:
        assert TABLE_PROGRAM[r.table] == r.prog
