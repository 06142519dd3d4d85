"""GPU: generated programs and swept cut points across the shard seam — the kernels and host paths that run only there (k_head,
k_dhead, k_dmap, k_shard_map, dfFallBack with a head, the delayed form's seam routes) and k_sync, whose result no other test can see.

  a. test_ranks_*      shardcuts.run_shards, one Program per shard, both engines, every plan of test_shard_seam.cases()
  b. test_windows_*    shardcuts.run_windows (FdStream::push restated), one Program, df_backoff 0 and 1; which seam route ran is read
                       from the lines the library prints under KX_DEBUG
  c. test_seam_populations   how often each route and each head class was reached on the device, against floors
  d. test_c_driver_on_generated_programs                    kx_run_sharded, ranks = threads
  e. test_produced_binary_windows_on_generated_programs     a produced binary in windows of 4 KiB (the one place where action stages
                                                            meet the seam)

Everything is compared byte for byte with the CPU oracle on the same blob, or with a plain restatement: the state of a sequential DFA
run (shardcuts.Truth), the bytes every step writes (Truth.own_bytes; validated against kxp.CpuShard in test_shard_seam.py), and
k_sync's figures (shardcuts.predict_forward).  All runs use 64-byte segments; one plan per program also runs at 4 096, at the
engine's own choice and in workgroups of 64 lanes (ranks), or at 256, 4 096 and the engine's own (windows: WINDOW_CONFIGS, with the
escaping cuts and the hand-built cases).  A program is left out only by a counted rule (it does not compile, its path tree
is too large, the engine refuses it); no case is skipped on a mismatch."""
import os
import re

import pytest
import shardcuts as sc
import test_random_inputs as tr
import test_shard_seam as ts
from conftest import blob_of
from test_instances_gpu import demit_lines, log  # noqa: F401  (log: the fixture)
from test_random_inputs_gpu import MODE_ENV, load, reset

from kleenexlang_amd import MatchError, Program, host
from oracle import oracle

pytestmark = pytest.mark.gpu

NCHUNK = 12
CHUNKS = [range(c, tr.NPROG, NCHUNK) for c in range(NCHUNK)]
SEG64 = {"segment_bytes": 64}
# (segment_bytes, block_threads, the segment size that results) for the one plan per program that runs in other configurations too
OTHER_CONFIGS = ((4096, 0, 4096), (0, 0, 4096), (64, 64, 64))      # (the engine's own choice is never below 4 096 bytes)

ROUTES = ("kept", "head", "outside", "unsettled", "open_to_end", "armed_later")
_ROUTE_TEXT = {"head": "a context that the delay does not decide (head)", "outside": "the incoming state is outside the table",
               "unsettled": "the start-leaf map does not settle", "open_to_end": "stays open to the end of the input"}
_FALLS_BACK = re.compile(r"\[kx\] delayed form: (.*?); stage (\d+) falls back to the general engine")
_ARMS = "arms the slow path of its forward pass"
HEAD_CLASSES = ("head", "head_crosses_piece", "head_whole_shard", "reject_in_head", "reject_in_last_byte")
COUNTS = {"routes": dict.fromkeys(ROUTES, 0), "heads": dict.fromkeys(HEAD_CLASSES, 0), "ranks_runs": 0, "windows_runs": 0,
          "programs": {"plain": 0, "wide": 0}, "refused": {"plain": 0, "wide": 0}}


def expect_of(src, data):
    try:
        return oracle.run(blob_of(src, 3), data)
    except oracle.OracleMatchError as e:
        return ("fail", e.pos)


# ------------------------------------------------------------------------------------------------------------ a. ranks
def check_ranks(got, src, data, plan, want, mode, seg, where, bad, count=True):
    """one run of run_shards against the oracle, Truth and (general engine) k_sync's restatement; mismatches go to `bad`"""
    truths = ts.truths_of(src, data)
    res = got["result"]
    if isinstance(want, bytes):
        if res != want:
            bad.append(where + ("other bytes" if isinstance(res, bytes) else res,))
            return
        if sum(r["out_len"] for r in got["shards"][-1]) != len(want):
            bad.append(where + ("the lengths do not add up",))
    elif res[:2] != want:
        bad.append(where + (res, want))
        return
    heads = dict.fromkeys(HEAD_CLASSES, 0)
    for recs, t in zip(got["shards"], truths):
        off = sc.offsets([r["n"] for r in recs])
        if off[-1] != t.n:
            bad.append(where + ("stage", recs[0]["stage"], "reads", off[-1], "bytes, not", t.n))
            return
        for r, a, b in zip(recs, off, off[1:]):
            at = where + ("stage", r["stage"], "shard", r["index"], (a, b))
            if t.states[b] is not None and r["fixed"]["end_state"] != t.states[b]:
                bad.append(at + ("end state", r["fixed"]["end_state"], "the plain run's", t.states[b]))
            if mode != "general":
                continue
            first = r["index"] == 0
            head, synced, unsynced = sc.predict_forward(t.stage, t.data[a:b], seg, first)
            f = r["forward"]
            if (f["head_len"], f["synced"], r["unsynced"]) != (head, synced, unsynced):
                bad.append(at + ("forward", (f["head_len"], f["synced"], r["unsynced"]), "k_sync restated", (head, synced, unsynced)))
            if t.fail is None and r["bytes"] != t.own_bytes(a, b, first):
                bad.append(at + ("the shard's own bytes",))
            if r["stage"] == 0 and seg == 64 and not first and b > a and (t.fail is None or a <= t.fail):
                heads["head"] += f["head_len"] > 0
                heads["head_crosses_piece"] += f["head_len"] >= 64
                heads["head_whole_shard"] += f["head_len"] == b - a and not f["synced"]
                if t.fail is not None and a <= t.fail < a + f["head_len"]:
                    heads["reject_in_head"] = 1
            if r["stage"] == 0 and seg == 64 and b > a and t.fail == b - 1:
                heads["reject_in_last_byte"] = 1
    if count:
        for k, v in heads.items():
            COUNTS["heads"][k] += v
        COUNTS["ranks_runs"] += 1


class Pool:
    """Programs of one source and configuration, one per rank, loaded as the widest plan asks for them"""

    def __init__(self, src, env, **fields):
        self.src, self.env, self.fields, self.ps = src, env, fields, []

    def take(self, world):
        assert not sc.FAULT, sc.FAULT      # (a load allocates and uploads: none behind an engine error)
        while len(self.ps) < world:
            p = load(self.src, self.env, **self.fields)
            if p is None:
                return None
            self.ps.append(p)
        return self.ps[:world]

    def close(self):
        for p in self.ps:
            p.close()


def run_ranks(src, mode, cases, where, bad, others=None):
    """every (data, plan) of `cases` on one Program per shard; `others`: the index of the case that also runs in OTHER_CONFIGS.
    -> False where the engine refuses the program"""
    pool = Pool(src, MODE_ENV[mode])
    try:
        if pool.take(2) is None:
            return False
        for j, (data, plan) in enumerate(cases):
            want = expect_of(src, data)
            for segb, bt, seg in ((64, 0, 64),) + (OTHER_CONFIGS if j == others else ()):
                ps = pool.take(len(plan))
                for p in ps:
                    reset(p)
                got = sc.run_shards(ps, sc.split(data, list(plan)), {"segment_bytes": segb, "block_threads": bt})
                check_ranks(got, src, data, plan, want, mode, seg, where + (mode, len(data), plan, (segb, bt)), bad)
                if mode == "general" and any(p.stage_delayed_form(0) for p in ps):
                    bad.append(where + ("the general engine was asked for",))
        return True
    finally:
        pool.close()


_RANKS = {}


def ranks_chunk(kind, mode, chunk):
    key = (kind, mode, chunk)
    if key in _RANKS:
        return _RANKS[key]
    bad, ran = [], 0
    for seed in CHUNKS[chunk]:
        src = tr.source(kind, seed)
        if src is None:
            continue
        cases = ts.cases(kind, seed, thin=(mode == "general"))
        ok = run_ranks(src, mode, cases, (kind, seed, src), bad, others=seed % len(cases) if cases else None)
        ran += ok
        if mode == "delayed":
            COUNTS["programs" if ok else "refused"][kind] += 1
    _RANKS[key] = ran
    assert not bad, (len(bad), bad[:5])
    return ran


@pytest.mark.parametrize("chunk", range(NCHUNK))
@pytest.mark.parametrize("mode", ["delayed", "general"])
@pytest.mark.parametrize("kind", ["plain", "wide"])
def test_ranks_on_generated_programs(kind, mode, chunk):
    """One Program per shard under sharded.run_stage_local, every stage: the concatenation is the oracle's (or every rank reports
    its global failure position), the lengths add up, and the end state that fix_head reports is the plain DFA run's wherever the
    input is accepted up to the shard's end.  On the general engine (KX_DF=0) also: head_len, synced and unsynced_segments behind
    forward are k_sync's restatement, and every shard's own bytes are the steps' it holds.  By default every plan runs; the general
    engine's pass keeps of the two-part plans the cuts 1, 2, 63, 64, 65, 4 095, 4 096, 4 097 and n - 1 (the thinning the time asks for)."""
    assert ranks_chunk(kind, mode, chunk) > 0


_HAND_BUILT = {}


def test_ranks_on_hand_built_programs():
    """The parity program (every later shard is one head: k_head walks it all, and the state is chained rank by rank), the never-merging
    program (start-leaf maps that are not constant: k_shard_map and the chain of end leaves) and apache_log with an escaped quote on
    the cut (the delayed form's head meets the context), both engines, with the same assertions."""
    if "ranks" in _HAND_BUILT:
        return
    bad = []
    by_src = {}
    for name, src, data, plan in ts.hand_built_cases():
        by_src.setdefault(src, []).append((data, plan))
    for src, cases in by_src.items():
        for mode in ("delayed", "general"):
            assert run_ranks(src, mode, cases, (src[:20],), bad)
    _HAND_BUILT["ranks"] = True
    assert not bad, (len(bad), bad[:5])


# ---------------------------------------------------------------------------------------------------------- b. windows
# (segment_bytes, block_threads) of the window runs: all cases at 64; the hand-built and the escaping cases and one plan per program
# also at 256 (the smallest size used here at which the lanes of a LATER shard on the delayed form have parts of their own: a part
# starts at the next multiple of 64 behind the lane's synchronisation point + K + J, and must start inside the lane's segment — at 64
# no lane but the first shard's lane 0 has one, and a later shard is one head that k_dhead walks alone), at 4 096 and at the engine's own
WINDOW_CONFIGS = ((64, 0), (256, 0), (4096, 0), (0, 0))


def routes_of(got, p):
    """the seam routes of one run_windows run, from what the library printed per window"""
    r = dict.fromkeys(ROUTES, 0)
    fell = armed_first = False
    for recs in got["shards"]:
        for w in recs:
            text = w["log"] + w["emit_log"]
            for why, _ in _FALLS_BACK.findall(text):
                fell = True
                for k, t in _ROUTE_TEXT.items():
                    r[k] += why == t
            r["open_to_end"] += _ROUTE_TEXT["open_to_end"] in text
            if _ARMS in text:
                r["armed_later"] += w["index"] > 0
                armed_first |= w["index"] == 0
    r["kept"] = int(not fell and not armed_first and not r["armed_later"] and p.stage_delayed_form(0) == 1)
    return r


def run_windows_cases(capfd, src, cases, backoff, where, bad, form_sample=None, run_log=None, everywhere=(), context_at=None):
    """every (data, plan) of `cases` through run_windows on ONE Program (reset before each run: every run starts on the form), in
    64-byte segments; the cases whose index is in `everywhere` (True: all) in every configuration of WINDOW_CONFIGS.
    `context_at(data)`: the position of the input's first context that the delay does not decide, where one is known.  In 64-byte
    segments a later window is one head: a two-part plan whose cut lies 16 bytes and more in front of that context must leave the form
    there — the `(head)` fall-back, or `outside` where the table has no start for the incoming state."""
    assert not sc.FAULT, sc.FAULT
    p = load(src, df_backoff=backoff)
    if p is None:
        return False
    try:
        runs = [(data, plan, cfg) for j, (data, plan) in enumerate(cases)
                for cfg in (WINDOW_CONFIGS if everywhere is True or j in everywhere else WINDOW_CONFIGS[:1])]
        for data, plan, (segb, bt) in runs:
            want = expect_of(src, data)
            reset(p)
            capfd.readouterr()
            got = sc.run_windows(p, sc.split(data, list(plan)), {"segment_bytes": segb, "block_threads": bt}, tap=lambda: capfd.readouterr().err)
            at = where + (backoff, len(data), plan, (segb, bt))
            res = got["result"]
            if (res if isinstance(want, bytes) else res[:2]) != want:
                bad.append(at + ("other bytes" if isinstance(res, bytes) else res, want if isinstance(want, tuple) else len(want)))
                continue
            routes = routes_of(got, p)
            e = context_at(data) if context_at else None
            if e is not None and segb == 64 and len(plan) == 2 and 0 < plan[0] <= e - 16 and isinstance(want, bytes) and p.stage_delayed_form(0):
                if routes["head"] + routes["outside"] < 1:
                    bad.append(at + ("a context at", e, "in a later window that is one head, and no (head) fall-back", routes))
            if routes["kept"] and p.stage_delayed_form(0) == 1 and isinstance(want, bytes):
                # the form kept: every window of stage 0 that holds bytes was written by the delayed form's emit
                for w in got["shards"][0]:
                    if w["n"] and w["bytes"] is not None and len(demit_lines(w["emit_log"])) != 1:
                        bad.append(at + ("window", w["index"], "kept the form but printed no delayed-form emit line", w["emit_log"][-200:]))
            for k, v in routes.items():
                COUNTS["routes"][k] += v
            COUNTS["windows_runs"] += 1
        if form_sample is not None:
            # the next run after reset_delayed_form is on the form again
            reset(p)
            p.configure(segment_bytes=64)
            with sc.guard():
                out, err = run_log(p, form_sample)
            if out != expect_of(src, form_sample) or p.stage_delayed_form(0) != 1 or not demit_lines(err):
                bad.append(where + (backoff, "after reset_delayed_form the run is not on the form", p.stage_delayed_form(0), err[-200:]))
        return True
    finally:
        p.close()


def first_escape(kind, seed):
    """where the simulated table first escapes on the program's 8 KiB sample; None where it stays on the form or has none"""
    from test_random_inputs_gpu import _first_escape
    d = tr.sample(kind, seed, tr.LONG)
    if len(d) < tr.LONG_MIN or tr.on_the_form(kind, seed, d) is not False:
        return None
    return _first_escape(kind, seed, d)


def escape_cases(kind, seed):
    """for a program whose 8 KiB sample escapes in the simulation: two-part plans cut within 70 bytes before and after the first
    escaping byte"""
    e = first_escape(kind, seed)
    if e is None:
        return ()
    d = tr.sample(kind, seed, tr.LONG)
    return tuple((d, (c, len(d) - c)) for c in sorted({e + x for x in (-70, -64, -17, -3, -1, 0, 1, 2, 17, 64, 70)}) if 0 < c < len(d))


_WINDOWS = {}


def windows_chunk(log, capfd, kind, chunk, backoff):
    key = (kind, chunk, backoff)
    if key in _WINDOWS:
        return _WINDOWS[key]
    bad, ran = [], 0
    for seed in CHUNKS[chunk]:
        src = tr.source(kind, seed)
        if src is None:
            continue
        sample = tr.sample(kind, seed, 4097)
        on_form = len(sample) > 1 and tr.on_the_form(kind, seed, sample) is True
        cases, esc = ts.cases(kind, seed), escape_cases(kind, seed)
        e, long_sample = first_escape(kind, seed), tr.sample(kind, seed, tr.LONG)
        ran += run_windows_cases(capfd, src, cases + esc, backoff, (kind, seed, src), bad, form_sample=sample if on_form else None, run_log=log,
                                 everywhere={seed % len(cases)} | set(range(len(cases), len(cases) + len(esc))) if cases else (),
                                 context_at=lambda d: e if d is long_sample or d == long_sample else None)
    _WINDOWS[key] = ran
    assert not bad, (len(bad), bad[:5])
    return ran


@pytest.mark.parametrize("chunk", range(NCHUNK))
@pytest.mark.parametrize("backoff", [0, 1])
@pytest.mark.parametrize("kind", ["plain", "wide"])
def test_windows_on_generated_programs(log, capfd, kind, backoff, chunk):
    """FdStream::push's order on ONE Program by default (the delayed form where the stage has one), with the back-off and without
    (df_backoff = 1): window i + 1 begins in the state window i left the stage in.  The oracle's bytes or failure position; a run that
    printed no fall-back and armed nothing wrote every window of stage 0 on the form (one delayed-form emit line each); the run
    after reset_delayed_form is on the form again.  Programs whose 8 KiB sample escapes also run with the cut within 70 bytes of
    the first escaping byte.  Every plan in 64-byte segments; the escaping cuts and one plan per program also in segments of 256
    and 4 096 bytes and the engine's own (WINDOW_CONFIGS)."""
    assert windows_chunk(log, capfd, kind, chunk, backoff) > 0


def test_windows_on_hand_built_programs(log, capfd):
    """The hand-built cases as windows of one Program, in every configuration of WINDOW_CONFIGS: apache_log's one escaped quote on the
    cut (in 64-byte segments the `(head)` fall-back) and 1 500 bytes inside a later window of 20 KiB (in 256-byte segments one
    escaping lane among 80: the slow path is armed in a later window); the never-merging program with a later window beyond 65 536
    bytes (k_dmap gives up: "the start-leaf map does not settle", dfFallBack with the head walk)."""
    if "windows" in _HAND_BUILT:
        return
    bad = []
    by_src = {}
    for name, src, data, plan in ts.hand_built_cases():
        by_src.setdefault(src, []).append((data, plan))
    apache, bs = ts.apache_input()
    for src, cases in by_src.items():
        for backoff in (0, 1):
            assert run_windows_cases(capfd, src, cases, backoff, (src[:20],), bad, everywhere=True,
                                     context_at=lambda d: bs if d == apache else None)
    _HAND_BUILT["windows"] = True
    assert not bad, (len(bad), bad[:5])


# ------------------------------------------------------------------------------------------------------ c. populations
# what the device reaches on an MI355X (the line test_seam_populations prints): 18 082 rank runs, 25 254 window runs; 119 + 120 programs,
# none refused.  `unsettled` (16) and `armed_later` (6) come from the hand-built cases alone: the never-merging program with a later
# shard beyond 65 536 bytes, and apache_log's escaped quote 1 500 bytes inside a later window of 20 KiB in 256-byte segments.
MEASURED = {"routes": {"kept": 20762, "head": 1843, "outside": 659, "unsettled": 16, "open_to_end": 197, "armed_later": 6},
            "heads": {"head": 13262, "head_crosses_piece": 1307, "head_whole_shard": 1846, "reject_in_head": 417, "reject_in_last_byte": 845}}
UNREACHED = {}      # (route: why no case can reach it) — none
# four fifths of what was measured, rounded down: room for an edit of a generator or of the plans, none for a class that empties
FLOORS = {g: {k: v * 4 // 5 for k, v in m.items() if k not in UNREACHED} for g, m in MEASURED.items()}


def test_seam_populations(log, capfd):
    """How often each seam route of (b) and each head class of test_shard_seam.py was reached on the device, over all chunks and the
    hand-built programs (whatever has not run yet runs here), against FLOORS: every route and every class has one."""
    for kind in ("plain", "wide"):
        for chunk in range(NCHUNK):
            ranks_chunk(kind, "delayed", chunk)
            ranks_chunk(kind, "general", chunk)
            for backoff in (0, 1):
                windows_chunk(log, capfd, kind, chunk, backoff)
    test_ranks_on_hand_built_programs()
    test_windows_on_hand_built_programs(log, capfd)
    print("seam populations", COUNTS)
    assert COUNTS["refused"]["plain"] + (tr.NPROG - len(tr.usable_seeds("plain"))) <= tr.NPROG - tr.MEASURED["plain"]["usable"], COUNTS
    assert COUNTS["refused"]["wide"] + (tr.NPROG - len(tr.usable_seeds("wide"))) <= tr.NPROG - tr.MEASURED["wide"]["usable"], COUNTS
    for group, floors in FLOORS.items():
        for k, floor in floors.items():
            assert floor >= 1 and COUNTS[group][k] >= floor, (group, k, COUNTS[group], floor)
    assert set(FLOORS.get("routes", ())) | set(UNREACHED) == set(ROUTES) and set(FLOORS.get("heads", ())) == set(HEAD_CLASSES)



# ---------------------------------------------------------------------------------------------------------- d. C driver
def c_driver_plans(n, world):
    """two plans of `world` parts with no cut on a multiple of 2: thirds or quarters at odd positions, and tiny shards at the ends"""
    at = [0] + [(n * i // world) | 1 for i in range(1, world)] + [n]
    even = [b - a for a, b in zip(at, at[1:])]
    tiny = [1, n - 2, 1] if world == 3 else ([4096, 1, 2, n - 4099] if n >= 4099 else [1, 2, n - 4, 1])
    return [even, tiny]


def run_c_driver(blob, parts):
    import threading
    import torch
    world = len(parts)
    grp = host.Group(world)
    outs, errs = [None] * world, [None] * world

    def body(r):
        try:
            p = Program(blob)
            t = torch.frombuffer(bytearray(parts[r] or b"\0"), dtype=torch.uint8).to("cuda:0")
            out = torch.empty(p.out_capacity(sum(len(x) for x in parts), 140), dtype=torch.uint8, device="cuda:0")
            mb = grp.member(r)
            try:
                res = p.run_sharded(r, world, mb, t.data_ptr(), len(parts[r]), out.data_ptr(), out.numel())
                torch.cuda.synchronize()
                outs[r] = (int(res.out_offset), bytes(out[:int(res.out_len)].cpu().numpy().tobytes()), int(res.total_out))
            finally:
                mb.close(); p.close()
        except Exception as e:   # noqa: BLE001
            errs[r] = e
    th = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    [x.start() for x in th]; [x.join() for x in th]
    grp.close()
    return outs, errs


def test_c_driver_on_generated_programs():
    """kx_run_sharded with ranks as threads of this process (kx_group_*), world 3 and 4, on ten programs per kind (a second stage
    included where the program has one), part lengths from two unaligned plans, the 8 209-byte sample and one rejected variant: the
    concatenation, the running offsets and total_out are the oracle's; a rejection is the same global position on every rank."""
    nrun = nrej = 0
    for kind in ("plain", "wide"):
        seeds = [s for s in tr.long_seeds(kind)][:10]
        assert len(seeds) == 10
        for seed in seeds:
            src = tr.source(kind, seed)
            d = tr.sample(kind, seed, tr.LONG)
            rejected = [v for _, v in ts.overwritten(kind, seed, tr.LONG) if isinstance(tr.expect(kind, seed, v), tuple)]
            for data in [d] + rejected[seed % 4:][:1]:
                want = tr.expect(kind, seed, data)
                for world in (3, 4):
                    for plan in c_driver_plans(len(data), world):
                        assert not sc.FAULT, sc.FAULT
                        outs, errs = run_c_driver(blob_of(src, 3), sc.split(data, plan))
                        where = (kind, seed, src, len(data), plan)
                        if any(isinstance(e, host.EngineError) for e in errs):
                            sc.FAULT.append(str(errs))
                        if isinstance(want, bytes):
                            assert errs == [None] * world, where + (errs,)
                            assert b"".join(o[1] for o in outs) == want and all(o[2] == len(want) for o in outs), where
                            assert [o[0] for o in outs] == sc.offsets([len(o[1]) for o in outs])[:-1], where
                        else:
                            assert all(isinstance(e, MatchError) for e in errs) and {e.pos for e in errs} == {want[1]}, where + (errs, want)
                            nrej += 1
                        nrun += 1
    assert nrun >= 2 * 10 * 4 + nrej and nrej >= 20, (nrun, nrej)


# ----------------------------------------------------------------------------------------------------- e. the binary
BIN_TARGET = 40 * 1024


def binary_inputs(kind, seed):
    """(the 40 KiB accepted sample, a variant of it with one byte overwritten that the oracle rejects) or None where the program has
    no such pair"""
    data = tr.sample(kind, seed, BIN_TARGET)
    if len(data) < BIN_TARGET:
        return None
    for p in (20001, 12288, 30000, len(data) - 1):
        bad = data[:p] + b"\xff" + data[p + 1:]
        if isinstance(tr.expect(kind, seed, bad), tuple):
            return data, bad
    return None


def binary_programs():
    """(kind, seed): one plain program on the form, one wide program with a second stage, one with register actions, one whose
    8 KiB sample escapes — the first of each that has a 40 KiB sample and a rejected variant of it"""
    from test_random_inputs_gpu import escaping_seeds

    def first(kind, seeds, ok=lambda s: True):
        return next((kind, s) for s in seeds if ok(s) and binary_inputs(kind, s))
    return [first("plain", tr.long_seeds("plain"), lambda s: tr.on_the_form("plain", s, tr.sample("plain", s, tr.LONG)) is True),
            first("wide", tr.long_seeds("wide"), lambda s: len(ts.stages_of(tr.source("wide", s))) > 1),
            first("actions", tr.long_seeds("actions")),
            first("plain", escaping_seeds("plain"))]


def test_produced_binary_windows_on_generated_programs(tmp_path):
    """`kexc compile --out` of four generated programs, a 40 KiB accepted sample and one rejected variant through a pipe in windows
    of 4 096 bytes (KX_WINDOW_BYTES): the oracle's bytes; on the rejection exit code 1, "Match error at input symbol N!" and a
    prefix of the accepted output on stdout."""
    import subprocess
    from kleenexlang_amd import build
    assert not sc.FAULT, sc.FAULT
    kexc = os.path.join(build.OUT, "kexc")
    env = dict(os.environ, KX_WINDOW_BYTES="4096")
    env.pop("KX_DEBUG", None)
    nrej = 0
    for i, (kind, seed) in enumerate(binary_programs()):
        src = tr.source(kind, seed)
        path, exe = tmp_path / ("p%d.kex" % i), tmp_path / ("p%d" % i)
        path.write_text(src)
        assert subprocess.run([kexc, "compile", "--quiet", str(path), "--out", str(exe)]).returncode == 0, (kind, seed, src)
        data, bad = binary_inputs(kind, seed)
        want = tr.expect(kind, seed, data)
        assert isinstance(want, bytes)
        r = subprocess.run([str(exe)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0 and r.stdout == want, (kind, seed, src, r.returncode, r.stderr[-300:])
        pos = tr.expect(kind, seed, bad)[1]
        r = subprocess.run([str(exe)], input=bad, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 1 and r.stderr.endswith(b"Match error at input symbol %d!\n" % pos), (kind, seed, src, r.returncode, r.stderr[-300:])
        assert want.startswith(r.stdout), (kind, seed, src, len(r.stdout))
        nrej += 1
    assert nrej == 4
