"""Helpers of the shard-seam tests (test_shard_seam.py, test_shard_seam_gpu.py): where an input is cut, what the protocol
kx_shard_begin / forward / fix_head / backward / resolve / emit must then report, and two drivers of the Python Shard API.

  plans(n)            the cut plans for an input of n bytes
  sync_points(...)    k_sync restated over the blob's sync_next / sync_state, and the general engine's figures derived from it
  Truth               one plain DFA run and one backward walk over a whole input: the state in front of every byte, the failure
                      position, and the bytes that every single step writes (the path form gives a step's bytes to the shard that
                      holds the step, so a shard's own bytes are a slice of these)
  run_cpu             CpuShard (kxp.py) under sharded.run_stage_local, stage after stage
  run_shards          the same on the device: one Program per shard (ranks) or one Program for all of them
  run_windows         FdStream::push's order restated on ONE Program: window i + 1 begins in the stage state that window i left

No fixtures here, and nothing starts the GPU on import."""
import contextlib

import kxp

from kleenexlang_amd import sharded
from kleenexlang_amd.host import NOFAIL, EngineError

TWO_PART_CUTS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097)
THIN_CUTS = (1, 2, 63, 64, 65, 4095, 4096, 4097)     # (with n - 1: what a thinned pass keeps of the two-part plans)


def plans(n, thin=False):
    """The cut plans for an input of n bytes: lists of part lengths that sum to n.

    The rule for short inputs (n < 4100, and the cut variants of a sample): a two-part plan is kept where its cut c has 0 < c < n; a
    multi-part plan is kept where every length it computes is >= 0 (an empty part is a legal shard, a negative one is none); the plan of
    100-byte parts takes as many whole parts as fit into min(n, 2000) bytes; and a plan equal to one already listed is dropped.
    `thin`: of the two-part plans only the cuts 1, 2, 63, 64, 65, 4095, 4096, 4097 and n - 1."""
    cuts = (THIN_CUTS + (n - 1,)) if thin else (TWO_PART_CUTS + (n - 65, n - 64, n - 2, n - 1))
    out = [[c, n - c] for c in cuts if 0 < c < n]
    multi = [[4096, 1, 2, n - 4099],          # middle shards shorter than the delay and than any sync run
             [64, 0, 63, 0, n - 127],         # empty middle shards between tiny ones
             [1, n - 2, 1],
             [0, n], [n, 0]]
    # five parts cut at the odd positions (n * i // 5) | 1: unequal, and no cut on a multiple of 2
    at = [0] + [(n * i // 5) | 1 for i in range(1, 5)] + [n]
    multi.append([b - a for a, b in zip(at, at[1:])])
    # 100-byte parts over the first 2 000 bytes, the rest as one part: 20 seams, none on a piece
    k = min(n, 2000) // 100
    multi.append([100] * k + [n - 100 * k])
    out += [p for p in multi if all(x >= 0 for x in p)]
    seen, uniq = set(), []
    for p in out:
        assert sum(p) == n, (n, p)
        if tuple(p) not in seen:
            seen.add(tuple(p))
            uniq.append(p)
    return uniq


def offsets(lens):
    return [sum(lens[:i]) for i in range(len(lens) + 1)]


def split(data, plan):
    """the parts of `data` under a plan"""
    off = offsets(plan)
    return [data[a:b] for a, b in zip(off, off[1:])]


# ------------------------------------------------------------------------------------------------------ k_sync restated
MULTI = 0xFFFFFFFF          # KXP_SYNC_MULTI: several states still possible


def _lists(stage):
    """the stage's tables as Python lists (numpy scalar indexing dominates these loops otherwise), once per stage"""
    if not hasattr(stage, "_l"):
        stage._l = {"cls": stage.cls.tolist(), "delta": stage.delta.tolist(), "sync_next": stage.sync_next.tolist(),
                    "sync_state": stage.sync_state.tolist(), "pback": stage.pback.tolist(), "back": stage.back.tolist()}
    return stage._l


def sync_points(stage, data, seg, is_first):
    """Per segment k of `data` (segments of `seg` bytes): (position, state) where the segment synchronises, or None.

    include/kxp_format.h: subset 0 of the synchronising automaton is "every state"; sync_next[subset][class] is the subset after one
    byte; sync_state[subset] is the state of a singleton subset, or KXP_SYNC_MULTI (several states still possible), KXP_SYNC_EMPTY (every
    start state has failed); a sync_next entry may be KXP_SYNC_UNKNOWN (the construction was capped there) and then names no subset.
    The comment above k_sync: segment k starts at byte k * seg with an unknown state and runs the automaton inside its own bytes; one
    that does not converge there is unsynchronised.  So: from subset 0 at byte k * seg, one byte at a time and never past
    min((k + 1) * seg, n); the first singleton gives (the position behind the byte that decided it, its state); an empty or capped
    subset, or the segment's end with several states left, gives None.  A start subset that is a singleton already (a one-state
    program) synchronises at k * seg.  Segment 0 of a first shard is (0, q0) by definition."""
    L = _lists(stage)
    cls, nxt, sst = L["cls"], L["sync_next"], L["sync_state"]
    n = len(data)
    out = []
    for k in range((n + seg - 1) // seg if n else 0):
        if k == 0 and is_first:
            out.append((0, stage.q0))
            continue
        pos, limit, sid = k * seg, min((k + 1) * seg, n), 0
        st = sst[0]
        while st == MULTI and pos < limit:
            sid = nxt[sid][cls[data[pos]]]
            pos += 1
            st = sst[sid] if sid < len(sst) else sid      # (KXP_SYNC_UNKNOWN names no subset)
        out.append((pos, st) if st < kxp.NO_STATE else None)
    return out


def predict_forward(stage, data, seg, is_first):
    """What kx_shard_forward of the GENERAL engine reports for this shard: (head_len, synced, unsynced_segments).  The head is what lies
    before the first synchronised position (the whole shard where there is none); a first shard has no head and knows its end; an empty
    shard has nothing to scan."""
    pts = sync_points(stage, data, seg, is_first)
    if is_first or not data:
        return 0, 1 if is_first else 0, pts.count(None)
    found = [p for p in pts if p is not None]
    return (found[0][0] if found else len(data)), 1 if found else 0, pts.count(None)


# ------------------------------------------------------------------------------------------------- the whole input, once
class Truth:
    """One stage on one whole input, sequentially: states[i] in front of byte i (None behind a failure), fail (None, or the position
    as the engines report it: the first byte with no transition, or n where the input ends in a non-final state), and — where the input
    is accepted — init (what the start leaf writes before the first byte), piece[i] (what step i writes) and out."""

    def __init__(self, stage, data):
        L = _lists(stage)
        cls, delta = L["cls"], L["delta"]
        n = len(data)
        self.stage, self.data, self.n = stage, data, n
        self.states = [None] * (n + 1)
        self.fail = None
        q = stage.q0
        for i, b in enumerate(data):
            self.states[i] = q
            q = delta[q][cls[b]]
            if q == kxp.NO_STATE:
                self.fail = i
                break
        else:
            self.states[n] = q
            if stage.fin_leaf[q] == kxp.NO_LEAF:
                self.fail = n
        self.init = self.piece = self.out = None
        if self.fail is None:
            pback, back, t = L["pback"], L["back"], stage
            leaf, piece = int(stage.fin_leaf[q]), [b""] * n
            for i in range(n - 1, -1, -1):
                e = back[pback[self.states[i]][cls[data[i]]]][leaf]
                assert e != 0xFFFFFFFF
                tb, pc = (e >> 24, (e >> 9) & 0x7FFF) if t.tables is not None else (0, e >> 9)
                c = t.pool[t.pconst_off[pc]:t.pconst_off[pc + 1]]
                piece[i] = (bytes([int(t.tables[tb - 1, data[i]]) if tb else data[i]]) + c) if e & 0x100 else c
                leaf = e & 0xFF
            ic = int(stage.init_const[leaf])
            self.init, self.piece = t.pool[t.pconst_off[ic]:t.pconst_off[ic + 1]], piece
            self.out = self.init + b"".join(piece)

    def own_bytes(self, a, b, first):
        return (self.init if first else b"") + b"".join(self.piece[a:b])


def truths(stages, data):
    """Truth of every stage that is reached: stage s + 1 reads what stage s wrote"""
    out = []
    for st in stages:
        out.append(Truth(st, data))
        if out[-1].fail is not None:
            break
        data = out[-1].out
    return out


# -------------------------------------------------------------------------------------------------------------- drivers
def _fwd(s):
    return {"synced": int(s.synced), "end_state": int(s.end_state), "head_len": int(s.head_len),
            "fail_pos": None if s.fail_pos == NOFAIL else int(s.fail_pos)}


class _Recorder:
    """a shard under sharded.stage_protocol that keeps what forward and fix_head reported"""

    def __init__(self, shard, rec):
        self.s, self.rec = shard, rec

    def forward(self):
        r = self.s.forward()
        self.rec["forward"] = _fwd(r)
        return r

    def fix_head(self, incoming):
        r = self.s.fix_head(incoming)
        self.rec["fixed"] = _fwd(r)
        return r

    def backward(self):
        return self.s.backward()

    def resolve(self, end_leaf):
        return self.s.resolve(end_leaf)


def _record(stage, index, n):
    return {"stage": stage, "index": index, "n": n, "forward": None, "fixed": None, "unsynced": None, "out_len": None, "bytes": None, "log": "", "emit_log": ""}


def run_cpu(stages, parts):
    """CpuShard for every part (bytes), stage after stage -> {"shards": [[record per shard] per stage], "result": bytes | ("fail", pos, stage)}"""
    datas = list(parts)
    world, log = len(parts), []
    for si, st in enumerate(stages):
        recs = [_record(si, i, len(d)) for i, d in enumerate(datas)]
        shards = [kxp.CpuShard(st, d, i == 0, i == world - 1) for i, d in enumerate(datas)]
        res = sharded.run_stage_local([_Recorder(s, r) for s, r in zip(shards, recs)], [len(d) for d in datas])
        log.append(recs)
        if res[0][0] == "fail":
            assert all(r == res[0] for r in res), res
            return {"shards": log, "result": ("fail", res[0][1], si)}
        datas = [s.emit() for s in shards]
        for r, d, x in zip(recs, datas, res):
            assert x[1] == len(d) and x[3] == sum(len(y) for y in datas)
            r["out_len"], r["bytes"] = len(d), d
    return {"shards": log, "result": b"".join(datas)}


FAULT = []     # an EngineError in a run of these drivers: after it nothing here starts anything on the GPU again


@contextlib.contextmanager
def guard():
    assert not FAULT, ("an earlier run ended in an engine error: nothing more is started on the GPU", FAULT)
    try:
        yield
    except EngineError as e:
        FAULT.append(str(e))
        raise


def _align16(x):
    return (x + 15) & ~15


def _upload(datas):
    """every part at a 16-byte-aligned offset of ONE fresh device tensor (a gap of 16 bytes and more between them) -> [(tensor, n)]"""
    import torch
    offs, total = [], 0
    for d in datas:
        offs.append(total)
        total += _align16(len(d)) + 16
    host = bytearray(total)
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = d
    t = torch.frombuffer(host, dtype=torch.uint8).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return [(t[o:o + _align16(len(d)) + 16], len(d)) for o, d in zip(offs, datas)]


def _out_slices(lens):
    """a fresh device tensor with a 16-byte-aligned slice per output; an empty output gets none (and gives an empty shard)"""
    import torch
    offs, total = [], 0
    for n in lens:
        offs.append(total)
        total += _align16(n) + 16
    t = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    assert t.data_ptr() % 16 == 0
    return t, [t[o:o + _align16(n) + 16] for o, n in zip(offs, lens)]


def run_shards(progs, parts, engine_env=None):
    """The Python Shard API under sharded.run_stage_local.  `progs`: a list with one Program per shard (ranks), or ONE Program for all
    shards.  `engine_env`: run-time fields for Program.configure (segment_bytes, block_threads).  Stage s + 1's shards are stage s's
    per-shard outputs as they lie on the device.  -> as run_cpu, with "unsynced" (kx_shard_stats) in every record."""
    world = len(parts)
    ps = list(progs) if isinstance(progs, (list, tuple)) else [progs] * world
    assert len(ps) == world
    log, live = [], []
    with guard():
        try:
            for p in set(ps):
                p.configure(**(engine_env or {}))
            ins = _upload(parts)
            for si in range(ps[0].num_stages):
                recs = [_record(si, i, n) for i, (_, n) in enumerate(ins)]
                live = [ps[i].shard_begin(si, t.data_ptr(), n, i == 0, i == world - 1) for i, (t, n) in enumerate(ins)]
                res = sharded.run_stage_local([_Recorder(s, r) for s, r in zip(live, recs)], [n for _, n in ins])
                log.append(recs)
                for r, s in zip(recs, live):
                    r["unsynced"] = int(s.stats().unsynced_segments)
                if res[0][0] == "fail":
                    assert all(r == res[0] for r in res), ("the ranks disagree on the failure", res)
                    return {"shards": log, "result": ("fail", res[0][1], si)}
                lens = [x[1] for x in res]
                assert [x[2] for x in res] == offsets(lens)[:-1] and all(x[3] == sum(lens) for x in res), ("running offsets", res)
                whole, outs = _out_slices(lens)
                for s, o, n in zip(live, outs, lens):
                    s.emit(o.data_ptr(), n)
                host = whole.cpu().numpy()       # (synchronises: every shard emitted on the null stream)
                base = whole.data_ptr()
                for r, o, n in zip(recs, outs, lens):
                    a = o.data_ptr() - base
                    r["out_len"], r["bytes"] = n, host[a:a + n].tobytes()
                for s in live:
                    s.end()
                live, ins = [], list(zip(outs, lens))
            return {"shards": log, "result": b"".join(r["bytes"] for r in log[-1])}
        finally:
            for s in live:
                s.end()


def run_windows(prog, parts, engine_env=None, tap=None):
    """FdStream::push restated on ONE Program.  Every window in turn: begin -> forward -> fix_head(the end state the window before
    left); a failure ends the run at consumed + fail_pos; -> backward.  A window that reports a constant start-leaf map settles every
    window pending before it, the last window settles all: ends[j] = start_leaf of window j + 1 at (0 where that map is constant, else
    ends[j + 1]); the settled windows are resolved, emitted and ended in order, and each output enters the next stage as a window of its
    own — an empty output only where it is the last.  -> as run_shards; the records of a stage in the order its windows began.
    `tap`: called behind a window's backward and behind its emit; what it returns (what the library printed since) is kept in the
    window's record as "log" and "emit_log"."""
    import torch
    nst = prog.num_stages
    log = [[] for _ in range(nst)]
    q = [{"pend": [], "end_state": 0, "first": True, "consumed": 0} for _ in range(nst)]
    final = []

    class Fail(Exception):
        pass

    def push(st, t, n, last):
        sq = q[st]
        rec = _record(st, len(log[st]), n)
        log[st].append(rec)
        sh = prog.shard_begin(st, t.data_ptr(), n, sq["first"], last)
        w = {"sh": sh, "in": t, "n": n, "rec": rec, "bs": None}
        sq["pend"].append(w)
        rec["forward"] = _fwd(sh.forward())
        fs = sh.fix_head(0 if sq["first"] else sq["end_state"])
        rec["fixed"] = _fwd(fs)
        rec["unsynced"] = int(sh.stats().unsynced_segments)
        if fs.fail_pos != NOFAIL:
            rec["log"] = tap() if tap else ""
            raise Fail(sq["consumed"] + int(fs.fail_pos), st)
        sq["end_state"], sq["first"] = int(fs.end_state), False
        sq["consumed"] += n
        bs = sh.backward()
        w["bs"] = (int(bs.constant), bytes(bs.start_leaf))
        rec["constant"] = w["bs"][0]
        rec["log"] = tap() if tap else ""
        pend = sq["pend"]
        nres = len(pend) if last else (len(pend) - 1 if w["bs"][0] else 0)
        if nres == 0:
            assert len(pend) <= 64, "the output stays undetermined across more than 64 windows"
            return
        ends = [0] * len(pend)
        for j in range(nres - 1, -1, -1):
            if j + 1 < len(pend):
                const, leaf = pend[j + 1]["bs"]
                ends[j] = leaf[0 if const else ends[j + 1]]
        for j in range(nres):
            r = pend[j]
            rlast = last and j + 1 == len(pend)
            ol = r["sh"].resolve(ends[j])
            out = torch.empty(_align16(ol) + 16, dtype=torch.uint8, device="cuda:0")
            r["sh"].emit(out.data_ptr(), ol)
            r["rec"]["out_len"], r["rec"]["bytes"] = ol, out[:ol].cpu().numpy().tobytes()
            r["sh"].end()
            r["sh"] = r["in"] = None
            r["rec"]["emit_log"] = tap() if tap else ""
            if st + 1 < nst:
                if ol or rlast:
                    push(st + 1, out, ol, rlast)
            else:
                final.append(r["rec"]["bytes"])
        del pend[:nres]

    with guard():
        try:
            prog.configure(**(engine_env or {}))
            ins = _upload(parts)
            try:
                for i, (t, n) in enumerate(ins):
                    push(0, t, n, i == len(ins) - 1)
            except Fail as e:
                return {"shards": log, "result": ("fail",) + e.args}
            return {"shards": log, "result": b"".join(final)}
        finally:
            for sq in q:
                for w in sq["pend"]:
                    if w["sh"] is not None:
                        w["sh"].end()
