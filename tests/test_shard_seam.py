"""The shard seam without a GPU: the cut plans (shardcuts.plans), the protocol's sequential restatement (kxp.CpuShard) on every plan,
k_sync's restatement (shardcuts.sync_points) against the true run — and the populations that test_shard_seam_gpu.py draws on, counted
and asserted here so that a later edit of a generator or of the plans cannot hollow the device tests out.

What the device tests run is decided HERE (cases): per program the 4 097-byte and the 8 209-byte accepted samples and, for each, the
variants with one byte overwritten at 64, 4 095, 4 096 and the last byte; every plan of a sample's length runs once, on one input of
that sample's group, the inputs taking turns along the plans (shifted by the seed, so that over the programs every plan meets every
kind of input)."""
import functools

import kxp
import pytest
import randprog
import shardcuts as sc
import test_random_inputs as tr
from conftest import blob_of

from kleenexlang_amd import workloads
from oracle import oracle

SEG = 64
TARGETS = (4097, tr.LONG)
VARIANT_AT = (64, 4095, 4096)           # and the last byte

# hand-built programs for the classes that generated ones reach seldom
PARITY = 'main := even\neven := ~/a/ odd | /b/ even | "E" /\\n/\nodd := ~/a/ even | ~/b/ odd | "O" /\\n/\n'      # no segment ever synchronises
NEVER_MERGING = 'main := /[ab]*/ "!" | /[ab]*/ ~/c/ "?"\n'                    # the start-leaf map stays open to the last byte


def parity_input(n):
    return (b"ab" * n)[:n - 2] + b"a\n"


def never_merging_input(n):
    import random
    rnd = random.Random(5)
    return bytes(rnd.choice(b"ab") for _ in range(n - 1)) + b"c"


def apache_input():
    """-> (apache_log lines with ONE escaped quote, in the request field of a line behind byte 4 096: a context that the delayed form's K
    symbols do not decide; the position of its backslash)"""
    lines = workloads.generate("apache_log", 24000, 31).split(b"\n")[:-1]
    k = next(i for i in range(len(lines)) if sum(len(ln) + 1 for ln in lines[:i]) > 4096)
    lines[k] = lines[k].replace(b' HTTP/', b'\\"   5x HTTP/', 1)
    data = b"\n".join(lines) + b"\n"
    assert data.count(b'\\"') == 1
    return data, data.index(b'\\"')


@functools.lru_cache(maxsize=None)
def stages_of(src):
    return kxp.parse(blob_of(src, 3))


def overwritten(kind, seed, target):
    """the variants of the sample that differ from it in ONE byte, at 64, 4 095, 4 096 or the last: [(position, data)]"""
    d = tr.sample(kind, seed, target)
    want = {p for p in VARIANT_AT + (len(d) - 1,) if p < len(d)}
    out = []
    for v in tr.variants(kind, seed, target):
        if len(v) == len(d) and v != d:      # (an overwrite with the byte that stood there is the sample again)
            p = next(i for i in range(len(d)) if v[i] != d[i])
            if p in want and p not in [x for x, _ in out]:
                out.append((p, v))
    return out


@functools.lru_cache(maxsize=None)
def cases(kind, seed, thin=False):
    """what the device tests run on this program: [(data, plan)] — every plan of each sample's length once, the sample and its
    overwritten variants taking turns"""
    out = []
    for target in TARGETS:
        d = tr.sample(kind, seed, target)
        if len(d) < 2:
            continue
        group = [d] + [v for _, v in overwritten(kind, seed, target)]
        for j, plan in enumerate(sc.plans(len(d), thin)):
            out.append((group[(j + seed) % len(group)], plan))
    return tuple((d, tuple(p)) for d, p in out)


@functools.lru_cache(maxsize=256)
def truths_of(src, data):
    return sc.truths(stages_of(src), data)


@functools.lru_cache(maxsize=None)
def stage0_fail(src, data):
    """where stage 0 rejects `data` (None: it does not) — the oracle's position where the program has one stage"""
    stages = stages_of(src)
    if len(stages) == 1:
        try:
            oracle.run(blob_of(src, 3), data)
            return None
        except oracle.OracleMatchError as e:
            return e.pos
    return sc.Truth(stages[0], data).fail


def head_classes(stage, data, plan, fail):
    """the head classes of one plan at 64-byte segments, from sync_points: per class the number of shards (or 1 / 0 for the two
    rejection classes).  A shard behind the failure is not counted: the engine's figures there are of no consequence."""
    c = dict.fromkeys(("head", "head_crosses_piece", "head_whole_shard", "reject_in_head", "reject_in_last_byte"), 0)
    off = sc.offsets(list(plan))
    for i, part in enumerate(sc.split(data, list(plan))):
        a, b = off[i], off[i + 1]
        if fail is not None and a > fail:
            break
        if fail is not None and len(part) and fail == b - 1:
            c["reject_in_last_byte"] = 1
        if i == 0 or not part:
            continue
        head, synced, _ = sc.predict_forward(stage, part, SEG, False)
        c["head"] += head > 0
        c["head_crosses_piece"] += head >= 64
        c["head_whole_shard"] += head == len(part) and not synced
        if fail is not None and a <= fail < a + head:
            c["reject_in_head"] = 1
    return c


# ----------------------------------------------------------------------------------------------------------------- plans
def test_plans():
    """Every plan sums to n.  At 8 209 bytes all the plans are there: 25 two-part cuts and 7 multi-part plans; at 4 097 the cut
    4 097 = n and the plan [4096, 1, 2, n - 4099] fall away, and n - 2, n - 1 are 4 095, 4 096 once more: 22 and 6.  Short inputs keep
    what makes sense; the thinned list keeps 1, 2, 63, 64, 65, 4 095, 4 096, 4 097 and n - 1."""
    for n in (0, 1, 2, 3, 63, 64, 65, 127, 128, 200, 2000, 4096, 4097, 4099, 4100, 8209, 20500):
        for p in sc.plans(n) + sc.plans(n, thin=True):
            assert sum(p) == n and all(x >= 0 for x in p), (n, p)
    p = sc.plans(8209)
    assert len(p) == 25 + 7 and [4096, 1, 2, 4110] in p and [64, 0, 63, 0, 8082] in p and [1, 8207, 1] in p and [0, 8209] in p and [8209, 0] in p
    assert [100] * 20 + [6209] in p and [1641, 1642, 1642, 1642, 1642] in p
    assert sorted(x[0] for x in p if len(x) == 2 and x[0] and x[1]) == sorted(sc.TWO_PART_CUTS + (8144, 8145, 8207, 8208))
    assert len(sc.plans(4097)) == 22 + 6 and [4096, 1] in sc.plans(4097) and [4096, 1, 2, -2] not in sc.plans(4097)
    assert [4096, 1, 2, 0] in sc.plans(4099)
    assert sc.plans(1)[:2] == [[0, 1], [1, 0]] and sc.plans(2)[:2] == [[1, 1], [1, 0, 1]] and sc.plans(0) == [[0, 0], [0]]
    assert [x[0] for x in sc.plans(8209, thin=True) if len(x) == 2 and x[0] and x[1]] == [1, 2, 63, 64, 65, 4095, 4096, 4097, 8208]


# --------------------------------------------------------------------------------------- CpuShard and Truth on every plan
CPU_SEEDS = range(0, tr.NPROG, 8)       # CpuShard walks every leaf of every shard in pure Python: every eighth program, 15 of 120 per kind


@pytest.mark.parametrize("kind", ["plain", "wide"])
def test_cpushard_on_every_plan(kind):
    """Every eighth program of seeds 0-119 (15 per kind: the restriction), every stage, on the 4 097-byte sample and
    on one of its rejected variants, under every plan: the concatenated bytes, or the global failure position on every rank, are the
    oracle's.  And what shardcuts.Truth gives a shard (the slice of the per-step bytes) is what CpuShard.emit() gives it: the device
    tests compare with Truth, which walks the input once and not once per plan."""
    nprog = nrej = nplans = 0
    for seed in CPU_SEEDS:
        src = tr.source(kind, seed)
        if src is None:
            continue
        stages = stages_of(src)
        d = tr.sample(kind, seed, 4097)
        rejected = [v for _, v in overwritten(kind, seed, 4097) if isinstance(tr.expect(kind, seed, v), tuple)]
        datas = [d] + ([rejected[seed % len(rejected)]] if rejected else [])
        nprog += 1
        nrej += len(datas) > 1
        for data in datas:
            want = tr.expect(kind, seed, data)
            ts = sc.truths(stages, data)
            for plan in sc.plans(len(data)):
                got = sc.run_cpu(stages, sc.split(data, plan))
                where = (kind, seed, src, len(data), plan)
                nplans += 1
                if isinstance(want, bytes):
                    assert got["result"] == want, where
                    for recs, t in zip(got["shards"], ts):
                        off = sc.offsets([r["n"] for r in recs])
                        assert off[-1] == t.n, where
                        for r, a, b in zip(recs, off, off[1:]):
                            assert r["bytes"] == t.own_bytes(a, b, r["index"] == 0), where + (r["stage"], r["index"])
                            assert r["fixed"]["end_state"] == t.states[b], where + (r["stage"], r["index"])
                else:
                    assert got["result"][:2] == want, where + (got["result"],)
                    assert ts[-1].fail == want[1] and got["result"][2] == len(ts) - 1, where
    print(kind, 'programs', nprog, 'with a rejected variant', nrej, 'plans run', nplans)
    assert nprog >= len(CPU_SEEDS) - 1 and nrej >= 5 and nplans >= 28 * 15, (nprog, nrej, nplans)


# ------------------------------------------------------------------------------------------------------- sync_points
CPU_HALF = range(0, tr.NPROG, 2)        # sync_points and the populations: every second program, 60 of 120 per kind (pure Python loops)


def check_sync_points(stage, data, seg, where):
    """wherever a segment synchronises and the true run is alive there, the true run is in the reported state; positions lie inside
    the segment, behind at least one byte unless the start subset is decided.  -> synchronised segments checked"""
    t = sc.Truth(stage, data)
    n = 0
    for first in (True, False):
        for k, p in enumerate(sc.sync_points(stage, data, seg, first)):
            if p is None or (first and k == 0):
                continue
            pos, st = p
            assert k * seg <= pos <= min((k + 1) * seg, len(data)), where + (k, p)
            assert pos > k * seg or stage.sync_state[0] != sc.MULTI, where + (k, p)
            if t.states[pos] is not None:
                assert t.states[pos] == st, where + (k, p, t.states[pos])
                n += 1
    return n


@pytest.mark.parametrize("kind", ["plain", "wide"])
def test_sync_points_report_the_state_of_the_true_run(kind):
    """On the 4 097-byte sample of every second program (60 per kind), in segments of 64 and of 4 096 bytes, every stage; the parity program synchronises
    nowhere but behind the newline that ends its input, the shipped apache_log one in every segment."""
    checked = 0
    for seed in [s for s in CPU_HALF if tr.source(kind, s) is not None]:
        data = tr.sample(kind, seed, 4097)
        for si, t in enumerate(sc.truths(stages_of(tr.source(kind, seed)), data)):
            for seg in (64, 4096):
                checked += check_sync_points(t.stage, t.data, seg, (kind, seed, si, seg))
    assert checked > 1000, checked
    st = stages_of(PARITY)[0]
    # (the newline that ends the input decides the state: the last segment — that one byte — synchronises at n, behind a head of n)
    assert sc.sync_points(st, parity_input(4097), 64, False) == [None] * 64 + [(4097, sc.Truth(st, parity_input(4097)).states[4097])]
    assert sc.predict_forward(st, parity_input(4097), 64, False) == (4097, 1, 64)
    assert sc.predict_forward(st, parity_input(4097)[:-1], 64, False) == (4096, 0, 64)
    assert sc.predict_forward(st, parity_input(4097), 64, True) == (0, 1, 63)
    log = workloads.generate("apache_log", 6000, 31)
    st = stages_of("apache_log")[0]
    assert check_sync_points(st, log, 64, ("apache_log",)) > 50


# ------------------------------------------------------------------------------------------------------- populations
def hand_built_cases():
    """[(name, source, data, plan)]: the parity program (every shard behind the first is one head, and a rejection inside it), the
    never-merging program (its start-leaf maps are not constant; with a shard beyond 65 536 bytes), apache_log with an escaped quote across
    the cut and far behind it"""
    out = []
    d = parity_input(4097)
    for plan in sc.plans(len(d)):
        out.append(("parity", PARITY, d, tuple(plan)))
    bad = d[:4000] + b"c" + d[4001:]
    for plan in ([64, 4033], [100] * 20 + [2097], [3999, 98], [4000, 97], [4001, 96]):
        out.append(("parity", PARITY, bad, tuple(plan)))
    d = never_merging_input(8209)
    for plan in sc.plans(len(d)):
        out.append(("never_merging", NEVER_MERGING, d, tuple(plan)))
    d, bs = apache_input()
    for c in (bs - 64, bs - 3, bs - 1, bs, bs + 1, bs + 2):       # (bs + 1: between the backslash and the quote)
        out.append(("apache_log", "apache_log", d, (c, len(d) - c)))
    # the context 1 500 bytes inside a later window of 20 KiB: in segments of 256 bytes (where the lanes of a later shard have parts
    # of their own) one escaping lane among 80 is less than a sixteenth, which arms the stage's slow path in that window
    for plan in ((bs - 1500, len(d) - bs + 1500), (1000, bs - 2500, len(d) - bs + 1500)):
        assert plan[-1] >= 80 * 256, plan
        out.append(("apache_log", "apache_log", d, plan))
    # a later shard of more than 65 536 bytes whose start-leaf map stays open all the way: k_dmap gives up at its cap
    d = never_merging_input(70001)
    for plan in ((100, 66000, 3901), (3000, 67001)):
        out.append(("never_merging", NEVER_MERGING, d, plan))
    return out


def population():
    tot = dict.fromkeys(("programs", "left_out", "plans", "head", "head_crosses_piece", "head_whole_shard", "reject_in_head",
                         "reject_in_last_byte"), 0)
    per_kind = {}
    for kind in ("plain", "wide"):
        k = dict(tot)
        for seed in range(tr.NPROG):
            src = tr.source(kind, seed)
            if src is None:
                k["left_out"] += 1
                continue
            if seed not in CPU_HALF:
                continue
            k["programs"] += 1
            stage = stages_of(src)[0]
            for data, plan in cases(kind, seed):
                c = head_classes(stage, data, plan, stage0_fail(src, data))
                k["plans"] += 1
                for name, v in c.items():
                    k[name] += v
        per_kind[kind] = k
    h = dict(tot)
    for name, src, data, plan in hand_built_cases():
        stage = stages_of(src)[0]
        c = head_classes(stage, data, plan, stage0_fail(src, data))
        h["plans"] += 1
        for cname, v in c.items():
            h[cname] += v
    h["programs"] = 3
    per_kind["hand_built"] = h
    return per_kind


# what population() gives (stage 0, 64-byte segments, every second program); the floors are four fifths of it, rounded down
MEASURED = {"plain": {"programs": 60, "left_out": 1, "plans": 2666, "head": 4320, "head_crosses_piece": 761, "head_whole_shard": 1027,
                      "reject_in_head": 183, "reject_in_last_byte": 294},
            "wide": {"programs": 60, "left_out": 0, "plans": 2832, "head": 4544, "head_crosses_piece": 93, "head_whole_shard": 181,
                     "reject_in_head": 87, "reject_in_last_byte": 326},
            "hand_built": {"programs": 3, "left_out": 0, "plans": 75, "head": 143, "head_crosses_piece": 75, "head_whole_shard": 43,
                           "reject_in_head": 4, "reject_in_last_byte": 1}}
FLOORS = {kind: {k: v * 4 // 5 for k, v in m.items() if k not in ("left_out",)} for kind, m in MEASURED.items()}


def test_populations():
    """What the device tests draw on (stage 0 of every SECOND usable program under cases() — 60 per kind, half of what the device runs —
    and the hand-built programs), in 64-byte segments:
    shards with a head, with a head that crosses a piece (head_len >= 64), that are one head (no segment synchronises: the state is
    chained through); plans whose rejection falls inside a head, and in a shard's last byte.  Generated programs synchronise within a
    few bytes nearly everywhere, so the long heads come from the parity program."""
    got = population()
    print(got)
    assert got["plain"]["left_out"] <= tr.NPROG - tr.MEASURED["plain"]["usable"] and got["wide"]["left_out"] <= tr.NPROG - tr.MEASURED["wide"]["usable"]
    for kind, floors in FLOORS.items():
        for k, floor in floors.items():
            assert got[kind][k] >= floor, (kind, k, got[kind], floor)
    for k in ("head", "head_crosses_piece", "head_whole_shard", "reject_in_head", "reject_in_last_byte"):
        assert sum(got[kind][k] for kind in got) >= 1, k
