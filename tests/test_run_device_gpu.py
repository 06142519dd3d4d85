"""kx_run_device into a caller's buffers, with guards: what the call does to memory it does not own.

The routes, their inputs and everything those have to be are test_run_device.py's (checked without a GPU).  Here every route keeps ONE
Program for all of its inputs, in two shuffled orders with rejected inputs between accepted ones: each test is also a test of the
grow-only work space, the stage and action buffers, the delayed form's back-off and the job-stride heuristic under reuse.

The output lies in a device arena as

    4 KiB guard | body of exactly out_len bytes | 4 KiB guard

with the body on a 256-byte boundary (or a few bytes behind one, for the refusal of unaligned addresses).  The guards hold a pattern that
depends on the position (a stray store of a constant onto the same constant would be invisible); the body is pre-filled with the bytewise
complement of the oracle's result, so that a byte the engine does not write cannot be right by accident.  4 KiB is more than the 1 KiB
a wave stores per step of its flush.  After the call the whole arena region is compared with what it has to be: a run that succeeds
changes the body into the oracle's bytes and nothing else; every other outcome (a rejected input, KX_E_CAPACITY, KX_E_ARG) changes nothing.
The input lies in an arena of its own with 4 KiB of junk in front and behind, `lead` bytes past a 256-byte boundary, and has to be
bit-identical afterwards, junk included."""
import ctypes

import numpy as np
import pytest
import test_run_device as rd
from conftest import blob_of

from kleenexlang_amd import Program, host, sharded, workloads
from oracle import oracle

pytestmark = pytest.mark.gpu

GUARD = 4096
DEV = "cuda:0"
KX_E_CAPACITY, KX_E_ARG = -3, -4


def _pattern(n):
    i = np.arange(n, dtype=np.uint64)
    return ((i * np.uint64(167) + (i >> np.uint64(8)) * np.uint64(29) + np.uint64(0x5A)) ^ (i >> np.uint64(3))).astype(np.uint8)


_PATTERN = _pattern((4 << 20) + 3 * GUARD + 16384)


def pattern(n, salt=0):
    """n bytes that depend on their position (no run of equal bytes, no period of 256); a copy"""
    return _PATTERN[salt:salt + n].copy()


class Arena:
    """a device allocation on a 256-byte boundary, written and read back as a whole region"""

    def __init__(self, nbytes):
        import torch
        self.t = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        assert self.t.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr()

    def put(self, arr):
        import torch
        assert len(arr) <= self.t.numel()
        self.t[:len(arr)].copy_(torch.from_numpy(arr))
        torch.cuda.synchronize()

    def get(self, n):
        import torch
        torch.cuda.synchronize()
        return self.t[:n].cpu().numpy()


_STATE = {}


def arenas():
    if "out" not in _STATE:
        _STATE["out"] = Arena(2 * GUARD + (4 << 20) + 256)
        _STATE["in"] = Arena(2 * GUARD + (64 << 10) + 256)
    return _STATE["out"], _STATE["in"]


def program(name):
    """the route's one Program (kept for the whole module: every test reuses what the tests before it left)"""
    progs = _STATE.setdefault("programs", {})
    if name not in progs:
        r = rd.ROUTE[name]
        progs[name] = Program(rd.blob(r.prog), segment_bytes=r.seg, config=rd.config(r))
    return progs[name]


@pytest.fixture(scope="module", autouse=True)
def _close_programs():
    yield
    for p in _STATE.pop("programs", {}).values():
        p.close()
    _STATE.clear()


def raw(p, d_in, n, d_out, cap, stream=0):
    """kx_run_device itself: (return code, *out_len, stats)"""
    ol = ctypes.c_size_t(0xDEADBEEF)
    st = host.KxStats()
    rc = p._lib.kx_run_device(p._h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap, ctypes.byref(ol), ctypes.byref(st),
                              ctypes.c_void_p(stream))
    return rc, ol.value, st


def place_input(data, lead=0, front=None, back=None):
    """the input in its arena: (device address, the region as written).  front / back: 4 KiB of junk each (default: the pattern)"""
    _, ain = arenas()
    n = len(data)
    region = np.empty(GUARD + lead + n + GUARD, dtype=np.uint8)
    region[:GUARD + lead] = pattern(GUARD + lead, 11) if front is None else np.frombuffer((front * ((GUARD + 16) // len(front) + 2))[-(GUARD + lead):], dtype=np.uint8)
    region[GUARD + lead:GUARD + lead + n] = np.frombuffer(data, dtype=np.uint8)
    region[GUARD + lead + n:] = pattern(GUARD, 12345) if back is None else np.frombuffer((back * (GUARD // len(back) + 2))[:GUARD], dtype=np.uint8)
    ain.put(region)
    return ain.ptr + GUARD + lead, region


def lay_output(body_len, want=None, shift=0):
    """the output region before the call: guard | `shift` more guard bytes | body | guard.  The body is the complement of `want` (the
    pattern where there is no result to complement).  Returns (device address of the body, the region as written)."""
    aout, _ = arenas()
    front = GUARD + shift
    region = pattern(front + body_len + GUARD, 777)
    if want is not None:
        assert len(want) == body_len
        region[front:front + body_len] = 255 - np.frombuffer(want, dtype=np.uint8)
    aout.put(region)
    return aout.ptr + front, region


def check_region(before, want, shift, where):
    """the output region after the call: `before` with the body replaced by `want` (None: untouched)"""
    aout, _ = arenas()
    exp = before
    if want is not None:
        exp = before.copy()
        front = GUARD + shift
        exp[front:front + len(want)] = np.frombuffer(want, dtype=np.uint8)
    got = aout.get(len(before))
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        front = GUARD + shift
        n = len(before) - front - GUARD
        what = ["front guard" if b < front else "body" if b < front + n else "rear guard / slack" for b in (bad[0], bad[-1])]
        raise AssertionError("%s: %d bytes differ, first at body offset %d (%s), last at %d (%s) of a body of %d bytes; got %s expected %s"
                             % (where, len(bad), bad[0] - front, what[0], bad[-1] - front, what[1], n, got[bad[:8]].tolist(), exp[bad[:8]].tolist()))


def check_input(region, where):
    _, ain = arenas()
    assert np.array_equal(ain.get(len(region)), region), "%s: the engine wrote to its input or to the bytes around it" % (where,)


def run_accepted(p, inp, where, cap_extra=0, query=False, short=False, **placing):
    """one accepted input into a body of exactly the result's length (+ cap_extra of slack, which is the rear guard)"""
    d_in, in_region = place_input(inp.data, **placing)
    n, L = len(inp.data), len(inp.want)
    if query:
        rc, ol, _ = raw(p, d_in, n, 0, 0)
        assert (rc, ol) == ((KX_E_CAPACITY if L else 0), L), (where, "size query", rc, ol, L)
    if short and L:
        body, before = lay_output(L, inp.want)
        rc, ol, _ = raw(p, d_in, n, body, L - 1)
        assert (rc, ol) == (KX_E_CAPACITY, L), (where, "one byte short", rc, ol, L)
        check_region(before, None, 0, where + ("one byte short",))
    if L == 0:
        rc, ol, _ = raw(p, d_in, n, 0, 0)
        assert (rc, ol) == (0, 0), (where, "empty result into no buffer", rc, ol)
    body, before = lay_output(L, inp.want)
    rc, ol, st = raw(p, d_in, n, body, L + cap_extra)
    assert (rc, ol) == (0, L), (where, rc, ol, L, p._err() if rc < 0 else "")
    assert st.out_bytes == L and st.in_bytes == n
    check_region(before, inp.want, 0, where)
    check_input(in_region, where)


def run_rejected(p, inp, where, **placing):
    """a rejected input with room for any result: rc 1, the oracle's position and stage, nothing written"""
    d_in, in_region = place_input(inp.data, **placing)
    cap = 2 * len(inp.data) + GUARD
    body, before = lay_output(cap)
    rc, ol, st = raw(p, d_in, len(inp.data), body, cap)
    assert rc == 1, (where, rc, ol)
    assert (st.fail_pos, st.fail_stage) == inp.want[1:], (where, st.fail_pos, st.fail_stage, inp.want)
    check_region(before, None, 0, where)
    check_input(in_region, where)


def sweep(name, seed, **kw):
    p = program(name)
    for k, inp in enumerate(rd.order(rd.ROUTE[name].table, seed)):
        where = (name, seed, k, inp.group, len(inp.data))
        if inp.group == "reject":
            run_rejected(p, inp, where)
        else:
            run_accepted(p, inp, where, **kw)


# --------------------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", rd.NAMES)
def test_exact_capacity(name):
    """the size query, one byte too few, exactly enough, and an empty result into no buffer at all"""
    sweep(name, 1, query=True, short=True)
    sweep(name, 2)


@pytest.mark.parametrize("name", rd.NAMES)
def test_slack_is_not_scratch(name):
    """cap = out_len + 4 KiB: no byte outside [d_out, d_out + *out_len) changes, whatever the capacity says"""
    sweep(name, 3, cap_extra=GUARD)
    sweep(name, 4, cap_extra=GUARD)


@pytest.mark.parametrize("name", rd.NAMES)
def test_rejected_input_writes_nothing(name):
    """`prints no output at all` holds for the device entry: every rejected variant twice, with accepted runs between them"""
    p = program(name)
    table = rd.ROUTE[name].table
    acc = [i for i in rd.inputs(table) if i.group == "40k"]
    for rnd in (0, 1):
        for k, inp in enumerate(i for i in rd.inputs(table) if i.group == "reject"):
            run_rejected(p, inp, (name, rnd, k, len(inp.data)))
            if k % 3 == 2:
                run_accepted(p, acc[(k // 3 + rnd) % len(acc)], (name, rnd, k, "accepted between"))


def junk_of(table):
    """three fillings for the bytes around the input: (front, back) that continue the language, bytes the program rejects, zeros"""
    valid = next(i.data for i in rd.inputs(table) if i.group == "40k")
    bad = rd.rejected_byte(table)
    fill = {"valid": (valid, valid), "rejected": (bad, bad), "zeros": (b"\0", b"\0")}
    assert len({f[0][:1] for f in fill.values()}) == 3 and bad != b"\0"
    return fill


@pytest.mark.parametrize("name", rd.NAMES)
def test_input_placement(name):
    """d_in in place (16-byte aligned) and 1, 7, 15 bytes past a boundary (the engine's aligned copy), among bytes that continue the
    language, bytes the program rejects and zeros: the result is the oracle's on the n bytes alone, the input arena is untouched"""
    p = program(name)
    table = rd.ROUTE[name].table
    ins = [i for i in rd.inputs(table) if i.group in ("small", "40k") or i.group == "reject" and (len(i.data) < rd.PIECE or len(i.data) > 36 * 1024)]
    ins = [i for i in ins if i.group != "small" or len(i.want) not in range(4, 16) or len(i.data) % 4 == 3]     # (thin the tiny ones)
    for lead in (0, 1, 7, 15):
        for kind, (front, back) in junk_of(table).items():
            for k, inp in enumerate(ins):
                where = (name, lead, kind, k, inp.group, len(inp.data))
                (run_rejected if inp.group == "reject" else run_accepted)(p, inp, where, lead=lead, front=front, back=back)


UNALIGNED = [n for n in rd.NAMES if n != "actions"]


@pytest.mark.parametrize("name", UNALIGNED)
def test_unaligned_output_is_refused_before_anything_runs(name, monkeypatch, capfd):
    """a d_out that is not 16-byte aligned, where the last stage has no register actions: KX_E_ARG, nothing written, and nothing launched
    (under KX_DEBUG the pipeline prints a line per stage it begins: the aligned call prints it, the refused ones print nothing)"""
    monkeypatch.setenv("KX_DEBUG", "1")
    p = program(name)
    inp = next(i for i in rd.inputs(rd.ROUTE[name].table) if i.group == "4k")
    d_in, in_region = place_input(inp.data)
    L = len(inp.want)
    form = p.stage_delayed_form(0)
    capfd.readouterr()
    for shift in (1, 8, 15):
        body, before = lay_output(L, inp.want, shift=shift)
        assert body % 16 == shift
        rc, ol, _ = raw(p, d_in, len(inp.data), body, L)
        assert rc == KX_E_ARG, (name, shift, rc)
        assert "16-byte aligned" in p._err() and "output" in p._err()
        check_region(before, None, shift, (name, "shift", shift))
    err = capfd.readouterr().err
    assert "[kx]" not in err, err[-600:]
    assert p.stage_delayed_form(0) == form
    run_accepted(p, inp, (name, "aligned"))
    assert "[kx] stage 0 host wall" in capfd.readouterr().err
    check_input(in_region, (name,))


@pytest.mark.parametrize("name", ["df_k2", "actions"])
def test_work_goes_to_the_callers_stream(name):
    """Everything on a stream of the test's own.  The input tensor holds bytes the program rejects; then, without the host waiting:
    filler passes over a large tensor, the copy of the real input, and the engine at once.  An engine that put work on another stream
    reads the rejected bytes.  The copy must still be pending when the engine is called (an event behind it has not completed), else
    the run proves nothing: the filler is doubled until it is, eight times at the most."""
    import torch
    p = program(name)
    table = rd.ROUTE[name].table
    inp = [i for i in rd.inputs(table) if i.group == "40k"][-1]
    n, L = len(inp.data), len(inp.want)
    assert isinstance(rd.expect(rd.ROUTE[name].prog, rd.rejected_byte(table) * n), tuple)
    aout, ain = arenas()
    src = torch.frombuffer(bytearray(inp.data), dtype=torch.uint8).to(DEV)
    scratch = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    s = torch.cuda.Stream(device=DEV)
    assert s.cuda_stream != torch.cuda.current_stream(DEV).cuda_stream
    passes, pending = 2, False
    for _ in range(9):
        d_in, _ = place_input(rd.rejected_byte(table) * n)
        body, before = lay_output(L, inp.want)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(passes):
                scratch.add_(1)
            ain.t[GUARD:GUARD + n].copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(s)
        pending = not ev.query()
        rc, ol, _ = raw(p, d_in, n, body, L, s.cuda_stream)
        torch.cuda.synchronize()
        if pending:
            break
        passes *= 2
    assert pending, "the copy of the input had completed before the engine was called, with %d filler passes: the test proves nothing" % passes
    assert (rc, ol) == (0, L), (name, rc, ol, "the engine did not wait for the work queued on its stream")
    check_region(before, inp.want, 0, (name, "stream"))


def test_hole_routes_take_the_paths_they_name(monkeypatch, capfd):
    """an escaped quote arms the slow path of the forward pass (hole lanes replay into `out`); with the slow path off the shard falls
    back to the general engine, every time"""
    monkeypatch.setenv("KX_DEBUG", "1")
    big = [i for i in rd.inputs("holes") if i.group == "40k"]
    for name in ("holes_slow", "holes_fall_back"):
        p = program(name)
        p.reset_delayed_form(0)
        for inp in big:
            capfd.readouterr()
            run_accepted(p, inp, (name, len(inp.data)))
            err = capfd.readouterr().err
            if name == "holes_slow":
                assert "the slow path resolved" in err and "falls back" not in err, err[-800:]
                assert p.stage_delayed_form(0) == 1
            else:
                assert "falls back to the general engine" in err and "the slow path resolved" not in err, err[-800:]


def test_the_never_delayed_route_leaves_the_form():
    p = program("gen_never_delayed")
    p.reset_delayed_form(0)
    inp = [i for i in rd.inputs("numbers") if i.group == "40k"][0]
    run_accepted(p, inp, ("gen_never_delayed",))
    assert p.stage_delayed_form(0) in (2, 3)


# --------------------------------------------------------------------------------------------------------------------- shards
@pytest.fixture(scope="module")
def shard_data():
    out = {}
    for prog, shape in (("apache_log", "apache_log"), ("csv2json", "csv"), ("iso_datetime_to_json", "datetime")):
        data = workloads.generate(shape, 300000, 41)
        out[prog] = (data, oracle.run(blob_of(prog), data))
    return out


@pytest.mark.parametrize("engine", ["delayed", "general"])
@pytest.mark.parametrize("prog", ["apache_log", "csv2json", "iso_datetime_to_json"])
def test_shards_into_guarded_buffers(prog, engine, shard_data):
    """kx_shard_emit under the same observation: every shard gets exactly the length kx_shard_resolve named, between guards (k_head /
    k_dhead, the init copy on the first shard only, k_fixtail).  2 and 5 shards cut at multiples of 16, an empty last and an empty
    middle shard."""
    import torch
    data, want = shard_data[prog]
    blob = blob_of(prog)
    cut = (len(data) // 2) // 16 * 16
    plans = [[data[(len(data) * i // w) // 16 * 16:(len(data) * (i + 1) // w) // 16 * 16 if i + 1 < w else len(data)] for i in range(w)] for w in (2, 5)]
    plans += [[data, b""], [data[:cut], b"", data[cut:]], [data[:cut], data[cut:], b""]]
    for parts in plans:
        assert b"".join(parts) == data
        world = len(parts)
        tens = [torch.frombuffer(bytearray(part if part else b"\0" * 16), dtype=torch.uint8).to(DEV) for part in parts]
        progs = [Program(blob, segment_bytes=1024, config=host.config_from_env({}, **(rd.GENERAL if engine == "general" else {}))) for _ in range(world)]
        shards = []
        try:
            for i in range(world):
                shards.append(progs[i].shard_begin(0, tens[i].data_ptr(), len(parts[i]), i == 0, i == world - 1))
            res = sharded.run_stage_local(shards, [len(part) for part in parts])
            assert all(r[0] == "ok" for r in res), res
            lens = [int(r[1]) for r in res]
            assert sum(lens) == len(want), (prog, engine, lens)
            at = 0
            for i, s in enumerate(shards):
                piece = want[at:at + lens[i]]
                body, before = lay_output(lens[i], piece)
                s.emit(body, lens[i])
                check_region(before, piece, 0, (prog, engine, [len(part) for part in parts], "shard", i))
                at += lens[i]
        finally:
            for s in shards:        # (a shard hands its work space back to its program when it ends: never after the program is gone)
                s.end()
            for p in progs:
                p.close()
