"""GPU: record mode with a multi-byte separator.  kx_split_records_rs through the C ABI against the offsets model
(split_rs_records_model): every separator length, every start alignment, tiny buffers, contexts, a separator straddling every
border of the tile shape, self-overlapping runs inside granules and through whole tiles, capacity, and windows chained on the
device; Program.run_records(rs=…) and `BIN --records --rs=…` with every record checked against the CPU oracle on that record alone."""
import ctypes
import os
import random
import subprocess

import pytest

from kleenexlang_amd import build, host
from kleenexlang_amd.host import MatchError, Program
from oracle import oracle

pytestmark = pytest.mark.gpu

KEXC = os.path.join(build.OUT, "kexc")
PARAGRAPHS = os.path.join(build.ROOT, "kleenexlang_amd", "examples", "paragraphs.kex")
T = 65536
# CRLF-terminated records whose fields may hold a bare \n (written as \n in the output); a bare \r is an error
CRLF = r'''
start: recs
recs := rec*
rec := (~/\n/ "\\n" | /[^\r\n]/)* ~/\r\n/ "\n"
'''
model = host.split_rs_records_model


def _split(view, rs, ctx=b"", base=0, cap=None):
    """kx_split_records_rs on a device view: (rc, n_records, offsets list, ctx_out, tail_len)."""
    import torch
    lib = host.load_engine()
    n, col, tl = ctypes.c_uint64(), ctypes.c_uint32(99), ctypes.c_uint64(99)
    cout = (ctypes.c_uint8 * 8)()
    cap = view.numel() + 2 if cap is None else cap
    off = torch.full((max(cap, 1),), -1, dtype=torch.int64, device="cuda")
    rc = lib.kx_split_records_rs(ctypes.c_void_p(view.data_ptr() if view.numel() else None), view.numel(), rs, len(rs), ctx, len(ctx), base,
                                 ctypes.c_void_p(off.data_ptr() if cap else None), cap, ctypes.byref(n), cout, ctypes.byref(col), ctypes.byref(tl),
                                 None)
    torch.cuda.synchronize()
    return rc, n.value, off.tolist(), bytes(cout[:min(col.value, 8)]), tl.value


def _dev(data, lead=0, guard=b"\r\n"):
    """data on the device at `lead` bytes past a 256-byte aligned allocation, with separator bytes as guards around it."""
    import torch
    buf = torch.tensor(list(guard) * ((lead + len(data) + 64) // len(guard) + 1), dtype=torch.uint8)
    if data:
        buf[lead:lead + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return buf.cuda()[lead:lead + len(data)]


def _check(data, rs, ctx=b"", lead=0, base=0):
    want = model(data, rs, ctx)
    rc, n, off, cout, tl = _split(_dev(data, lead, guard=rs), rs, ctx, base)
    assert rc == 0 and n == len(want[0]) - 1, (data[:40], rs, ctx, lead, n, len(want[0]) - 1)
    assert off[:n + 1] == [base + x for x in want[0]], (data[:40], rs, ctx, lead)
    assert off[n + 1] == -1                                        # nothing written past the last offset
    assert (cout, tl) == want[1:], (data[:40], rs, ctx, lead, cout, tl, want[1:])


def _soup(r, rs, n, other=b"x"):
    alphabet = bytes(set(rs)) + other
    return bytes(r.choice(alphabet) for _ in range(n))


# ---------------------------------------------------------------------------------------------------------- kx_split_records_rs
@pytest.mark.parametrize("rs", [b"\n", b"\r\n", b"aba", b"abab", b"|~|x~", b"ab\0abc", b"\xff\xfe\xff\xfe\xff\xfe\xff", b"aaaaaaaa", b"\r\n\r\n",
                                b"abcdefgh"])
def test_every_separator_length_on_random_data(rs):
    import torch
    r = random.Random(len(rs))
    data = _soup(r, rs, 3 * T + 1234, other=b"" if len(set(rs)) > 1 else b"x")
    _check(data, rs, lead=5)
    _check(data[:T + 100], rs, lead=0, base=1000003)
    if len(rs) == 1:
        v = _dev(data, 5)
        assert host.split_records_tensor(v, rs).tolist() == host.split_rs_records_tensor(v, rs)[0].tolist() == model(data, rs)[0]


def test_every_start_alignment_and_tiny_buffers():
    r = random.Random(2)
    for rs in (b"\r\n", b"\n\n", b"abab", b"aaaaaaaa"):
        data = _soup(r, rs, 700)
        for lead in range(16):
            _check(data, rs, lead=lead)
        m = len(rs)
        for lead in (0, 9, 15):
            for d in (b"", rs[:1], rs[:m - 1], rs, rs[1:], rs + rs[:1], b"x"):
                _check(d, rs, lead=lead)
                for k in range(1, m):                              # a context that completes a separator with the first m - k bytes
                    _check(rs[k:] + d, rs, ctx=rs[:k], lead=lead)
                    _check(d, rs, ctx=rs[:k], lead=lead)
                    _check(rs[k:], rs, ctx=rs[:k], lead=lead)


@pytest.mark.parametrize("rs", [b"\r\n", b"|~|", b"\n\n", b"abab", b"abcdefgh", b"aaaaaaaa"])
def test_one_separator_straddling_every_border(rs):
    """Granule (16 B), wave step (1 KiB), (step, wave) group (4 KiB steps and 1 KiB waves inside a tile) and tile (64 KiB)
    borders, at every split of the separator's bytes, with a second copy well behind it."""
    m = len(rs)
    for border in (16, 48, 1024, 3 * 1024, 4096, 5 * 4096, T, 2 * T):
        for s in range(0, m + 1):                                  # s bytes of the separator before the border
            data = bytearray(b"x" * (border + 300))
            data[border - s:border - s + m] = rs
            data[border + 100:border + 100 + m] = rs
            for lead in (0, 11):
                _check(bytes(data[lead:]), rs, lead=lead)          # (lead + offset = the position inside the aligned allocation)


@pytest.mark.parametrize("rs", [b"\n\n", b"aba", b"abab", b"aaaaaaaa"])
def test_self_overlapping_runs_at_every_granule_phase(rs):
    period = {b"\n\n": b"\n", b"aba": b"ab", b"abab": b"ab", b"aaaaaaaa": b"a"}[rs]
    parts, cur = [], 0
    for length in range(1, 41):
        for phase in range(16):
            pad = (phase - cur) % 16
            run = (period * 41)[:length * len(period)] if rs != b"aba" else (period * 41)[:2 * length + 1]
            parts.append(b"x" * (pad + 16) + run + b"y")
            cur += len(parts[-1])
    data = b"".join(parts)
    for lead in (0, 7):
        _check(data, rs, lead=lead)
    _check(data, rs, ctx=rs[:-1], lead=3)


def test_self_overlap_through_whole_tiles():
    for rs, unit in ((b"\n\n", b"\n"), (b"aba", b"ab"), (b"aaaaaaaa", b"a")):
        run = (unit * (T + 40))[:T + 33]
        _check(b"ab" + run + b"x" + rs + b"y", rs, lead=0)
        _check(run, rs, lead=1)
        run = (unit * (2 * T + 8))[:2 * T + 5]
        _check(b"x" * (T - 7) + run + b"z" + rs + rs + b"q", rs, lead=0)       # starts 7 bytes before a tile border
        _check(b"x" * (T - 7 - 13) + run + b"z" + rs, rs, ctx=rs[:1], lead=13)


def test_capacity_and_size_query():
    data = b"one\r\ntwo\nstill two\r\n\r\nfour"
    v = _dev(data, 5)
    assert _split(v, b"\r\n", cap=0)[:2] == (-3, 4)
    rc, n, off, cout, tl = _split(v, b"\r\n", cap=4)
    assert (rc, n) == (-3, 4) and off[:4] == [-1, -1, -1, -1]        # too small: nothing written
    assert _split(v, b"\r\n", cap=5) == (0, 4, [0, 5, 20, 22, 26], b"r", 4)
    assert _split(_dev(b""), b"\r\n", cap=0)[:2] == (-3, 0)
    assert _split(_dev(b""), b"\r\n", ctx=b"\r", cap=1) == (0, 0, [0], b"\r", 0)
    assert _split(v, b"\n\n", cap=0)[:2] == (-3, 1) and _split(_dev(b"\n" * 9), b"\n\n", cap=0)[:2] == (-3, 5)
    assert _split(v, b"", cap=5)[0] == -4 and _split(v, b"123456789")[0] == -4 and _split(v, b"ab", ctx=b"ab")[0] == -4   # KX_E_ARG


@pytest.mark.parametrize("rs", [b"\r\n", b"\n\n", b"abab"])
def test_windows_chained_on_the_device(rs):
    r = random.Random(len(rs) + 40)
    data = _soup(r, rs, 200 * 1024)
    want = model(data, rs)[0]
    cuts = sorted(r.sample(range(1, len(data)), 17) + [5000, 5001, 5001])     # (two one-byte windows and an empty one)
    v = _dev(data, 3, guard=rs)
    ends, ctx = [], b""
    edges = [0, *cuts, len(data)]
    for lo, hi in zip(edges, edges[1:]):
        rc, n, off, ctx, tl = _split(v[lo:hi], rs, ctx, base=lo)
        assert rc == 0
        ends += off[1:n + 1] if tl == 0 else off[1:n]
    if ends[-1] != len(data):
        ends.append(len(data))
    assert [0] + ends == want


# ---------------------------------------------------------------------------------------------------------- Program.run_records
def _want_records(blob, data, rs):
    """(stdout, stderr, per-record results) that record mode must give, from the model and the oracle on every record."""
    offs = model(data, rs)[0]
    out, err, res = [], [], []
    for i in range(len(offs) - 1):
        rec = data[offs[i]:offs[i + 1]]
        try:
            o = oracle.run(blob, rec)
            out.append(o)
            res.append(o)
        except oracle.OracleMatchError as e:
            err.append("Match error at input symbol %d in record %d!\n" % (e.pos, i + 1))
            res.append((e.pos, e.stage))
    return b"".join(out), "".join(err).encode(), res


_BLOBS, _BINS = {}, {}


def _blob(src):
    if src not in _BLOBS:
        _BLOBS[src] = host.compile_file(src)
    return _BLOBS[src]


def _crlf_src(tmp_path_factory):
    p = tmp_path_factory.getbasetemp() / "crlf_records.kex"
    if not p.exists():
        p.write_text(CRLF)
    return str(p)


def _crlf_data(r, nrec, long_at=None):
    recs = []
    for i in range(nrec):
        body = b"".join(r.choice([b"field ", b"x", b"multi\nline ", b"\n", b"\n\n", b"tab\t"]) for _ in range(r.randrange(0, 12)))
        if i % 11 == 5:
            body += b"bare\rcr"                                       # rejected: a \r that starts no \r\n
        if i == long_at:
            body = body * 40 + b"long\n" * 2000
        recs.append(body + b"\r\n")
    return b"".join(recs)


def _as_res(got):
    return [(g.pos, g.stage) if isinstance(g, MatchError) else g for g in got]


def test_run_records_crlf_with_bare_newlines(tmp_path_factory):
    blob = _blob(_crlf_src(tmp_path_factory))
    data = _crlf_data(random.Random(7), 600) + b"no terminator\nat the end"
    _, _, want = _want_records(blob, data, b"\r\n")
    got = Program(blob).run_records(data, rs=b"\r\n")
    assert _as_res(got) == want
    assert sum(isinstance(w, tuple) for w in want) > 20 and len(want) == 601
    assert len(Program(blob).run_records(data)) != len(want)          # (the line split cuts these records)


def test_run_records_paragraphs():
    blob = _blob(PARAGRAPHS)
    r = random.Random(9)
    paras = []
    for i in range(400):
        lines = [b" ".join(r.choice([b"lorem", b"ipsum", b"dolor", b"sit"]) for _ in range(r.randrange(1, 9))) for _ in range(r.randrange(1, 6))]
        paras.append(b"\n".join(lines) + (b"\n\n\n" if i % 13 == 4 else b"\n\n"))   # three newlines: the next paragraph starts with one
    data = b"".join(paras) + b"last one\nwith a single newline\n"
    _, _, want = _want_records(blob, data, b"\n\n")
    got = Program(blob).run_records(data, rs=b"\n\n")
    assert _as_res(got) == want
    assert 20 < sum(isinstance(w, tuple) for w in want) < 40 and want[0].count(b"\n") == 1 and want[-1] == b"last one with a single newline\n"


# ---------------------------------------------------------------------------------------------------------- BIN --records --rs
def _bin(tmp_path_factory, src):
    if src not in _BINS:
        exe = tmp_path_factory.mktemp("recrsbin") / "bin"
        r = subprocess.run([KEXC, "compile", "--quiet", src, "--out", str(exe)], stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr
        _BINS[src] = str(exe)
    return _BINS[src]


def _check_bin(exe, blob, data, rs, spelling, window):
    out, err, _ = _want_records(blob, data, rs)
    env = dict(os.environ, KX_WINDOW_BYTES=str(window))
    r = subprocess.run(["timeout", "-k", "10", "300", exe, "--records", "--rs=" + spelling], input=data, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env, timeout=330)
    assert r.returncode == (1 if err else 0), (r.returncode, r.stderr[-500:])
    assert r.stderr == err, (r.stderr[:300], err[:300])
    assert r.stdout == out, (len(r.stdout), len(out))


def test_binary_with_small_windows(tmp_path_factory):
    """4 KiB windows: separators straddle window borders at both splits, one record is longer than many windows."""
    src = _crlf_src(tmp_path_factory)
    blob, exe = _blob(src), _bin(tmp_path_factory, src)
    W = 4096
    data = _crlf_data(random.Random(11), 900, long_at=300)
    for k in (W - 1, W, W + 1):                                       # the \r at byte k - 1, the \n at byte k, right around a window border
        pre = b"m" * (k - 1) + b"\r\n"
        _check_bin(exe, blob, pre + data, b"\r\n", "\\r\\n", W)
    _check_bin(exe, blob, data[:-2], b"\r\n", "\\r\\n", W)            # no terminator at the end
    _check_bin(exe, blob, data + b"\r", b"\r\n", "\\x0d\\x0a", W)      # half a separator at the end
    _check_bin(exe, blob, b"", b"\r\n", "\\r\\n", W)
    pblob, pexe = _blob(PARAGRAPHS), _bin(tmp_path_factory, PARAGRAPHS)
    data = b"".join(b"line %d\nmore\n\n" % i + (b"\n" if i % 50 == 7 else b"") for i in range(1500))
    _check_bin(pexe, pblob, data, b"\n\n", "\\n\\n", W)
    _check_bin(pexe, pblob, b"x" * (W - 1) + b"\n\n\n\n\n" + data, b"\n\n", "\\n\\n", W)
