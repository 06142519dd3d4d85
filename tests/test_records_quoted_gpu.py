"""GPU: quote-aware record mode.  kx_split_records_quoted against the offsets model (split_records_model with a quote);
Program.run_records(quote=…) and `BIN --records --quote` with every record checked against the CPU oracle run on that record
alone: stdout is the concatenation of the accepted records' outputs, stderr one exact line per rejected record, the exit status
0 or 1."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest
from conftest import blob_of

from kleenexlang_amd import build, host, workloads
from kleenexlang_amd.host import MatchError, Program
from oracle import oracle

pytestmark = pytest.mark.gpu

KEXC = os.path.join(build.OUT, "kexc")
EXAMPLE = os.path.join(build.ROOT, "kleenexlang_amd", "examples", "csv_rfc4180.kex")
Q = b'"'


def _want_records(blob, data, sep=b"\n", quote=Q):
    """(stdout, stderr, per-record results) that quoted record mode must give, from the model and the oracle on every record."""
    offs = host.split_records_model(data, sep, quote)
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


_BLOB = []


def _csv_blob():
    if not _BLOB:
        _BLOB.append(host.compile_file(EXAMPLE))
    return _BLOB[0]


def _corrupt_rfc(data, every=9, seed=1):
    """Every `every`-th row damaged: a stray quote inside a bare field, or a byte after a closing quote (a bad field)."""
    r = random.Random(seed)
    offs = host.split_records_model(data, quote=Q)
    rows = [data[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    for i in range(0, len(rows) - 1, every):
        row = rows[i]
        if r.random() < 0.5 and b'"' in row:
            k = row.rindex(b'"') + 1
            rows[i] = row[:k] + b"x" + row[k:]           # "..."x  — balanced, rejected
        else:
            rows[i] = b"ab" + Q + b"c" + Q + b"," + row   # ab"c",  — a bad bare field, balanced
    return b"".join(rows)


# ---------------------------------------------------------------------------------------------------------- kx_split_records_quoted
def _split(view, sep=b"\n", quote=Q, parity=0, base=0, cap=None):
    """kx_split_records_quoted on a device view: (rc, n_records, offsets list, parity_out)."""
    import torch
    lib = host.load_engine()
    n, po = ctypes.c_uint64(), ctypes.c_uint32(7)
    cap = view.numel() + 2 if cap is None else cap
    off = torch.full((max(cap, 1),), -1, dtype=torch.int64, device="cuda")
    rc = lib.kx_split_records_quoted(ctypes.c_void_p(view.data_ptr() if view.numel() else None), view.numel(), host._check_sep(sep),
                                     host._check_sep(quote), parity, base, ctypes.c_void_p(off.data_ptr() if cap else None), cap,
                                     ctypes.byref(n), ctypes.byref(po), None)
    torch.cuda.synchronize()
    return rc, n.value, off.tolist(), po.value


def _dev(data, lead=0):
    """data on the device at `lead` bytes past a 256-byte aligned allocation, with guard bytes (separators and quotes) around it."""
    import torch
    buf = torch.tensor(list(b'\n"') * ((lead + len(data) + 64) // 2 + 1), dtype=torch.uint8)
    if data:
        buf[lead:lead + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return buf.cuda()[lead:lead + len(data)]


def _check(data, sep=b"\n", quote=Q, parity=0, lead=0, base=0):
    want = host.split_records_model(data, sep, quote, parity)
    rc, n, off, po = _split(_dev(data, lead), sep, quote, parity, base)
    assert rc == 0 and n == len(want) - 1, (data[:40], lead, parity, n, len(want) - 1)
    assert off[:n + 1] == [base + x for x in want], (data[:40], lead, parity)
    assert off[n + 1] == -1                                       # nothing written past the last offset
    assert po == parity ^ (data.count(quote) & 1)


def test_quoted_split_small_lengths_at_every_alignment():
    r = random.Random(5)
    for n in range(0, 300):
        data = bytes(r.choice(b'ab\n"\n"') for _ in range(n))
        for lead in range(16):
            _check(data, lead=lead, parity=(n + lead) & 1)
    for phase in range(16):                                       # a quote and a separator at every byte phase of a granule
        _check(b"x" * phase + b'"\n"\n' + b"y" * (40 - phase), lead=3)
        _check(b"x" * phase + b'\n"' + b"y" * 13 + b"\n", lead=phase)
    for data, sep, quote in ((b"a,'b,c',d", b",", b"'"), (b'a\0"\0"\0b', b"\0", b'"'), (b"a\n\0\n\0\n", b"\n", b"\0"),
                             (b"\xff\xfe\xff\xfe" * 9, b"\xff", b"\xfe"), (b"\x7f\x80\x00\xff" * 9, b"\x80", b"\x00")):
        for parity in (0, 1):
            _check(data, sep, quote, parity, lead=1)
    _check(b'a"\nb\n"c\n', base=1000003, lead=7)


def test_quoted_split_all_quotes_all_separators_and_capacity():
    for n in (1, 15, 16, 17, 4096, 65536, 65537, 3 * 65536 + 5):
        for parity in (0, 1):
            _check(b'"' * n, parity=parity, lead=n % 16)
            _check(b"\n" * n, parity=parity, lead=n % 16)
    v = _dev(b'one\n"t\nwo"\nthree', 5)
    assert _split(v, cap=0)[:2] == (-3, 3)
    rc, n, off, po = _split(v, cap=3)
    assert (rc, n, po) == (-3, 3, 0) and off[:3] == [-1, -1, -1]    # too small: nothing written
    assert _split(v, cap=4) == (0, 3, [0, 4, 11, 16], 0)
    assert _split(_dev(b""), cap=0)[:2] == (-3, 0)
    assert _split(_dev(b""), cap=1, parity=1) == (0, 0, [0], 1)
    assert _split(v, quote=b"\n")[0] == -4 and _split(v, parity=2)[0] == -4   # KX_E_ARG


def test_quoted_split_around_tile_and_granule_edges():
    """Tiles are 64 KiB: quotes placed so that the parity flips exactly at a tile or a granule edge, and records that span tiles."""
    T = 65536
    r = random.Random(7)
    for lead in (0, 1, 15):
        for edge in (T, 2 * T, T + 16, T - 16):
            for d in (-1, 0, 1):
                k = edge - lead + d
                if k < 0:
                    continue
                data = bytearray(r.choice(b"abc\n") for _ in range(3 * T + 100))
                data[k] = ord('"')                              # the parity flips at (or next to) the edge ...
                data[k + 1] = ord("\n")                        # ... right before a separator it then hides
                data[k + 40000] = ord('"')                      # and closes in the next tile
                for parity in (0, 1):
                    _check(bytes(data), parity=parity, lead=lead)
    data = bytearray(b"x" * (4 * T))
    for i in range(16, len(data), 16):                           # a quote at every granule start: parity flips each granule
        data[i] = ord('"')
    for i in range(8, len(data), 16):
        data[i] = ord("\n")
    _check(bytes(data))
    _check(bytes(data), parity=1, lead=9)


def test_quoted_split_on_a_few_hundred_megabytes():
    import torch
    g = torch.Generator(device="cuda").manual_seed(9)
    n = 300 * 1000 * 1000 + 13
    for qdensity in (2, 40, 4000):                               # a quote in about 1 / qdensity bytes
        u = torch.randint(0, 40 * qdensity, (n + 32,), dtype=torch.int32, device="cuda", generator=g)
        b = torch.full((n + 32,), ord("a"), dtype=torch.uint8, device="cuda")
        b[u < qdensity] = ord("\n")                                          # a separator in about 1 / 40 bytes
        b[(u >= qdensity) & (u < qdensity + 40)] = ord('"')
        del u
        v = b[5:5 + n]
        for parity in (0, 1):
            offs, po = host.split_quoted_records_tensor(v, b"\n", Q, parity)
            h = v.cpu().numpy()
            isq = h == 34
            par = (np.cumsum(isq, dtype=np.int64) + parity) & 1           # parity after each byte (= at a separator)
            pos = np.flatnonzero((h == 10) & (par == 0)).astype(np.int64) + 1
            want = np.concatenate([[0], pos] if len(pos) and pos[-1] == n else [[0], pos, [n]])
            got = offs.cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), (qdensity, parity)
            assert po == (parity + int(isq.sum())) & 1
            del offs
        del b, v


# ---------------------------------------------------------------------------------------------------------- Program.run_records
def _as_res(got):
    return [(g.pos, g.stage) if isinstance(g, MatchError) else g for g in got]


def test_run_records_quoted_on_rfc4180_with_bad_rows():
    blob = _csv_blob()
    data = _corrupt_rfc(workloads.generate("rfc4180", 300000, seed=4))
    data += b'stray "quote, to the end\nand on\n'
    _, _, want = _want_records(blob, data)
    got = Program(blob).run_records(data, quote=Q)
    assert _as_res(got) == want
    assert sum(isinstance(w, tuple) for w in want) > 20 and isinstance(want[-1], tuple)


def test_run_records_quoted_on_apache_log_equals_the_line_split():
    blob = blob_of("apache_log")
    data = workloads.generate("apache_log", 400000, seed=2)
    assert host.split_records_model(data, quote=Q) == host.split_records_model(data)
    got = Program(blob).run_records(data, quote=Q)
    assert _as_res(got) == _want_records(blob, data)[2]
    assert _as_res(got) == _as_res(Program(blob).run_records(data))


# ---------------------------------------------------------------------------------------------------------- BIN --records --quote
_BINS = {}


def _bin(tmp_path_factory, src):
    if src not in _BINS:
        exe = tmp_path_factory.mktemp("recqbin") / "bin"
        r = subprocess.run([KEXC, "compile", "--quiet", src, "--out", str(exe)], stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr
        _BINS[src] = str(exe)
    return _BINS[src]


def _run_bin(exe, data, tmp_path, window=None, via_file=False, args=("--records", "--quote")):
    env = dict(os.environ)
    if window:
        env["KX_WINDOW_BYTES"] = str(window)
    cmd = ["timeout", "-k", "10", "600", exe, *args]
    if via_file:
        f = tmp_path / "in.dat"
        f.write_bytes(data)
        with open(f, "rb") as fi:
            return subprocess.run(cmd, stdin=fi, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=660)
    return subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=660)


def _check_bin(exe, blob, data, tmp_path, **kw):
    out, err, _ = _want_records(blob, data)
    r = _run_bin(exe, data, tmp_path, **kw)
    assert r.returncode == (1 if err else 0), (r.returncode, r.stderr[-500:])
    assert r.stderr == err, (r.stderr[:300], err[:300])
    assert r.stdout == out, (len(r.stdout), len(out))
    return r


@pytest.mark.parametrize("window", [4096, 65536, None])
def test_binary_pipe_and_file_against_the_oracle(tmp_path_factory, tmp_path, window):
    blob = _csv_blob()
    exe = _bin(tmp_path_factory, EXAMPLE)
    data = _corrupt_rfc(workloads.generate("rfc4180", 300000, seed=window or 1), every=13)
    _check_bin(exe, blob, data, tmp_path, window=window)
    _check_bin(exe, blob, data, tmp_path, window=window, via_file=True)
    _check_bin(exe, blob, data[:-1], tmp_path, window=window)   # no trailing separator
    # apache_log: balanced quotes in every line, so the quoted split is the line split
    blob = blob_of("apache_log")
    exe = _bin(tmp_path_factory, host.program_path("apache_log"))
    data = workloads.generate("apache_log", 200000, seed=5)
    r = _check_bin(exe, blob, data, tmp_path, window=window)
    assert r.stdout == _run_bin(exe, data, tmp_path, window=window, args=("--records",)).stdout


def test_window_edges_inside_quotes_and_doubled_quotes(tmp_path_factory, tmp_path):
    """4 KiB windows whose boundaries fall inside a quoted field, between the two bytes of a "", and right after a quote."""
    blob = _csv_blob()
    exe = _bin(tmp_path_factory, EXAMPLE)
    W = 4096
    for where in (-2, -1, 0, 1, 2):
        head = b"a,b\n" * ((W - 40) // 4)
        pad = W - len(head) - 4 + where
        row = b'x,"' + b"q" * pad + b'""' + b"\n,\n" * 3 + b'"' + b',z\n'   # the "" at bytes W - 1 + where, W + where
        data = head + row + b'"1\n2",3\n' * 50
        _check_bin(exe, blob, data, tmp_path, window=W)
        _check_bin(exe, blob, data, tmp_path, window=W, via_file=True)
    for k in range(W - 3, W + 3):                                  # a "" split by the window end at every offset near it
        data = b'p,"' + b"m" * (k - 4) + b'a""b\nc"\n' + b'd,"e\nf"\n' * 700   # the "" at bytes k, k + 1
        _check_bin(exe, blob, data, tmp_path, window=W)


def test_long_quoted_record_over_many_windows_and_a_stray_quote(tmp_path_factory, tmp_path):
    blob = _csv_blob()
    exe = _bin(tmp_path_factory, EXAMPLE)
    r = random.Random(3)
    field = b"".join(r.choice([b"ab", b"\n", b",", b'""', b"\r\n", b"cd"]) for _ in range(60000))   # ~150 KiB, many quoted separators
    data = b"h1,h2\n" + b'k,"' + field + b'"\n' + b"1,2\n" * 100
    for window in (4096, 65536):
        res = _check_bin(exe, blob, data, tmp_path, window=window)
        assert res.returncode == 0 and res.stdout.count(b"\n") == 102
    prog = Program(blob, window_bytes=4096)
    f = tmp_path / "long.in"
    f.write_bytes(data)
    with open(f, "rb") as fi, open(tmp_path / "long.out", "wb") as fo:
        st = prog.run_records_fd(fi.fileno(), fo.fileno(), quote=Q)
    assert (tmp_path / "long.out").read_bytes() == oracle.run(blob, data)
    assert st["records"] == 102 and not st["rejected"] and st["longest_record"] == len(field) + 5 and st["records_routed"] == 1
    # a stray quote with no quote after it: the rest of the stream is one last record, rejected once
    good = workloads.generate("rfc4180", 50000, seed=8)
    data = good + b'a,b"c,d\n' + b"1,2,3\n" * 3000
    for window in (4096, None):
        res = _check_bin(exe, blob, data, tmp_path, window=window)
        assert res.returncode == 1 and res.stderr.count(b"\n") == 1
        assert res.stderr.endswith(b" in record %d!\n" % (len(host.split_records_model(good, quote=Q))))


def test_all_accepted_rfc4180_gives_the_whole_stream_bytes(tmp_path_factory, tmp_path):
    exe = _bin(tmp_path_factory, EXAMPLE)
    data = workloads.generate("rfc4180", 2 << 20, seed=6)
    whole = subprocess.run(["timeout", "-k", "10", "600", exe], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=660)
    assert whole.returncode == 0 and whole.stdout == oracle.run(_csv_blob(), data)
    for window in (4096, None):
        r = _run_bin(exe, data, tmp_path, window=window)
        assert (r.returncode, r.stderr) == (0, b"") and r.stdout == whole.stdout
    r = _run_bin(exe, b"", tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
