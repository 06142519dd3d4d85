"""GPU: record mode.  kx_split_records against the offsets model; Program.run_records and `BIN --records` with every record checked
against the CPU oracle run on that record alone: stdout is the concatenation of the accepted records' outputs, stderr one exact
line per rejected record, the exit status 0 or 1."""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest
from conftest import GOLDEN, blob_of

from kleenexlang_amd import build, host, program_path, workloads
from kleenexlang_amd.host import MatchError, Program
from oracle import oracle

pytestmark = pytest.mark.gpu

PROGRAMS = sorted(f[:-4] for f in os.listdir(host.PROGRAM_DIR) if f.endswith(".kex"))
LINE_SHAPE = dict(workloads.PROGRAM_INPUT, add_commas="numbers")
KEXC = os.path.join(build.OUT, "kexc")
PIPELINE = 'start: a >> b\na := (~/x/ "Q" | /[a-wyz\\n]/)*\nb := /[a-z\\n]*/\n'
ACTIONS = json.load(open(os.path.join(GOLDEN, "action_vectors.json")))
ACTIONS = next(t for t in ACTIONS["line_tests"] if t["name"] == "actionbug")["program"]


def _want_records(blob, data, sep=b"\n"):
    """(stdout, stderr lines, per-record results) that record mode must give, from the oracle on every record alone."""
    offs = host.split_records_model(data, sep)
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


def _lines(name, nbytes, seed=3):
    if name in LINE_SHAPE:
        return workloads.generate(LINE_SHAPE[name], nbytes, seed=seed)
    r = random.Random(seed)
    parts, n = [], 0
    while n < nbytes:
        p = bytes(r.choice(b"ab") for _ in range(r.randint(0, 60))) + b"\n"
        parts.append(p)
        n += len(p)
    return b"".join(parts)


def _corrupt(data, every=7, seed=1):
    """Every `every`-th line damaged: a byte no program's lines hold, at the start, the middle or just before the newline."""
    r = random.Random(seed)
    lines = data.split(b"\n")
    for i in range(0, len(lines) - 1, every):
        l = lines[i]
        k = r.choice([0, len(l) // 2, max(0, len(l) - 1)])
        lines[i] = l[:k] + b"\x01" + l[k:]
    return b"\n".join(lines)


_BINS = {}


def _bin(tmp_path_factory, prog):
    """`kexc compile … --out BIN` for a workload name or an inline source (cached per session)."""
    if prog not in _BINS:
        d = tmp_path_factory.mktemp("recbin")
        src = program_path(prog) if ":=" not in prog else str(d / "p.kex")
        if ":=" in prog:
            open(src, "w").write(prog)
        exe = d / "bin"
        r = subprocess.run([KEXC, "compile", "--quiet", src, "--out", str(exe)], stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr
        _BINS[prog] = str(exe)
    return _BINS[prog]


def _run_bin(exe, data, tmp_path, window=None, via_file=False, args=("--records",)):
    env = dict(os.environ)
    if window:
        env["KX_WINDOW_BYTES"] = str(window)
    if via_file:
        f = tmp_path / "in.dat"
        f.write_bytes(data)
        with open(f, "rb") as fi:
            return subprocess.run(["timeout", "-k", "10", "600", exe, *args], stdin=fi, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                                  timeout=660)
    return subprocess.run(["timeout", "-k", "10", "600", exe, *args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                          timeout=660)


def _check_bin(exe, blob, data, tmp_path, **kw):
    out, err, _ = _want_records(blob, data)
    r = _run_bin(exe, data, tmp_path, **kw)
    assert r.returncode == (1 if err else 0), (r.returncode, r.stderr[-500:])
    assert r.stderr == err, (r.stderr[:300], err[:300])
    assert r.stdout == out, (len(r.stdout), len(out))
    return r


# ---------------------------------------------------------------------------------------------------------- kx_split_records
def _split(view, sep=b"\n", base=0, cap=None):
    """kx_split_records on a device view: (rc, n_records, offsets list)."""
    import torch
    lib = host.load_engine()
    n = ctypes.c_uint64()
    cap = view.numel() + 2 if cap is None else cap
    off = torch.full((max(cap, 1),), -1, dtype=torch.int64, device="cuda")
    rc = lib.kx_split_records(ctypes.c_void_p(view.data_ptr() if view.numel() else None), view.numel(), host._check_sep(sep), base,
                              ctypes.c_void_p(off.data_ptr() if cap else None), cap, ctypes.byref(n), None)
    torch.cuda.synchronize()
    return rc, n.value, off.tolist()


def _dev(data, lead=0):
    """data on the device at `lead` bytes past a 256-byte aligned allocation, with guard bytes around it."""
    import torch
    buf = torch.full((lead + len(data) + 64,), 0x0A, dtype=torch.uint8)
    if data:
        buf[lead:lead + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return buf.cuda()[lead:lead + len(data)]


def test_split_kernel_edge_cases_phases_lengths_and_slices():
    cases = [(b"", b"\n"), (b"abc", b"\n"), (b"\n", b"\n"), (b"\n" * 37, b"\n"), (b"ab\ncd\n", b"\n"), (b"ab\ncd", b"\n"),
             (b"a\0b\0\0c", b"\0"), (b"\xff\xfex\xff", b"\xff"), (b"\x7f\x80\x00\xff" * 9, b"\x80"), (b"\x0a\x0b" * 40, b"\x0b")]
    r = random.Random(5)
    for phase in range(16):                     # a separator at every byte phase of a granule, alone and in pairs
        cases.append((b"x" * phase + b"\n" + b"y" * (40 - phase), b"\n"))
        cases.append((b"x" * phase + b",," + b"y" * 13, b","))
    for n in list(range(1, 70)) + [127, 129, 1000, 4095, 4097]:   # lengths that are not multiples of 16
        cases.append((bytes(r.choice(b"ab\n\x00") for _ in range(n)), b"\n"))
    for data, sep in cases:
        want = host.split_records_model(data, sep)
        for lead in (0, 1, 7, 15):
            rc, n, off = _split(_dev(data, lead), sep)
            assert rc == 0 and n == len(want) - 1 and off[:n + 1] == want, (data[:40], sep, lead, off[:n + 2])
            assert off[n + 1] == -1                       # nothing written past the last offset
        rc, n, off = _split(_dev(data, 3), sep, base=1000003)   # a slice: base != 0
        assert rc == 0 and off[:n + 1] == [1000003 + x for x in want]


def test_split_kernel_capacity_query():
    data = b"one\ntwo\nthree"
    v = _dev(data, 5)
    assert _split(v, cap=0)[:2] == (-3, 3)
    rc, n, off = _split(v, cap=3)
    assert (rc, n) == (-3, 3) and off[:3] == [-1, -1, -1]    # too small: nothing written
    rc, n, off = _split(v, cap=4)
    assert (rc, n, off) == (0, 3, [0, 4, 8, 13])
    assert _split(_dev(b""), cap=0)[:2] == (-3, 0)
    assert _split(_dev(b""), cap=1) == (0, 0, [0])


def test_split_kernel_on_a_few_hundred_megabytes():
    """Several thousand tiles: the tile scan and every tile's prefix; random bytes with a dense separator, at an odd start."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(9)
    n = 300 * 1000 * 1000 + 13
    for sep, hi in ((ord("\n"), 40), (0, 256)):
        buf = torch.randint(0, hi, (n + 32,), dtype=torch.uint8, device="cuda", generator=g)
        v = buf[5:5 + n]
        offs = host.split_records_tensor(v, bytes([sep]))
        h = v.cpu().numpy()
        pos = np.flatnonzero(h == sep).astype(np.int64) + 1
        want = np.concatenate([[0], pos, [n]] if pos[-1] != n else [[0], pos])
        got = offs.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want)
        del buf, v, offs
    big = torch.full((1 << 26,), ord("\n"), dtype=torch.uint8, device="cuda")   # a separator in every byte
    offs = host.split_records_tensor(big)
    assert offs.numel() == (1 << 26) + 1 and bool((offs == torch.arange((1 << 26) + 1, device="cuda")).all())


# ---------------------------------------------------------------------------------------------------------- Program.run_records
@pytest.mark.parametrize("name", PROGRAMS)
def test_run_records_on_every_program_with_corrupted_lines(name):
    blob = blob_of(name)
    data = _corrupt(_lines(name, 200000))
    data += b"tail without separator"
    _, _, want = _want_records(blob, data)
    got = Program(blob).run_records(data)
    assert len(got) == len(want)
    assert any(isinstance(w, bytes) for w in want)
    assert any(isinstance(w, tuple) for w in want) == (name != "add_commas")   # (add_commas copies any byte it does not rewrite)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, tuple):
            assert isinstance(g, MatchError) and (g.pos, g.stage) == w, (i, g, w)
        else:
            assert g == w, i


def test_run_records_with_other_separators_and_nothing():
    blob = blob_of("flip_ab")
    prog = Program(blob)
    assert prog.run_records(b"") == []
    for data, sep in ((b"ab\0ba\0b", b"\0"), (b"ab\nba,b\n", b","), (b"a\xffb\n\xff\xff", b"\xff")):
        got = prog.run_records(data, sep=sep)
        assert [(g.pos, g.stage) if isinstance(g, MatchError) else g for g in got] == _want_records(blob, data, sep)[2]


# ---------------------------------------------------------------------------------------------------------- BIN --records
@pytest.mark.parametrize("window", [4096, 65536, None])
def test_binary_pipe_and_file_against_the_oracle(tmp_path_factory, tmp_path, window):
    for name in ("apache_log", "csv2json"):
        blob = blob_of(name)
        exe = _bin(tmp_path_factory, name)
        data = _corrupt(_lines(name, 300000, seed=window or 1), every=11)
        _check_bin(exe, blob, data, tmp_path, window=window)
        _check_bin(exe, blob, data, tmp_path, window=window, via_file=True)
        _check_bin(exe, blob, data[:-1], tmp_path, window=window)   # no trailing separator


def test_long_records_straddle_and_route(tmp_path_factory, tmp_path):
    """A 20 KiB and a 100 KiB record in 4 KiB windows: both are carried over several windows; the second is longer than
    batch_doc_max (64 KiB) and so takes the single-document route."""
    blob = blob_of("thousand_sep")
    exe = _bin(tmp_path_factory, "thousand_sep")
    r = random.Random(2)
    digits = lambda k: bytes(r.choice(b"0123456789") for _ in range(k))
    recs = [digits(r.randint(1, 30)) + b"\n" for _ in range(50)]
    recs[10] = digits(20 * 1024) + b"\n"
    recs[30] = digits(100 * 1024) + b"\n"
    recs[40] = digits(30000) + b"x" + digits(10) + b"\n"     # a long rejected one
    data = b"".join(recs)
    for window in (4096, 65536):
        _check_bin(exe, blob, data, tmp_path, window=window)
    f = tmp_path / "long.in"
    f.write_bytes(data)
    prog = Program(blob, window_bytes=4096, collect_timing=True)
    with open(f, "rb") as fi, open(tmp_path / "long.out", "wb") as fo, open(tmp_path / "long.err", "wb") as fe:
        st = prog.run_records_fd(fi.fileno(), fo.fileno(), report_fd=fe.fileno())
    out, err, _ = _want_records(blob, data)
    assert (tmp_path / "long.out").read_bytes() == out and (tmp_path / "long.err").read_bytes() == err
    assert st["rejected"] and st["records"] == 50 and st["records_rejected"] == 1 and st["records_routed"] == 1
    assert st["longest_record"] == 100 * 1024 + 1 and st["in_bytes"] == len(data) and st["out_bytes"] == len(out)
    assert st["windows"] >= len(data) // 4096


def test_empty_input_pipeline_and_actions(tmp_path_factory, tmp_path):
    exe = _bin(tmp_path_factory, "apache_log")
    r = _run_bin(exe, b"", tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    r = _run_bin(exe, b"", tmp_path, via_file=True, args=("-t", "--records"))
    assert r.returncode == 0 and r.stdout == b"" and r.stderr.startswith(b"time (ms): ")
    # a two-stage pipeline: rejections at either stage
    blob = host.compile_source(PIPELINE)
    exe = _bin(tmp_path_factory, PIPELINE)
    r = random.Random(8)
    data = b"".join(bytes(r.choice(b"abxz1") for _ in range(r.randint(0, 12))) + b"\n" for _ in range(400))
    _check_bin(exe, blob, data, tmp_path)
    _check_bin(exe, blob, data, tmp_path, window=4096)
    # register actions: every record takes the single-document route
    blob = host.compile_source(ACTIONS)
    exe = _bin(tmp_path_factory, ACTIONS)
    data = b"".join(r.choice([b"c\n", b"cc\n", b"\n", b"ccc\n", b"cx\n", b"x\n"]) for _ in range(40))
    _check_bin(exe, blob, data, tmp_path)


def test_sixteen_million_one_byte_records(tmp_path_factory, tmp_path):
    blob = blob_of("flip_ab")
    exe = _bin(tmp_path_factory, "flip_ab")
    one = oracle.run(blob, b"\n")
    data = b"\n" * (1 << 24)
    for via_file in (False, True):
        r = _run_bin(exe, data, tmp_path, via_file=via_file)
        assert (r.returncode, r.stderr) == (0, b"") and r.stdout == one * (1 << 24)


@pytest.mark.parametrize("name", ["csv2json", "iso_datetime_to_json", "thousand_sep"])
def test_all_accepted_record_programs_give_the_whole_stream_bytes(tmp_path_factory, tmp_path, name):
    exe = _bin(tmp_path_factory, name)
    data = _lines(name, 2 << 20, seed=6)
    whole = subprocess.run(["timeout", "-k", "10", "600", exe], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=660)
    assert whole.returncode == 0 and whole.stdout == oracle.run(blob_of(name), data)
    for window in (4096, None):
        r = _run_bin(exe, data, tmp_path, window=window)
        assert (r.returncode, r.stderr) == (0, b"") and r.stdout == whole.stdout
