"""CPU: escape-aware record mode (kx_split_records_escaped / kx_run_records_fd_escaped, `BIN --records --escape[=E]`) — the
offsets model's edge cases and its row count against csv.reader, the granule rule of the kernels restated and checked
exhaustively, the example program on the oracle, the ABI, the command line's escape spellings and refusals, and the Python
binding's argument checks.  Nothing here needs a device."""
import csv
import ctypes
import io
import json
import os
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path, workloads
from oracle import oracle

INC = os.path.join(build.ROOT, "include")
EXAMPLE = os.path.join(build.ROOT, "kleenexlang_amd", "examples", "csv_escaped.kex")
ISSUE_INPUT = b'a,"b\\"c",d\\\ne\n"x\ny",\\\\\n1,2\\,3,\\"q\n'


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def _reader_rows(data):
    return list(csv.reader(io.StringIO(data.decode("ascii"), newline=""), escapechar="\\", doublequote=False))


def _spec_model(data, sep=b"\n", quote=None, escape=b"\\", state=0):
    """The byte-by-byte statement of the split (the issue's normative model), to hold the faster host model to."""
    s, e = sep[0], escape[0]
    q = None if quote is None else quote[0]
    p, x, offs = state & 1, state >> 1, [0]
    for i, b in enumerate(data):
        if x:
            x = 0
        elif b == e:
            x = 1
        elif b == q:
            p ^= 1
        elif b == s and p == 0:
            offs.append(i + 1)
    if offs[-1] != len(data):
        offs.append(len(data))
    return offs, p | x << 1


def test_escaped_model_edge_cases():
    m = lambda d, sep=b"\n", quote=None, escape=b"\\", state=0: host.split_escaped_records_model(d, sep, quote, escape, state)
    assert m(b"") == ([0], 0) and m(b"", state=2) == ([0], 2) and m(b"", quote=b'"', state=3) == ([0], 3)
    assert m(b"a\\\nb\nc") == ([0, 5, 6], 0)                    # an escaped separator ends no record
    assert m(b"a\\\\\nb\n") == ([0, 4, 6], 0)                   # \\ is a literal backslash: the byte after it is live again
    assert m(b"a\\\\\\\nb\n") == ([0, 7], 0)                    # \\\ + LF: the LF is escaped
    assert m(b"ab\\") == ([0, 3], 2)                            # an escape as the last byte ends the tail record; state bit 1
    assert m(b"ab\n\\") == ([0, 3, 4], 2)
    assert m(b"ab\\\n") == ([0, 4], 0)                          # a buffer ending in an escaped separator has a tail
    assert m(b"ab\n") == ([0, 3], 0)                            # (an unescaped one has none)
    assert m(b'a\\"\nb\n', quote=b'"') == ([0, 4, 6], 0)        # an escaped quote outside quotes flips nothing
    assert m(b'"a\\"\nb"\nc', quote=b'"') == ([0, 8, 9], 0)     # ... nor inside quotes
    assert m(b'"a\\\\"\nb\n', quote=b'"') == ([0, 6, 8], 0)     # \\ then a real closing quote
    assert m(b'"\\\n"\n', quote=b'"') == ([0, 5], 0)            # an escaped separator inside quotes
    assert m(b'x\n', quote=b'"', state=1) == ([0, 2], 1)        # parity 1: the separator is inside quotes
    assert m(b'\nx\n', state=2) == ([0, 3], 0)                  # escaped first byte: the first separator is data
    assert m(b'\\\nx\n', state=2) == ([0, 2, 4], 0)             # escaped first escape: the separator after it is live
    assert m(b'"\n', quote=b'"', state=2) == ([0, 2], 0)        # escaped first quote: no parity flip
    assert m(b'"\n', quote=b'"', state=3) == ([0, 2], 1)
    for e in (b"\0", b"^", b"\xff"):                            # other escape bytes
        d = b"a" + e + b"\nb\n" + e + e + b"\nc" + e
        assert m(d, escape=e) == ([0, 5, 8, 10], 2), e
        assert m(d.replace(b"\n", b","), b",", escape=e) == ([0, 5, 8, 10], 2), e
    assert m(b"a\\\nb\n", escape=b"^") == host.split_escaped_records_model(b"a\\\nb\n", escape=b"^") == ([0, 3, 5], 0)
    assert m(ISSUE_INPUT, quote=b'"')[0] == [0, 14, 23, 34] and len(_reader_rows(ISSUE_INPUT)) == 3
    assert m(b"\n" * 5)[0] == host.split_records_model(b"\n" * 5)   # no escape byte: the line split
    assert m(b'a"\n"b\nc', quote=b'"')[0] == host.split_records_model(b'a"\n"b\nc', quote=b'"')


def test_escaped_model_is_the_byte_by_byte_rule():
    import random
    r = random.Random(17)
    for _ in range(3000):
        d = bytes(r.choice(b'\\\\"\n\nab') for _ in range(r.randrange(0, 40)))
        for quote in (None, b'"'):
            for state in ((0, 2) if quote is None else (0, 1, 2, 3)):
                assert host.split_escaped_records_model(d, quote=quote, state=state) == _spec_model(d, quote=quote, state=state)


def _esc16(e, c):
    """The kernels' escaped mask of a 16-byte granule (kx_records_escaped.inc, re_esc): escape bits e, carry-in c."""
    EVEN = 0x5555
    b = e & ~c & 0xFFFF
    fe = b << 1 | c
    odd = b & ~EVEN & ~fe
    s = odd + b
    return (EVEN ^ (s << 1)) & fe & 0xFFFF, s >> 16


def test_granule_rule_exhaustively():
    """All 2^17 (escape pattern, carry-in): the branchless mask equals the sequential rule; the carry-out is the carry-in for
    a granule of 16 escapes and independent of it otherwise."""
    for e in range(1 << 16):
        outs = []
        for c in (0, 1):
            x, want = c, 0
            for i in range(16):
                if x:
                    want |= 1 << i
                    x = 0
                elif e >> i & 1:
                    x = 1
            got, co = _esc16(e, c)
            assert (got, co) == (want, x), (e, c)
            outs.append(co)
        assert (outs == [0, 1]) if e == 0xFFFF else outs[0] == outs[1], e


def test_escaped_model_counts_the_rows_csv_reader_counts():
    for seed in range(4):
        data = workloads.generate("csv_escaped", 300000, seed=seed)
        rows = _reader_rows(data)
        offs, st = host.split_escaped_records_model(data, quote=b'"')
        assert len(offs) - 1 == len(rows) and st == 0
        assert len(host.split_records_model(data, quote=b'"')) - 1 != len(rows)   # (escapes do matter on this data)
        for i in range(0, len(rows), 53):                                        # each record is one row
            assert _reader_rows(data[offs[i]:offs[i + 1]]) == [rows[i]]
    assert b"\\\n" in data and b"\\\"" in data and b"\r\n" in data and b"\\\\" in data and b",," in data


def test_generators_are_seeded_and_stay_off_the_program_table():
    for shape in ("csv_escaped", "tsv_escaped"):
        assert workloads.generate(shape, 50000, seed=3) == workloads.generate(shape, 50000, seed=3)
        assert shape not in workloads.PROGRAM_INPUT.values()
    assert not os.path.exists(os.path.join(host.PROGRAM_DIR, "csv_escaped.kex"))
    t = workloads.generate("tsv_escaped", 200000, seed=1)
    assert b'"' in t and b"\\\t" in t and b"\\\n" in t and b"\\\\" in t
    offs, st = host.split_escaped_records_model(t)
    assert st == 0 and len(offs) < len(host.split_records_model(t))
    assert b"\\" not in workloads.generate("apache_log", 400000, seed=2)     # (so --escape is --records there)


def test_escaped_abi_is_declared_and_exported():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_split_records_escaped", "kx_run_records_fd_escaped"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]
    assert args("kx_split_records_escaped") == ["d_in", "n", "sep", "quote", "escape", "state_in", "base", "d_off", "cap", "n_records",
                                                "state_out", "stream"]
    assert args("kx_run_records_fd_escaped") == ["p", "in_fd", "out_fd", "sep", "quote", "escape", "report_fd", "stats"]


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    f = lib.kx_split_records_escaped
    f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint8, ctypes.c_int, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64,
                  ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    n, so = ctypes.c_uint64(), ctypes.c_uint32()
    for sep, quote, esc, state in ((10, -1, 10, 0), (10, 34, 34, 0), (10, 10, 92, 0), (10, 256, 92, 0), (10, -2, 92, 0),
                                   (10, 34, 92, 4), (10, -1, 92, 1), (10, -1, 92, 3)):
        assert f(None, 0, sep, quote, esc, state, 0, None, 0, ctypes.byref(n), ctypes.byref(so), None) == -4, (sep, quote, esc, state)
    g = lib.kx_run_records_fd_escaped
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint8, ctypes.c_int, ctypes.c_uint8, ctypes.c_int, ctypes.c_void_p]
    assert g(None, 0, 1, 10, -1, 92, -1, None) == -4


# ---------------------------------------------------------------------------------------------------------- the example on the oracle
@pytest.fixture(scope="module")
def csv_blob():
    return host.compile_file(EXAMPLE)


def _records(blob, data, quote, escape):
    """(accepted outputs joined, rejected record numbers) of every record alone under the model."""
    offs = host.split_escaped_records_model(data, quote=quote, escape=escape)[0] if escape else host.split_records_model(data, quote=quote)
    out, bad = [], []
    for i in range(len(offs) - 1):
        try:
            out.append(oracle.run(blob, data[offs[i]:offs[i + 1]]))
        except oracle.OracleMatchError:
            bad.append(i + 1)
    return b"".join(out), bad


def test_example_program_on_the_oracle(csv_blob):
    assert oracle.run(csv_blob, ISSUE_INPUT) == b'["a", "b\\"c", "d\\ne"]\n["x\\ny", "\\\\"]\n["1", "2,3", "\\"q"]\n'
    with pytest.raises(oracle.OracleMatchError):
        oracle.run(csv_blob, b'a,b"c\n')
    data = workloads.generate("csv_escaped", 200000, seed=11)
    whole = oracle.run(csv_blob, data)
    assert whole == "".join(json.dumps(row) + "\n" for row in _reader_rows(data)).encode()   # independent of the .kex
    out, bad = _records(csv_blob, data, b'"', b"\\")
    assert bad == [] and out == whole                       # escaped split: the whole stream's bytes, record by record
    out, bad = _records(csv_blob, data, b'"', None)
    assert len(bad) > 10                                    # quoted split alone: escaped line breaks and quotes cut rows


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rece") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


@pytest.mark.parametrize("args", [["--records", "--escape"], ["--escape", "--records"], ["--records", "--escape=^"],
                                  ["--records", "--escape=\\x5c"], ["--records", "--escape=\\\\"], ["--records=,", "--escape=\\n"],
                                  ["--records", "--quote", "--escape"], ["--records", "--escape", "--quote='"],
                                  ["--records=\\t", "--escape=\\0"], ["-t", "--records", "--escape=\\r"], ["--records", "--escape=\\t"],
                                  ["--records", "--escape=\""]])
def test_good_escape_spellings_reach_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("arg", ["", "ab", "\\q", "\\x", "\\x4", "\\xg0", "\\x100", "\\nn", "\\\\\\", "\\N"])
def test_bad_escapes_are_refused_with_the_exact_message(flip_bin, arg):
    r = _run(flip_bin, "--records", "--escape=" + arg)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr == ("Invalid escape character: %s\n" % arg).encode()


def test_escape_refusals_before_loading(flip_bin):
    for args in (["--escape"], ["--escape=^"], ["-t", "--escape"], ["--escape=\\t"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": --escape needs --records\n").encode(), (args, r.stderr)
    for args in (["--records", "--escape=\\n"], ["--records=,", "--escape=,"], ["--records=\\x5c", "--escape"], ["--escape=\\x0a", "--records"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": the escape character cannot be the record separator\n").encode(), (args, r.stderr)
    for args in (["--records", "--quote", "--escape=\""], ["--records", "--quote=\\\\", "--escape"], ["--escape=^", "--quote=^", "--records"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": the escape character cannot be the quote character\n").encode(), (args, r.stderr)
    r = _run(flip_bin, "--records", "--escape", "--gpus", "2")
    assert r.returncode == 1 and r.stderr.endswith(b": --records cannot be combined with --gpus\n")
    r = _run(flip_bin, "--records", "--escape", "--phase", "1")
    assert r.returncode == 1 and r.stderr.endswith(b": --records cannot be combined with --phase\n")


def test_usage_mentions_escape(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--escape[=E]" in r.stdout
    assert b"--records[=SEP] --quote[=Q]\"" in r.stdout and b"--records[=SEP]\"" in r.stdout   # (the earlier lines stay)


# ---------------------------------------------------------------------------------------------------------- Python argument checks
def test_python_argument_errors_before_any_device():
    import torch
    m = host.split_escaped_records_model
    for bad, exc in ((b"", ValueError), (b"ab", ValueError), (256, ValueError), ("\\", TypeError), (True, TypeError), (b"\n", ValueError),
                     (10, ValueError), (None, TypeError)):
        with pytest.raises(exc):
            m(b"a\\\n", escape=bad)
    with pytest.raises(ValueError, match="record separator"):
        m(b"a,", sep=b",", escape=b",")
    with pytest.raises(ValueError, match="quote character"):
        m(b"a,", quote=b"^", escape=b"^")
    with pytest.raises(ValueError, match="record separator"):
        m(b"a,", quote=b"\n")
    for bad, exc, quote in ((4, ValueError, b'"'), (-1, ValueError, b'"'), (True, TypeError, b'"'), (None, TypeError, None), (0.0, TypeError, None),
                            (1, ValueError, None), (3, ValueError, None)):
        with pytest.raises(exc):
            m(b"a\\\n", quote=quote, state=bad)
    with pytest.raises(TypeError):
        m("a\\\n")
    v = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        host.split_escaped_records_tensor(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        host.split_escaped_records_tensor(torch.zeros(8, dtype=torch.uint8)[::2])
    with pytest.raises(ValueError, match="record separator"):
        host.split_escaped_records_tensor(v, b"\n", None, b"\n")
    with pytest.raises(ValueError, match="quote character"):
        host.split_escaped_records_tensor(v, b"\n", b'"', b'"')
    with pytest.raises(ValueError, match="state"):
        host.split_escaped_records_tensor(v, state=1)
    with pytest.raises(ValueError, match="state"):
        host.split_escaped_records_tensor(v, quote=b'"', state=4)
    with pytest.raises(host.EngineError, match="HIP device"):
        host.split_escaped_records_tensor(v)
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    with pytest.raises(ValueError, match="record separator"):
        prog.run_records(b"a\n", escape=b"\n")
    with pytest.raises(ValueError, match="quote character"):
        prog.run_records(b"a\n", quote=b'"', escape=b'"')
    with pytest.raises(ValueError, match="escape"):
        prog.run_records(b"a\n", escape=b"")
    with pytest.raises(TypeError, match="escape"):
        prog.run_records(b"a\n", escape="\\")
    with pytest.raises(ValueError, match="record separator"):
        prog.run_records_fd(0, 1, sep=b",", escape=ord(","))
    with pytest.raises(ValueError, match="escape"):
        prog.run_records_fd(0, 1, escape=300)
    with pytest.raises(ValueError, match="quote character"):
        prog.run_records_fd(0, 1, quote=b"'", escape=b"'")
