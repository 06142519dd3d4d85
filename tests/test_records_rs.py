"""CPU: record mode with a multi-byte separator (kx_split_records_rs / kx_run_records_fd_rs, `BIN --records --rs=STR`) — the
offsets model against bytes.split and against itself over every cut of short inputs, the command line's spellings and refusals,
the Python binding's argument checks and the ABI.  Nothing here needs a device."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path

INC = os.path.join(build.ROOT, "include")
SEPS = [b"\r\n", b"\n\n", b"aba", b"abab", b"aaaaaaaa", b"|~|", b"\r\n\r\n"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def _split_offsets(data, rs):
    """The record boundaries bytes.split gives: each piece but the last with its separator; a non-empty last piece is a record."""
    offs, pos = [0], 0
    pieces = data.split(rs)
    for p in pieces[:-1]:
        pos += len(p) + len(rs)
        offs.append(pos)
    if pieces[-1]:
        offs.append(len(data))
    return offs


def _soup(r, rs, n):
    alphabet = bytes(set(rs)) + b"x"
    return bytes(r.choice(alphabet) for _ in range(n))


def test_model_edge_cases():
    m = host.split_rs_records_model
    assert m(b"", b"\r\n") == ([0], b"", 0)
    assert m(b"", b"\r\n", b"\r") == ([0], b"\r", 0)                       # an empty buffer hands its context on
    assert m(b"a\nb\r\nc", b"\r\n") == ([0, 5, 6], b"c", 1)                 # a bare \n ends no record
    assert m(b"ab\r\n", b"\r\n") == ([0, 4], b"", 0)
    assert m(b"ab\r", b"\r\n") == ([0, 3], b"\r", 3)
    assert m(b"\nab", b"\r\n", b"\r") == ([0, 1, 3], b"b", 2)              # the context completes a separator
    assert m(b"\n" * 5, b"\n\n") == ([0, 2, 4, 5], b"\n", 1)                # every second candidate
    assert m(b"\n" * 4, b"\n\n", b"\n") == ([0, 1, 3, 4], b"\n", 1)
    assert m(b"ababab", b"abab") == ([0, 4, 6], b"ab", 2)
    assert m(b"xy", b"aaaaaaaa", b"aaaa") == ([0, 2], b"aaaaxy", 2)         # no separator: the context grows to len(rs) - 1
    assert m(b"wxyz", b"|~|", b"|") == ([0, 4], b"yz", 4)


@pytest.mark.parametrize("rs", SEPS)
def test_model_boundaries_are_those_of_bytes_split(rs):
    r = random.Random(len(rs) * 131 + rs[0])
    for _ in range(1500):
        d = _soup(r, rs, r.randrange(0, 60))
        offs, ctx, tail = host.split_rs_records_model(d, rs)
        assert offs == _split_offsets(d, rs), (d, rs)
        piece = d.split(rs)[-1]                                              # what lies behind the last selected separator
        assert tail == len(piece) and ctx == piece[len(piece) - min(len(rs) - 1, len(piece)):]


@pytest.mark.parametrize("rs", SEPS)
def test_model_chains_over_every_cut(rs):
    """Cutting the input at every position (and at every pair of positions for the shortest inputs, empty and tiny windows
    included) and chaining ctx_out → ctx gives the one-shot boundaries."""
    r = random.Random(len(rs) * 17 + rs[-1])
    for it in range(120):
        d = _soup(r, rs, r.randrange(0, 28))
        want = host.split_rs_records_model(d, rs)[0]
        cuts = [(c,) for c in range(len(d) + 1)]
        if it < 40:
            cuts += [(a, b) for a in range(len(d) + 1) for b in range(a, len(d) + 1)]
        for cut in cuts:
            ends, ctx, pos = [], b"", 0
            edges = [0, *cut, len(d)]
            for lo, hi in zip(edges, edges[1:]):
                offs, ctx2, tail = host.split_rs_records_model(d[lo:hi], rs, ctx)
                complete = offs[1:] if tail == 0 else offs[1:-1]
                ends += [lo + o for o in complete]
                assert len(ctx2) < len(rs) and (d[:hi].endswith(ctx2))
                ctx = ctx2
            if not ends or ends[-1] != len(d):
                if d:
                    ends.append(len(d))
            assert [0] + ends == want, (d, rs, cut)


def test_one_byte_separator_is_the_plain_split():
    r = random.Random(5)
    for _ in range(500):
        d = bytes(r.choice(b"a,\n") for _ in range(r.randrange(0, 50)))
        for sep in (b"\n", b","):
            offs, ctx, tail = host.split_rs_records_model(d, sep)
            assert offs == host.split_records_model(d, sep) and ctx == b""
            assert tail == len(d) - (d.rfind(sep) + 1)


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recrs") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


@pytest.mark.parametrize("arg", ["\\r\\n", "\\n\\n", "|~|", "\\x1e\\n", "abcdefgh", "\\x00\\0\\\\\\t\\r\\n\\xFFz", "x", "\\n"])
def test_good_rs_spellings_reach_the_engine(flip_bin, arg):
    for args in (["--records", "--rs=" + arg], ["--rs", arg, "--records"], ["-t", "--records", "--rs=" + arg]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("arg", ["", "abcdefghi", "\\q", "ab\\", "\\", "\\x4", "\\x", "a\\xg0", "\\n\\n\\n\\n\\n\\n\\n\\n\\n", "\\N"])
def test_bad_rs_is_refused_with_the_exact_message(flip_bin, arg):
    r = _run(flip_bin, "--records", "--rs=" + arg)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr == ("Invalid record separator: %s\n" % arg).encode()


def test_rs_refusals_before_loading(flip_bin):
    for args in (["--rs=\\r\\n"], ["-t", "--rs=ab"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": --rs needs --records\n").encode(), (args, r.stderr)
    for args in (["--records=,", "--rs=\\r\\n"], ["--rs=ab", "--records=\\n"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": --rs cannot be combined with --records=SEP\n").encode(), (args, r.stderr)
    for args in (["--records", "--rs=\\r\\n", "--quote"], ["--records", "--escape", "--rs=ab"], ["--records", "--quote", "--escape=^", "--rs=ab"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": --rs cannot be combined with --quote or --escape\n").encode(), (args, r.stderr)
    r = _run(flip_bin, "--records", "--rs=ab", "--gpus", "2")
    assert r.returncode == 1 and r.stderr.endswith(b": --records cannot be combined with --gpus\n")
    r = _run(flip_bin, "--records", "--rs=ab", "--phase", "1")
    assert r.returncode == 1 and r.stderr.endswith(b": --records cannot be combined with --phase\n")


def test_usage_mentions_rs(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--records --rs=STR\"" in r.stdout
    assert b"--records[=SEP]\"" in r.stdout and b"--escape[=E]\"" in r.stdout   # (the earlier lines stay)


# ---------------------------------------------------------------------------------------------------------- Python argument checks
def test_python_argument_errors_before_any_device():
    import torch
    m = host.split_rs_records_model
    for bad, exc in ((b"", ValueError), (b"123456789", ValueError), ("\r\n", TypeError), (10, TypeError), (None, TypeError)):
        with pytest.raises(exc):
            m(b"a\r\n", bad)
    with pytest.raises(ValueError, match="context"):
        m(b"a", b"\r\n", b"\r\n")
    with pytest.raises(ValueError, match="context"):
        m(b"a", b"\n", b"x")
    with pytest.raises(TypeError):
        m(b"a", b"\r\n", "\r")
    with pytest.raises(TypeError):
        m("a", b"\r\n")
    v = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        host.split_rs_records_tensor(torch.zeros(4, dtype=torch.int32), b"\r\n")
    with pytest.raises(ValueError, match="contiguous"):
        host.split_rs_records_tensor(torch.zeros(8, dtype=torch.uint8)[::2], b"\r\n")
    with pytest.raises(ValueError, match="separator"):
        host.split_rs_records_tensor(v, b"")
    with pytest.raises(ValueError, match="context"):
        host.split_rs_records_tensor(v, b"ab", b"ab")
    with pytest.raises(host.EngineError, match="HIP device"):
        host.split_rs_records_tensor(v, b"\r\n")
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    for call in (lambda **kw: prog.run_records(b"a\r\n", **kw), lambda **kw: prog.run_records_fd(0, 1, **kw)):
        with pytest.raises(ValueError, match="sep"):
            call(rs=b"\r\n", sep=b",")
        with pytest.raises(ValueError, match="quote"):
            call(rs=b"\r\n", quote=b'"')
        with pytest.raises(ValueError, match="escape"):
            call(rs=b"\r\n", escape=b"\\")
        with pytest.raises(ValueError, match="separator"):
            call(rs=b"")
        with pytest.raises(ValueError, match="separator"):
            call(rs=b"123456789")
        with pytest.raises(TypeError, match="separator"):
            call(rs="\r\n")
        with pytest.raises(TypeError, match="separator"):
            call(rs=13)


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_rs_abi_is_declared_and_exported_and_the_structs_keep_their_sizes():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_split_records_rs", "kx_run_records_fd_rs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]
    assert args("kx_split_records_rs") == ["d_in", "n", "rs", "rs_len", "ctx_in", "ctx_in_len", "base", "d_off", "cap", "n_records", "ctx_out",
                                           "ctx_out_len", "tail_len", "stream"]
    assert args("kx_run_records_fd_rs") == ["p", "in_fd", "out_fd", "rs", "rs_len", "report_fd", "stats"]
    assert ctypes.sizeof(host.KxRecordsStats) == 7 * 8 + 3 * 4 + 4 * 4 + 4
    assert ctypes.sizeof(host.KxConfig) == 112


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    f = lib.kx_split_records_rs
    f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64,
                  ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p]
    n = ctypes.c_uint64()
    for rs, rs_len, ctx, ctx_len in ((b"", 0, b"", 0), (b"123456789", 9, b"", 0), (b"\r\n", 2, b"\r\n", 2), (b"\n", 1, b"x", 1),
                                     (b"abc", 3, b"abcd", 4), (None, 2, b"", 0)):
        assert f(None, 0, rs, rs_len, ctx, ctx_len, 0, None, 0, ctypes.byref(n), None, None, None, None) == -4, (rs, rs_len, ctx_len)
    g = lib.kx_run_records_fd_rs
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    assert g(None, 0, 1, b"", 0, -1, None) == -4 and g(None, 0, 1, b"123456789", 9, -1, None) == -4
    assert g(None, 0, 1, b"\r\n", 2, -1, None) == -4     # (a null program, as the other record entry points answer it)
