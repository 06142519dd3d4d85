"""CPU: record mode's framing options (`BIN --records … --chomp --ors=STR`, kx_run_batch_framed, kx_run_records_fd_opts) — the
normative model chomp_records_model against a plain Python loop in every split mode, the command line's refusals and messages
on the produced binary, the Python binding's argument checks and the ABI.  Nothing here needs a device."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path

INC = os.path.join(build.ROOT, "include")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def _loop_docs(data, sep, quote=None, escape=None):
    """The chomped records by a byte-at-a-time loop: a separator byte that is unescaped and outside quotes ends a record and is
    dropped; every other byte is data; what is left behind the last separator is the tail, whole."""
    docs, cur, parity, escaped = [], bytearray(), 0, False
    for b in data:
        if escaped:
            escaped = False
        elif escape is not None and b == escape:
            escaped = True
        elif quote is not None and b == quote:
            parity ^= 1
        elif b == sep and parity == 0:
            docs.append(bytes(cur))
            cur = bytearray()
            continue
        cur.append(b)
    if cur:
        docs.append(bytes(cur))
    return docs


def _tail(model_offsets, data):
    """The last record has no valid separator: appending a byte does not leave a boundary at len(data)."""
    return bool(data) and len(data) not in model_offsets(data + b"x")[:-1]


def _soup(r, alphabet, n):
    return bytes(r.choice(alphabet) for _ in range(n))


# ---------------------------------------------------------------------------------------------------------- the model
def test_model_edge_cases():
    m = host.chomp_records_model
    assert m(b"", [0], 1, False) == []
    assert m(b"a,b\n\nxy", [0, 4, 5, 7], 1, True) == [b"a,b", b"", b"xy"]          # a record that is only its separator: empty, not skipped
    assert m(b"a,b\n\nxy\n", [0, 4, 5, 8], 1, False) == [b"a,b", b"", b"xy"]
    assert m(b"a\r\n\r\nb\r", [0, 3, 5, 7], 2, True) == [b"a", b"", b"b\r"]       # half a separator at the end is data
    assert m(b'a\n"b\n', [0, 2, 5], 1, True) == [b"a", b'"b\n']                   # the tail ends in a quoted separator byte: it stays
    assert m(b"a\nb\\\n", [0, 2, 5], 1, True) == [b"a", b"b\\\n"]                 # … or in an escaped one
    assert m(b"xxab\ncd\nyy", [2, 5, 8], 1, False) == [b"ab", b"cd"]              # offsets[0] need not be 0
    assert m(b"ab\ncd\n", [0, 3, 6], 0, False) == [b"ab\n", b"cd\n"]              # trim 0: the records themselves
    with pytest.raises(ValueError, match="shorter"):
        m(b"a\r\n\n", [0, 3, 4], 2, False)
    assert m(b"a\r\n\n", [0, 3, 4], 2, True) == [b"a", b"\n"]                     # (the short last range is a tail: whole)


@pytest.mark.parametrize("rs", [b"\n", b"\0", b",", b"\r\n", b"\n\n", b"|~|", b"abab", b"aaaaaaaa"])
def test_model_is_bytes_split(rs):
    r = random.Random(len(rs) * 7 + rs[0])
    for _ in range(1500):
        d = _soup(r, bytes(set(rs)) + b"xy", r.randrange(0, 50))
        offs, _, tail_len = host.split_rs_records_model(d, rs)
        pieces = d.split(rs)
        want = pieces[:-1] + ([pieces[-1]] if pieces[-1] else [])
        assert host.chomp_records_model(d, offs, len(rs), tail_len > 0) == want, (d, rs)
        if len(rs) == 1:
            offs1 = host.split_records_model(d, rs)
            assert host.chomp_records_model(d, offs1, 1, not d.endswith(rs) and bool(d)) == want, (d, rs)


def test_model_quoted_against_the_loop():
    r = random.Random(11)
    mo = lambda d: host.split_records_model(d, b"\n", b'"')   # noqa: E731
    seen_quoted_tail = 0
    for _ in range(3000):
        d = _soup(r, b'a"\n\n,', r.randrange(0, 40))
        tail = _tail(mo, d)
        seen_quoted_tail += tail and d.endswith(b"\n")
        assert host.chomp_records_model(d, mo(d), 1, tail) == _loop_docs(d, 0x0A, quote=0x22), d
    assert seen_quoted_tail > 50                                                   # tails that end in a quoted separator byte


@pytest.mark.parametrize("quote", [None, b'"'])
def test_model_escaped_against_the_loop(quote):
    r = random.Random(13 if quote else 12)
    mo = lambda d: host.split_escaped_records_model(d, b"\n", quote, b"\\")[0]   # noqa: E731
    seen_escaped_tail = 0
    for _ in range(3000):
        d = _soup(r, b'a\\\\\n\n"' if quote else b"a\\\\\n\n", r.randrange(0, 40))
        tail = _tail(mo, d)
        seen_escaped_tail += tail and d.endswith(b"\n")
        assert host.chomp_records_model(d, mo(d), 1, tail) == _loop_docs(d, 0x0A, quote=quote and quote[0], escape=0x5C), d
    assert seen_escaped_tail > 50


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recchomp") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


@pytest.mark.parametrize("args", [["--records", "--chomp"], ["--chomp", "--records=\\0", "--ors=\\n"], ["--records", "--ors="],
                                  ["--records", "--ors", ""], ["--records", "--rs=\\r\\n", "--chomp", "--ors=\\n"],
                                  ["--records", "--quote", "--chomp", "--ors=\\r\\n"], ["--records", "--escape", "--quote", "--ors=12345678"],
                                  ["-t", "--records", "--ors=\\x00\\0\\\\\\t\\r\\n\\xFFz", "--chomp"]])
def test_good_options_reach_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("arg", ["abcdefghi", "\\q", "ab\\", "\\", "\\x4", "\\x", "a\\xg0", "\\n\\n\\n\\n\\n\\n\\n\\n\\n", "\\N"])
def test_bad_ors_is_refused_with_the_exact_message(flip_bin, arg):
    for args in (["--records", "--ors=" + arg], ["--ors=" + arg]):                 # (parsed before --records is missed)
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr == ("Invalid output record separator: %s\n" % arg).encode()


def test_refusals_before_loading(flip_bin):
    for args in (["--chomp"], ["-t", "--chomp"], ["--chomp", "--ors=\\n"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": --chomp needs --records\n").encode(), (args, r.stderr)
    for args in (["--ors=\\n"], ["--ors="], ["-t", "--ors", "ab"]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and r.stderr == (flip_bin + ": --ors needs --records\n").encode(), (args, r.stderr)
    r = _run(flip_bin, "--records", "--chomp", "--gpus", "2")
    assert r.returncode == 1 and r.stderr.endswith(b": --records cannot be combined with --gpus\n")
    r = _run(flip_bin, "--records", "--ors=x", "--phase", "1")
    assert r.returncode == 1 and r.stderr.endswith(b": --records cannot be combined with --phase\n")


def test_usage_mentions_the_options(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--chomp\"" in r.stdout and b"--ors=STR\"" in r.stdout
    assert b"--records --rs=STR\"" in r.stdout and b"--records[=SEP]\"" in r.stdout   # (the earlier lines stay)


# ---------------------------------------------------------------------------------------------------------- Python argument checks
def test_python_argument_errors_before_any_device():
    import torch
    m = host.chomp_records_model
    with pytest.raises(TypeError, match="bytes"):
        m("a\n", [0, 2], 1, False)
    for bad, exc in ((-1, ValueError), (1 << 32, ValueError), (True, TypeError), (1.0, TypeError), (b"\n", TypeError)):
        with pytest.raises(exc, match="trim"):
            m(b"a\n", [0, 2], bad, False)
    with pytest.raises(TypeError, match="tail"):
        m(b"a\n", [0, 2], 1, 0)
    with pytest.raises(ValueError, match="offsets"):
        m(b"a\n", [0, 3], 1, False)
    with pytest.raises(ValueError, match="offsets"):
        m(b"a\nb\n", [0, 4, 2], 1, False)
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    v, o = torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 2, 4])
    for kw, exc, what in (({"trim": -1}, ValueError, "trim"), ({"trim": "1"}, TypeError, "trim"), ({"trim": True}, TypeError, "trim"),
                          ({"last_whole": 1}, TypeError, "last_whole"), ({"suffix": "\n"}, TypeError, "suffix"),
                          ({"suffix": b"123456789"}, ValueError, "suffix"), ({"suffix": 10}, TypeError, "suffix")):
        with pytest.raises(exc, match=what):
            prog.run_batch_tensor(v, o, **kw)
    with pytest.raises(host.EngineError, match="HIP device"):
        prog.run_batch_tensor(v, o, trim=1, suffix=b"\n")
    for call in (lambda **kw: prog.run_records(b"a\r\n", **kw), lambda **kw: prog.run_records_fd(0, 1, **kw)):
        with pytest.raises(ValueError, match="output record separator"):
            call(ors=b"123456789")
        with pytest.raises(TypeError, match="output record separator"):
            call(ors="\n")
        with pytest.raises(TypeError, match="output record separator"):
            call(ors=10)
        with pytest.raises(TypeError, match="output record separator"):
            call(ors=None)
        with pytest.raises(TypeError, match="chomp"):
            call(chomp=1)
        with pytest.raises(TypeError, match="chomp"):
            call(chomp=None)
        with pytest.raises(ValueError, match="sep"):
            call(rs=b"\r\n", sep=b",", chomp=True)                                 # (the earlier checks stay in front)


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_abi_is_declared_and_exported_and_the_structs_keep_their_sizes():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_run_batch_framed", "kx_run_records_fd_opts", "kx_run_batch", "kx_run_records_fd", "kx_run_records_fd_quoted",
                 "kx_run_records_fd_escaped", "kx_run_records_fd_rs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]
    batch = ["prog", "d_in", "d_in_off", "n_docs", "d_out", "cap", "d_out_off", "d_docs", "out_len", "stats", "stream"]
    assert args("kx_run_batch") == batch                                           # (unchanged)
    assert args("kx_run_batch_framed") == batch[:4] + ["frame"] + batch[4:]
    assert args("kx_run_records_fd_opts") == ["p", "in_fd", "out_fd", "o", "report_fd", "stats"]
    assert args("kx_run_records_fd") == ["p", "in_fd", "out_fd", "sep", "report_fd", "stats"]
    assert args("kx_run_records_fd_rs") == ["p", "in_fd", "out_fd", "rs", "rs_len", "report_fd", "stats"]
    # the existing structs: sizes as the earlier tests pin them
    assert ctypes.sizeof(host.KxRecordsStats) == 7 * 8 + 3 * 4 + 4 * 4 + 4
    assert ctypes.sizeof(host.KxConfig) == 112
    assert ctypes.sizeof(host.KxBatchStats) == 5 * 8 + 6 * 4 + 8 + 4 + 4
    assert ctypes.sizeof(host.KxBatchDoc) == 16
    # the new ones, field by field as the header declares them
    frame = re.search(r"typedef struct kx_batch_frame \{(.*?)\} kx_batch_frame;", txt, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", frame) == [f for f, _ in host.KxBatchFrame._fields_]
    assert ctypes.sizeof(host.KxBatchFrame) == 3 * 4 + 8 + 3 * 4
    opts = re.search(r"typedef struct kx_records_opts \{(.*?)\} kx_records_opts;", txt, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", opts) == [f for f, _ in host.KxRecordsOpts._fields_]
    assert ctypes.sizeof(host.KxRecordsOpts) == 64 and host.KxRecordsOpts.ors_len.offset == 44


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    g = lib.kx_run_records_fd_opts
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(host.KxRecordsOpts), ctypes.c_int, ctypes.c_void_p]
    size = ctypes.sizeof(host.KxRecordsOpts)
    assert g(None, 0, 1, None, -1, None) == -4
    good = dict(size=size, mode=host.KX_RECORDS_BYTE, sep=10, quote=-1, escape=-1, chomp=1, ors_len=1)
    bad = [dict(good, size=size - 4), dict(good, size=0), dict(good, mode=4), dict(good, ors_len=9), dict(good, chomp=2),
           dict(good, mode=host.KX_RECORDS_QUOTED, quote=10), dict(good, mode=host.KX_RECORDS_QUOTED, quote=-1),
           dict(good, mode=host.KX_RECORDS_ESCAPED, escape=10), dict(good, mode=host.KX_RECORDS_ESCAPED, escape=-1),
           dict(good, mode=host.KX_RECORDS_ESCAPED, quote=92, escape=92), dict(good, mode=host.KX_RECORDS_ESCAPED, quote=256, escape=92),
           dict(good, mode=host.KX_RECORDS_RS, rs_len=0), dict(good, mode=host.KX_RECORDS_RS, rs_len=9)]
    for kw in bad:
        assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**kw)), -1, None) == -4, kw
    o = host.KxRecordsOpts(**good)
    o.reserved[2] = 1
    assert g(None, 0, 1, ctypes.byref(o), -1, None) == -4
    lib.kx_last_error.restype = ctypes.c_char_p
    assert b"reserved" in lib.kx_last_error()
    assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**good)), -1, None) == -4    # (a null program, as the other record entry points answer it)
    f = lib.kx_run_batch_framed
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.POINTER(host.KxBatchFrame), ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 5
    assert f(None, None, None, 0, None, None, 0, None, None, None, None, None) == -4
