"""CPU: field mode (`BIN --records … --field=K --fs=F`, kx_run_batch_fields, kx_run_records_fd_fields) — the normative model
field_records_model against independent restatements in every split mode, the command line's refusals on the produced binary,
the Python binding's argument checks and the ABI.  Nothing here needs a device."""
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


def _loop_fields(body, fs, quote=None, escape=None):
    """The fields of a body by a character loop that knows nothing of the model: cut at every live separator."""
    fields, cur, parity, escaped = [], bytearray(), 0, False
    for b in body:
        live = False
        if escaped:
            escaped = False
        elif escape is not None and b == escape:
            escaped = True
        elif quote is not None and b == quote:
            parity ^= 1
        elif b == fs and parity == 0:
            live = True
        if live:
            fields.append(bytes(cur)); cur = bytearray()
        else:
            cur.append(b)
    return fields + [bytes(cur)]


def _want(body, sep, fields, k, fs):
    """What the model must say for field k of a body cut into `fields`."""
    if k > len(fields):
        return len(fields)
    f = bytes([fs])
    return (b"".join(x + f for x in fields[:k - 1]), fields[k - 1], b"".join(f + x for x in fields[k:]), sep)


def _records(r, alphabet, sep, n):
    """n random bodies over the alphabet, each with its separator; the empty body, the lone separator among them."""
    recs = [b"".join(r.choice(alphabet) for _ in range(r.randrange(0, 12))) for _ in range(n)]
    recs[0], recs[1], recs[n // 2] = b"", b"", b""
    data, offs = host.pack_batch([b + sep for b in recs])
    return recs, data, offs


# ---------------------------------------------------------------------------------------------------------- the model
def test_model_edge_cases():
    m = host.field_records_model
    assert m(b"", [0], 1, False, 1, b"\t") == []
    assert m(b"\n", [0, 1], 1, False, 1, b",") == [(b"", b"", b"", b"\n")]          # the lone separator: one empty field
    assert m(b"\n", [0, 1], 1, False, 2, b",") == [1]
    assert m(b"", [0, 0], 0, False, 1, b",") == [(b"", b"", b"", b"")]              # the empty body
    assert m(b"a,b,c\nx", [0, 6, 7], 1, True, 2, b",") == [(b"a,", b"b", b",c", b"\n"), 1]   # the tail has no separator
    assert m(b"a,b,c\nx\n", [0, 6, 8], 1, True, 1, b",")[1] == (b"", b"x\n", b"", b"")      # last_whole: its last byte is body
    assert m(b",,\r\n", [0, 4], 2, False, 3, b",") == [(b",,", b"", b"", b"\r\n")]  # empty fields, the last one too
    assert m(b",,\r\n", [0, 4], 2, False, 4, b",") == [3]
    assert m(b'a,"b,c",d\n', [0, 10], 1, False, 2, b",", quote=b'"') == [(b"a,", b'"b,c"', b",d", b"\n")]   # quotes stay in the field
    assert m(b'a,"b""c,",d\n', [0, 12], 1, False, 3, b",", quote=b'"') == [(b'a,"b""c,",', b"d", b"", b"\n")]
    assert m(b"a\\,b,c\n", [0, 7], 1, False, 1, b",", escape=b"\\") == [(b"", b"a\\,b", b",c", b"\n")]
    assert m(b"a\\\\,b\n", [0, 6], 1, False, 2, b",", escape=b"\\") == [(b"a\\\\,", b"b", b"", b"\n")]      # an escaped escape
    assert m(b'a\\",b",c\n', [0, 9], 1, False, 2, b",", quote=b'"', escape=b"\\") == [(b'a\\",', b'b",c', b"", b"\n")]
    assert m(b"xxa,b\nyy", [2, 6], 1, False, 2, b",") == [(b"a,", b"b", b"", b"\n")]  # offsets[0] need not be 0


@pytest.mark.parametrize("sep", [b"\n", b"\r\n", b"|~|"])
def test_model_is_bytes_split(sep):
    """BYTE and RS mode: the fields are body.split(fs)."""
    r = random.Random(len(sep))
    alphabet = [b"a", b"\t", b"\t", sep[:1], b'"', b"\\"]                             # (the model takes the ranges as given: a separator byte may be in a body)
    recs, data, offs = _records(r, alphabet, sep, 2000)
    for tail in (b"", b"a\tb", b"\t"):
        d, o = data + tail, offs + ([len(data) + len(tail)] if tail else [])
        bodies = recs + ([tail] if tail else [])
        for k in range(1, 9):
            got = host.field_records_model(d, o, len(sep), bool(tail), k, b"\t")
            assert len(got) == len(bodies)
            for i, (body, g) in enumerate(zip(bodies, got)):
                fields = body.split(b"\t")
                assert g == _want(body, b"" if tail and i == len(recs) else sep, fields, k, 9), (body, k, g)
    for body in set(recs):                                                           # every K from 1 to fields + 2
        n = len(body.split(b"\t"))
        for k in range(1, n + 3):
            g = host.field_records_model(body + sep, [0, len(body) + len(sep)], len(sep), False, k, b"\t")[0]
            assert (g == n) if k > n else (g[1] == body.split(b"\t")[k - 1] and b"".join(g) == body + sep)


@pytest.mark.parametrize("quote,escape", [(b'"', None), (None, b"\\"), (b'"', b"\\")])
def test_model_quoted_and_escaped_against_the_loop(quote, escape):
    r = random.Random(7 + (quote is not None) + 2 * (escape is not None))
    alphabet = [b"a", b",", b",", b"\n"] + ([quote] if quote else []) + ([escape] if escape else [])
    # (the separator byte inside a body: quoted or escaped in a real stream; the model takes the ranges as given)
    recs, data, offs = _records(r, alphabet, b"\n", 2000)
    q, e = quote and quote[0], escape and escape[0]
    seen = set()
    for tail in (b"", b'a,"b'):
        d, o = data + tail, offs + ([len(data) + len(tail)] if tail else [])
        bodies = recs + ([tail] if tail else [])
        for k in range(1, 8):
            got = host.field_records_model(d, o, 1, bool(tail), k, b",", quote=quote, escape=escape)
            for i, (body, g) in enumerate(zip(bodies, got)):
                fields = _loop_fields(body, 0x2C, q, e)
                assert g == _want(body, b"" if tail and i == len(recs) else b"\n", fields, k, 0x2C), (body, k, g)
                seen.add(len(fields) != len(body.split(b",")))
    assert seen == {False, True}                                                    # some separators were not live
    for body in list(set(recs))[:300]:
        n = len(_loop_fields(body, 0x2C, q, e))
        for k in range(1, n + 3):
            g = host.field_records_model(body, [0, len(body)], 0, False, k, b",", quote=quote, escape=escape)[0]
            assert (g == n) if k > n else b"".join(g) == body


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recfield") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


@pytest.mark.parametrize("args", [["--records", "--field=1"], ["--records", "--field", "3", "--fs=,"], ["--field=4294967295", "--records=\\0", "--fs=\\n"],
                                  ["--records", "--rs=\\r\\n", "--field=2", "--fs=\\r", "--chomp", "--ors=\\n"],
                                  ["--records", "--quote", "--field=2", "--fs=,"], ["--records", "--escape", "--quote", "--fs=\\x3b", "--field=7"]])
def test_good_options_reach_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("args,names", [
    (["--field=2"], b"--field"), (["--field=2", "--fs=,"], b"--field"), (["-t", "--field=1"], b"--field"),   # --field without --records
    (["--records", "--fs=,"], b"--fs"), (["--fs=,"], b"--fs"),                                                     # --fs without --field
    (["--records", "--field=0"], b"--field"), (["--records", "--field=x"], b"--field"), (["--records", "--field=1x"], b"--field"),
    (["--records", "--field=-1"], b"--field"), (["--records", "--field=4294967296"], b"--field"), (["--records", "--field="], b"--field"),
    (["--records", "--field=1", "--fs=ab"], b"--fs"), (["--records", "--field=1", "--fs="], b"--fs"),
    (["--records", "--field=1", "--fs=\\n"], b"--fs"), (["--records=,", "--field=1", "--fs=,"], b"--fs"),         # F = SEP
    (["--records", "--rs=,", "--field=1", "--fs=,"], b"--fs"), (["--records", "--rs=\\t", "--field=1"], b"--fs"),                # F = a one-byte --rs
    (["--records", "--quote", "--field=1", "--fs=\""], b"--fs"), (["--records", "--quote=,", "--field=1", "--fs=,"], b"--fs"),   # F = Q
    (["--records", "--escape", "--field=1", "--fs=\\\\"], b"--fs"), (["--records", "--quote", "--escape=;", "--field=1", "--fs=;"], b"--fs")])   # F = E
def test_refusals_before_loading(flip_bin, args, names):
    r = _run(flip_bin, *args)
    assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
    assert names in r.stderr and b"cannot load" not in r.stderr, (args, r.stderr)


def test_usage_mentions_the_option(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--field=K [--fs=F]\"" in r.stdout and b"--ors=STR\"" in r.stdout


# ---------------------------------------------------------------------------------------------------------- Python argument checks
def test_python_argument_errors_before_any_device():
    import torch
    m = host.field_records_model
    with pytest.raises(TypeError, match="bytes"):
        m("a\n", [0, 2], 1, False, 1, b",")
    for bad, exc in ((0, ValueError), (1 << 32, ValueError), (True, TypeError), (1.0, TypeError), (b"1", TypeError)):
        with pytest.raises(exc, match="field"):
            m(b"a\n", [0, 2], 1, False, bad, b",")
    for bad, exc in ((b"ab", ValueError), (b"", ValueError), (256, ValueError), (",", TypeError), (None, TypeError)):
        with pytest.raises(exc, match="field separator"):
            m(b"a\n", [0, 2], 1, False, 1, bad)
    with pytest.raises(ValueError, match="quote"):
        m(b"a\n", [0, 2], 1, False, 1, b",", quote=b",")
    with pytest.raises(ValueError, match="escape"):
        m(b"a\n", [0, 2], 1, False, 1, b",", escape=b",")
    with pytest.raises(ValueError, match="sep_len"):
        m(b"a\n", [0, 2], 9, False, 1, b",")
    with pytest.raises(ValueError, match="shorter"):
        m(b"a\n\n", [0, 2, 3], 2, False, 1, b",")
    with pytest.raises(TypeError, match="last_whole"):
        m(b"a\n", [0, 2], 1, 0, 1, b",")
    with pytest.raises(ValueError, match="offsets"):
        m(b"a\n", [0, 3], 1, False, 1, b",")
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    v, o = torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 2, 4])
    for kw, exc, what in (({"field": 0}, ValueError, "field"), ({"field": "1"}, TypeError, "field"), ({"field": 1, "fs": b"ab"}, ValueError, "field separator"),
                          ({"field": 1, "fs": b",", "quote": b","}, ValueError, "quote"), ({"field": 1, "fs": b",", "escape": b","}, ValueError, "escape"),
                          ({"field": 1, "quote": b'"', "escape": b'"'}, ValueError, "escape"), ({"field": 1, "sep_len": 9}, ValueError, "sep_len"),
                          ({"field": 1, "last_whole": 1}, TypeError, "last_whole"), ({"field": 1, "keep_sep": 1}, TypeError, "keep_sep"),
                          ({"field": 1, "suffix": b"123456789"}, ValueError, "suffix"), ({"field": 1, "suffix": "\n"}, TypeError, "suffix")):
        with pytest.raises(exc, match=what):
            prog.run_batch_fields_tensor(v, o, **kw)
    with pytest.raises(host.EngineError, match="HIP device"):
        prog.run_batch_fields_tensor(v, o, 1)
    for call in (lambda **kw: prog.run_records(b"a\tb\n", **kw), lambda **kw: prog.run_records_fd(0, 1, **kw)):
        with pytest.raises(ValueError, match="field"):
            call(field=0)
        with pytest.raises(TypeError, match="field"):
            call(field="2")
        with pytest.raises(ValueError, match="record separator"):
            call(field=1, fs=b"\n")
        with pytest.raises(ValueError, match="record separator"):
            call(field=1, fs=b",", rs=b",")                                        # (a one-byte rs is a one-byte separator)
        with pytest.raises(ValueError, match="quote"):
            call(field=1, fs=b'"', quote=b'"')
        with pytest.raises(ValueError, match="escape"):
            call(field=1, fs=b"\\", escape=b"\\")
        with pytest.raises(ValueError, match="field separator"):
            call(field=1, fs=b"ab")
    e = host.NoFieldError(3)
    assert isinstance(e, host.KleenexError) and e.fields == 3


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_abi_is_declared_and_exported():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_run_batch_fields", "kx_run_records_fd_fields", "kx_fields_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]
    batch = ["prog", "d_in", "d_in_off", "n_docs", "d_out", "cap", "d_out_off", "d_docs", "out_len", "stats", "stream"]
    assert args("kx_run_batch") == batch
    assert args("kx_run_batch_fields") == batch[:4] + ["fields"] + batch[4:]
    assert args("kx_run_records_fd_fields") == ["p", "in_fd", "out_fd", "o", "field", "fs", "report_fd", "stats"]
    spec = re.search(r"typedef struct kx_batch_fields \{(.*?)\} kx_batch_fields;", txt, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", spec) == [f for f, _ in host.KxBatchFields._fields_]
    assert ctypes.sizeof(host.KxBatchFields) == 12 + 8 + 16 + 8 + 16 == 60
    # the structs that field mode leaves alone
    assert ctypes.sizeof(host.KxBatchFrame) == 3 * 4 + 8 + 3 * 4 and ctypes.sizeof(host.KxRecordsOpts) == 64
    assert ctypes.sizeof(host.KxBatchStats) == 5 * 8 + 6 * 4 + 8 + 4 + 4 and ctypes.sizeof(host.KxRecordsStats) == 7 * 8 + 3 * 4 + 4 * 4 + 4


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    lib.kx_last_error.restype = ctypes.c_char_p
    f = lib.kx_run_batch_fields
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.POINTER(host.KxBatchFields), ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 5
    size = ctypes.sizeof(host.KxBatchFields)
    good = dict(size=size, field=2, fs=9, quote=-1, escape=-1, sep_len=1, keep_sep=1)
    ol = ctypes.c_size_t()
    tail = (None, 0, None, None, ctypes.cast(ctypes.byref(ol), ctypes.c_void_p), None, None)
    assert f(None, None, None, 0, ctypes.byref(host.KxBatchFields(**good)), *tail) == -4        # a null program
    assert f(None, None, None, 0, None, *tail) == -4
    # (a program handle that is no program: a call that got past the checks would read it and crash, not return -4)
    fake = ctypes.c_void_p(16)
    assert f(fake, None, None, 0, None, *tail) == -4                                             # a null spec
    bad = [dict(good, size=size - 4), dict(good, size=0), dict(good, field=0), dict(good, quote=9), dict(good, escape=9),
           dict(good, quote=34, escape=34), dict(good, quote=256), dict(good, escape=-2), dict(good, sep_len=9), dict(good, suffix_len=9)]
    for kw in bad:
        assert f(fake, None, None, 0, ctypes.byref(host.KxBatchFields(**kw)), *tail) == -4, kw
        assert b"kx_run_batch_fields" in lib.kx_last_error()
    for k in range(4):
        o = host.KxBatchFields(**good)
        o.reserved[k] = 1
        assert f(fake, None, None, 0, ctypes.byref(o), *tail) == -4 and b"reserved" in lib.kx_last_error()
    o = host.KxBatchFields(**good)
    o.pad[1] = 1
    assert f(fake, None, None, 0, ctypes.byref(o), *tail) == -4 and b"reserved" in lib.kx_last_error()
    g = lib.kx_run_records_fd_fields
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(host.KxRecordsOpts), ctypes.c_uint32, ctypes.c_uint8, ctypes.c_int,
                  ctypes.c_void_p]
    osz = ctypes.sizeof(host.KxRecordsOpts)
    ro = dict(size=osz, mode=host.KX_RECORDS_BYTE, sep=10, quote=-1, escape=-1)
    assert g(None, 0, 1, None, 1, 9, -1, None) == -4
    assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**ro)), 0, 9, -1, None) == -4 and b"field" in lib.kx_last_error()
    for kw, fs in ((ro, 10), (dict(ro, mode=host.KX_RECORDS_QUOTED, quote=34), 34), (dict(ro, mode=host.KX_RECORDS_ESCAPED, quote=34, escape=92), 92),
                   (dict(ro, mode=host.KX_RECORDS_ESCAPED, quote=34, escape=92), 34), (dict(ro, size=osz - 4), 9), (dict(ro, chomp=2), 9)):
        assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**kw)), 1, fs, -1, None) == -4, (kw, fs)
    rs1 = host.KxRecordsOpts(**dict(ro, mode=host.KX_RECORDS_RS, rs_len=1))
    rs1.rs[0] = 44
    assert g(None, 0, 1, ctypes.byref(rs1), 1, 44, -1, None) == -4 and b"record separator" in lib.kx_last_error()   # a one-byte rs equal to fs
    rs = host.KxRecordsOpts(**dict(ro, mode=host.KX_RECORDS_RS, rs_len=2))
    rs.rs[:2] = b"\r\n"
    assert g(None, 0, 1, ctypes.byref(rs), 1, 13, -1, None) == -4 and b"null argument" in lib.kx_last_error()   # (a byte of rs may be fs: refused only for the null program)
    assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**ro)), 1, 9, -1, None) == -4 and b"null argument" in lib.kx_last_error()
