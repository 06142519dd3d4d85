"""CPU: field mode on unquoted values (`BIN --records … --quote|--escape --field=K|LIST --unquote`, kx_run_batch_field_values,
kx_run_records_fd_field_values) — the two normative models host.unquote_field_model and host.requote_field_model by hand, against
Python's csv.writer and against each other, the command line's refusals on the produced binary, the C entry point's refusals
and the Python binding's argument checks.  Nothing here needs a device."""
import csv
import ctypes
import io
import os
import random
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path

U, R = host.unquote_field_model, host.requote_field_model
Q, E = b'"', b"\\"
MODES = [dict(quote=Q), dict(quote=Q, escape=E), dict(escape=E)]


# ---------------------------------------------------------------------------------------------------------- the two models by hand
@pytest.mark.parametrize("raw,value", [(b'""', b""), (b'""""', b'"'), (b'"a""b"', b'a"b'), (b'ab"c,d"e', b"abc,de"), (b'"abc', b"abc"),
                                       (b"", b""), (b"abc", b"abc"), (b'"a,b"', b"a,b"), (b'"a"b"c"', b"abc"), (b'"a" "b"', b"a b"),
                                       (b'""""""', b'""'), (b'a""b', b"ab")])
def test_value_by_hand_quote(raw, value):
    assert U(raw, quote=Q) == value
    if b"\\" not in raw:
        assert U(raw, quote=Q, escape=E) == value                                       # no escape byte in it: the escape changes nothing


@pytest.mark.parametrize("raw,value", [(b"\\", b""), (b"\\\\", b"\\"), (b"a\\,b", b"a,b"), (b"a\\", b"a"), (b'\\"', b'"'), (b"\\\\\\", b"\\"),
                                       (b"\\a\\b", b"ab"), (b"\\\n", b"\n")])
def test_value_by_hand_escape(raw, value):
    assert U(raw, escape=E) == value
    assert U(raw, quote=Q, escape=E) == value


def test_value_by_hand_both():
    assert U(b'"a\\"b"', quote=Q, escape=E) == b'a"b'
    assert U(b'"a"\\""b"', quote=Q, escape=E) == b'a"b'                                 # the escaped quote sits between a closing and an opening one: no third
    assert U(b'"a""b"', quote=Q, escape=E) == b'a"b'
    assert U(b'"a\\', quote=Q, escape=E) == b"a"                                        # an unclosed quote and a last escape alone: both dropped
    assert U(b'a"b', escape=E) == b'a"b'                                                # without a quote byte a quote is data
    assert U(b"a'b''c'", quote=b"'") == b"ab'c"                                         # any byte can be the quote


def test_spelling_by_hand():
    q = dict(fs=b",", quote=Q)
    assert R(b"abc", False, **q) == b"abc" and R(b"abc", True, **q) == b'"abc"'         # both was_quoted values
    assert R(b"", False, **q) == b"" and R(b"", True, **q) == b'""'                     # an empty output of a quoted field
    assert R(b"a,b", False, **q) == b'"a,b"' and R(b'a"b', False, **q) == b'"a""b"' and R(b"a\nb", False, **q) == b'"a\nb"'
    assert R(b'"', False, **q) == b'""""' and R(b'"', True, **q) == b'""""'
    assert R(b"a\nb", False, special=b"", **q) == b"a\nb" and R(b"a;b", False, special=b";|", **q) == b'"a;b"'
    assert R(b"a\\b", False, **q) == b"a\\b"                                            # no escape byte set: a backslash is data
    qe = dict(fs=b",", quote=Q, escape=E)
    assert R(b"abc", False, **qe) == b"abc" and R(b"abc", True, **qe) == b'"abc"' and R(b"", True, **qe) == b'""'
    assert R(b'a"b', False, **qe) == b'a\\"b' and R(b'a"b', True, **qe) == b'"a\\"b"'   # a quote alone does not wrap here
    assert R(b"a\\b", False, **qe) == b"a\\\\b" and R(b"a,b", False, **qe) == b'"a,b"' and R(b"a\nb", False, **qe) == b'"a\nb"'
    e = dict(fs=b",", escape=E)
    assert R(b"abc", False, **e) == b"abc" and R(b"", False, **e) == b""
    assert R(b'a,b\nc\\d"e', False, **e) == b'a\\,b\\\nc\\\\d"e'
    assert R(b"a;b", False, special=b";", **e) == b"a\\;b"


# ---------------------------------------------------------------------------------------------------------- against csv.writer
def _rows(r, n, alphabet):
    """n rows of 2 to 4 fields of 0 to 6 characters; one field in 200 keeps a leading space, the others lose theirs."""
    field = lambda: "".join(r.choice(alphabet) for _ in range(r.randrange(0, 7)))   # noqa: E731
    return [[f if r.randrange(200) == 0 else f.lstrip(" ") for f in (field() for _ in range(r.randrange(2, 5)))] for _ in range(n)]


@pytest.mark.parametrize("dialect", ["default", "all", "escape"])
def test_models_against_csv_writer(dialect):
    """Rows of 2 to 4 fields over ab,"\\ LF CR space x (a z for the backslash where the writer has no escape character), written by
    csv.writer with the record separator as its line terminator.  The liveness rule finds the writer's fields, the decoded value
    is the written string, and the spelling of that value is the written field byte for byte.  Only rows with a field that begins
    with a space are left out (skipinitialspace is not modelled: a leading space is data here)."""
    r = random.Random({"default": 1, "all": 2, "escape": 3}[dialect])
    esc = dialect == "escape"
    alphabet = 'ab,"\n\r x' + ("\\" if esc else "z")
    kw = dict(lineterminator="\n")
    if dialect == "all":
        kw["quoting"] = csv.QUOTE_ALL
    if esc:
        kw.update(escapechar="\\", doublequote=False)
    m = dict(quote=Q, escape=E) if esc else dict(quote=Q)
    rows = _rows(r, 3000, alphabet)
    checked, quoted = 0, 0
    for row in rows:
        if any(f.startswith(" ") for f in row):
            continue
        buf = io.StringIO(newline="")
        csv.writer(buf, **kw).writerow(row)
        line = buf.getvalue().encode()
        (rec,) =[x for x in host.field_list_records_model(line, host.split_escaped_records_model(line, b"\n", Q, E)[0] if esc
                                                           else host.split_records_model(line, b"\n", Q), 1, False, [(1, None)], b",", **m)]
        gaps, fields, sep = rec
        assert sep == b"\n" and len(fields) == len(row), (row, line)
        for (_, raw), want in zip(fields, row):
            assert U(raw, **m) == want.encode(), (row, raw)
            was_quoted = raw[:1] == Q
            assert R(want.encode(), was_quoted, b",", special=b"\n", **m) == raw, (row, raw, was_quoted)
            quoted += was_quoted
        checked += 1
    assert 0.95 * len(rows) <= checked < len(rows) and quoted > checked // 2           # at least 95 % of the rows, many quoted fields


# ---------------------------------------------------------------------------------------------------------- round trip, liveness
@pytest.mark.parametrize("m", MODES)
def test_round_trip_and_one_field(m):
    r = random.Random(5 + len(m))
    alphabet = b'ab,"\\\n\r x'
    for _ in range(4000):
        v = bytes(r.choice(alphabet) for _ in range(r.randrange(0, 9)))
        for was_quoted in (False, True):
            if was_quoted and "quote" not in m:
                continue                                                                # (no quote byte: no field was quoted)
            s = R(v, was_quoted, b",", special=b"\n", **m)
            assert U(s, **m) == v, (v, was_quoted, s)
            (rec,) = host.field_list_records_model(s, [0, len(s)], 0, False, [(1, None)], b",", **m)
            assert rec == ([b"", b""], [(1, s)], b""), (v, s, rec)                       # one field: no live separator in the spelling
            offs = host.split_escaped_records_model(s + b"\n", b"\n", m.get("quote"), E)[0] if "escape" in m else host.split_records_model(s + b"\n", b"\n", Q)
            assert list(offs) == [0, len(s) + 1], (v, s, offs)                           # … and no live record separator


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recunquote") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


@pytest.mark.parametrize("args", [["--records", "--quote", "--unquote"], ["--records", "--escape", "--chomp", "--unquote"], ["--unquote"],
                                  ["--records", "--field=2", "--unquote"], ["--records", "--field=2,4-", "--fs=,", "--unquote"],
                                  ["--records=;", "--chomp", "--field=1-", "--unquote"]])
def test_unquote_refusals_before_loading(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
    assert b"--unquote" in r.stderr and b"cannot load" not in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("args", [["--records", "--quote", "--field=2", "--fs=,", "--unquote"], ["--records", "--escape", "--field=2,4-", "--unquote"],
                                  ["--records", "--quote", "--escape", "--chomp", "--ors=\\n", "--unquote", "--field=1-", "--fs=;"]])
def test_unquote_reaches_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr, (args, r.stderr)


def test_usage_shows_the_new_line_and_the_old_ones(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--unquote\"" in r.stdout
    assert b"--field=K [--fs=F]\": runs field K (from 1; fields end at F, default a tab) of every record, the rest is copied.\n" in r.stdout
    assert b"--field=LIST [--fs=F]\": the same on every field of LIST (2,5-7,9-); a record is written only if all of them are accepted.\n" in r.stdout


# ---------------------------------------------------------------------------------------------------------- the C entry points
def _list(**kw):
    kw = dict(dict(size=ctypes.sizeof(host.KxBatchFieldList), n_ranges=1, fs=0x2C, quote=34, escape=-1, sep_len=1, keep_sep=1), **kw)
    spec = host.KxBatchFieldList(**kw)
    spec.ranges[0].lo, spec.ranges[0].hi = 2, 0
    return spec


def _codec(special=b"\n", **kw):
    c = host.KxFieldCodec(**dict(dict(size=ctypes.sizeof(host.KxFieldCodec), n_special=len(special)), **kw))
    c.special[:len(special)] = special
    return c


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    lib.kx_last_error.restype = ctypes.c_char_p
    assert ctypes.sizeof(host.KxFieldCodec) == 32 and host.KxFieldCodec.special.offset == 8 and host.KxFieldCodec.reserved.offset == 16
    f = lib.kx_run_batch_field_values
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.POINTER(host.KxBatchFieldList), ctypes.POINTER(host.KxFieldCodec), ctypes.c_void_p,
                                          ctypes.c_size_t] + [ctypes.c_void_p] * 6
    ol = ctypes.c_size_t()
    tail = (None, 0, None, None, None, ctypes.cast(ctypes.byref(ol), ctypes.c_void_p), None, None)
    # (a program handle that is no program: a call that got past the checks would read it and crash, not return -4)
    fake = ctypes.c_void_p(16)
    call = lambda l, c: f(fake, None, None, 0, l, c, *tail)   # noqa: E731
    named = lambda: b"kx_run_batch_field_values" in lib.kx_last_error()   # noqa: E731
    assert f(None, None, None, 0, ctypes.byref(_list()), ctypes.byref(_codec()), *tail) == -4      # a null program
    assert call(ctypes.byref(_list()), None) == -4 and call(None, ctypes.byref(_codec())) == -4      # a null codec, a null list
    for kw in (dict(size=0), dict(size=28), dict(size=ctypes.sizeof(host.KxBatchFieldList)), dict(n_special=9), dict(n_special=1 << 31)):
        assert call(ctypes.byref(_list()), ctypes.byref(_codec(**kw))) == -4 and named(), kw
    for k in range(4):
        c = _codec()
        c.reserved[k] = 1
        assert call(ctypes.byref(_list()), ctypes.byref(c)) == -4 and b"reserved" in lib.kx_last_error()
    assert call(ctypes.byref(_list()), ctypes.byref(_codec(b'\n"'))) == -4 and b"special" in lib.kx_last_error()             # the quote byte
    assert call(ctypes.byref(_list(escape=92)), ctypes.byref(_codec(b"\\"))) == -4 and b"special" in lib.kx_last_error()     # the escape byte
    assert call(ctypes.byref(_list(quote=-1, escape=-1)), ctypes.byref(_codec())) == -4 and b"quote or an escape" in lib.kx_last_error()
    # what kx_run_batch_field_list refuses
    for kw in (dict(size=0), dict(n_ranges=0), dict(n_ranges=9), dict(quote=0x2C), dict(escape=0x2C), dict(quote=34, escape=34), dict(sep_len=9),
               dict(suffix_len=9)):
        assert call(ctypes.byref(_list(**kw)), ctypes.byref(_codec())) == -4 and named(), kw
    l = _list()
    l.reserved[2] = 1
    assert call(ctypes.byref(l), ctypes.byref(_codec())) == -4 and b"reserved" in lib.kx_last_error()
    # the records entry point: a mode without a quote or an escape byte, and kx_run_records_fd_field_list's refusals
    g = lib.kx_run_records_fd_field_values
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(host.KxRecordsOpts), ctypes.POINTER(host.KxFieldRange), ctypes.c_uint32,
                  ctypes.c_uint8, ctypes.c_int, ctypes.c_void_p]
    ro = dict(size=ctypes.sizeof(host.KxRecordsOpts), mode=host.KX_RECORDS_QUOTED, sep=10, quote=34, escape=-1)
    arr = _list().ranges
    assert g(None, 0, 1, None, arr, 1, 0x2C, -1, None) == -4 and g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**ro)), None, 1, 0x2C, -1, None) == -4
    for kw in (dict(ro, mode=host.KX_RECORDS_BYTE), dict(ro, mode=host.KX_RECORDS_RS, rs_len=1)):
        assert g(fake, 0, 1, ctypes.byref(host.KxRecordsOpts(**kw)), arr, 1, 0x2C, -1, None) == -4
        assert b"kx_run_records_fd_field_values" in lib.kx_last_error() and b"quote or an escape" in lib.kx_last_error(), lib.kx_last_error()
    for kw, fs, n in ((ro, 34, 1), (ro, 10, 1), (dict(ro, size=8), 0x2C, 1), (ro, 0x2C, 0), (ro, 0x2C, 9), (dict(ro, mode=host.KX_RECORDS_ESCAPED, escape=92), 92, 1)):
        assert g(fake, 0, 1, ctypes.byref(host.KxRecordsOpts(**kw)), arr, n, fs, -1, None) == -4, (kw, fs, n)
        assert b"kx_run_records_fd_field_values" in lib.kx_last_error()
    assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**ro)), arr, 1, 0x2C, -1, None) == -4 and b"null argument" in lib.kx_last_error()


# ---------------------------------------------------------------------------------------------------------- Python argument checks
def test_python_argument_errors_before_any_device():
    import torch
    for fn, args in ((U, (b"a",)), (R, (b"a", False, b","))):
        with pytest.raises(ValueError, match="quote= or an escape="):
            fn(*args)
        with pytest.raises(ValueError, match="escape character"):
            fn(*args, quote=Q, escape=Q)
        with pytest.raises(ValueError, match="quote character"):
            fn(*args, quote=b"ab")
        with pytest.raises(TypeError, match="bytes"):
            fn("a", *args[1:], quote=Q)
    with pytest.raises(TypeError, match="was_quoted"):
        R(b"a", 1, b",", quote=Q)
    with pytest.raises(ValueError, match="field separator"):
        R(b"a", False, b'"', quote=Q)
    with pytest.raises(ValueError, match="special"):
        R(b"a", False, b",", quote=Q, special=b"123456789")
    with pytest.raises(ValueError, match="special"):
        R(b"a", False, b",", quote=Q, special=b'\n"')
    with pytest.raises(TypeError, match="special"):
        R(b"a", False, b",", quote=Q, special="\n")
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    v, o = torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 2, 4])
    for ranges, kw, exc, what in (([1], {}, ValueError, "quote= or an escape="), ([0], {"quote": Q}, ValueError, "field"),
                                  ("2,3", {"quote": Q}, TypeError, "fields"), ([1], {"quote": Q, "fs": b'"'}, ValueError, "quote"),
                                  ([1], {"quote": Q, "escape": Q}, ValueError, "escape"), ([1], {"quote": Q, "special": b'"'}, ValueError, "special"),
                                  ([1], {"escape": E, "special": b"\\"}, ValueError, "special"), ([1], {"quote": Q, "special": b"123456789"}, ValueError, "special"),
                                  ([1], {"quote": Q, "special": 10}, TypeError, "special"), ([1], {"quote": Q, "sep_len": 9}, ValueError, "sep_len"),
                                  ([1], {"quote": Q, "last_whole": 1}, TypeError, "last_whole"), ([1], {"quote": Q, "keep_sep": 1}, TypeError, "keep_sep"),
                                  ([1], {"quote": Q, "suffix": b"123456789"}, ValueError, "suffix")):
        with pytest.raises(exc, match=what):
            prog.run_batch_field_values_tensor(v, o, ranges, **kw)
    with pytest.raises(host.EngineError, match="HIP device"):
        prog.run_batch_field_values_tensor(v, o, [2], fs=b",", quote=Q)
    for call in (lambda **kw: prog.run_records(b'a,"b"\n', **kw), lambda **kw: prog.run_records_fd(0, 1, **kw)):
        with pytest.raises(ValueError, match="unquote= needs field"):
            call(unquote=True, quote=Q)
        with pytest.raises(ValueError, match="unquote= needs quote"):
            call(unquote=True, field=2, fs=b",")
        with pytest.raises(ValueError, match="unquote= needs quote"):
            call(unquote=True, fields=[2], fs=b",")
        with pytest.raises(ValueError, match="rs="):
            call(unquote=True, fields=[2], fs=b",", quote=Q, rs=b"\r\n")
        with pytest.raises(TypeError, match="unquote"):
            call(unquote=1, field=2, fs=b",", quote=Q)
        with pytest.raises(ValueError, match="exclude"):
            call(unquote=True, field=1, fields=[2], quote=Q)
        with pytest.raises(ValueError, match="field"):
            call(unquote=True, field=0, quote=Q)
