"""CPU: field mode by key (`--field=LIST --keys[=C]`): the parser of the key list, the normative model host.keyed_records_model
against an independent split / partition restatement, what the binary and the C entry points refuse before the engine does any
work, and the two kernels' lane bodies run on the host under a sanitizer (tests/native/field_keys.cpp)."""
import ctypes
import itertools
import os
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "include")


# ---------------------------------------------------------------------------------------------------------- parse_field_keys
@pytest.mark.parametrize("text, want", [
    ("a", ((b"a",), 0, (0,))), ("ts,msg?", ((b"ts", b"msg"), 2, (0, 1))), ("b?,a?", ((b"b", b"a"), 3, (0, 1))),
    ("200", ((b"200",), 0, (0,))), ("2-3,1-", ((b"2-3", b"1-"), 0, (0, 1))),                 # every item is a name
    ("a\\x3F", ((b"a?",), 0, (0,))), ("a\\x3F?", ((b"a?",), 1, (0,))), ("a\\,b,\\\\?", ((b"a,b", b"\\"), 2, (0, 1))),
    ("m,a,m?,a", ((b"m", b"a"), 0, (0, 1, 0, 1))), ("m?,m?", ((b"m",), 1, (0, 0))), ("m?,m", ((b"m",), 0, (0, 0))),
    ("\\n\\t\\r\\0\\x41", ((b"\n\t\r\0A",), 0, (0,))), ("a??", ((b"a?",), 1, (0,))), ("é", (("é".encode(),), 0, (0,))),
    (",".join("k%d" % i for i in range(16)), (tuple(b"k%d" % i for i in range(16)), 0, tuple(range(16)))),
    ("n" * 255 + "?", ((b"n" * 255,), 1, (0,)))])
def test_parse_field_keys(text, want):
    assert host.parse_field_keys(text) == want


@pytest.mark.parametrize("text", ["", "?", "a,,b", "a,", ",a", "a\\", "a\\q", "a\\x4", "a\\x4g", "a,?", "n" * 256, "n" * 256 + "?",
                                  ",".join("k%d" % i for i in range(17)), ",".join(["a"] * 17)])
def test_parse_field_keys_refuses(text):
    with pytest.raises(ValueError):
        host.parse_field_keys(text)
    with pytest.raises(TypeError):
        host.parse_field_keys(text.encode())


# ---------------------------------------------------------------------------------------------------------- the model
def _pack(records):
    data, offs = b"".join(records), [0]
    for r in records:
        offs.append(offs[-1] + len(r))
    return data, offs


def _restate(body, names, optional, kv, fs):
    """the PLAIN model with split / partition: independent of the model's code (fs None: words)"""
    fields = body.split(fs) if fs is not None else body.replace(b"\t", b" ").split()
    found, sel = {}, []
    for f in fields:
        key, c, value = f.partition(kv)
        if c and key in names and key not in found:
            found[key] = value
            sel.append((names.index(key), value))
    if any(n not in found and n not in optional for n in names):
        return sum(1 << names.index(k) for k in found)
    return sel


@pytest.mark.parametrize("names, optional", [([b"a"], ()), ([b"ab"], ()), ([b"a", b"b"], (b"b",)), ([b"b", b"a"], (b"b", b"a")), ([b"b", b"a"], ())])
@pytest.mark.parametrize("blanks", [False, True])
def test_plain_is_split_and_partition(names, optional, blanks):
    fs = None if blanks else b","
    alphabet = b"ab= " if blanks else b"ab=,"
    bodies = [bytes(t) for n in range(6) for t in itertools.product(alphabet, repeat=n)]
    if blanks:
        bodies += [b"a=1\tb=2", b"\ta=\t", b"a=b\t \tb=a"]
    data, offs = _pack([b + b"\n" for b in bodies])
    got = host.keyed_records_model(data, offs, 1, False, names, b"=", fs, blanks=blanks, optional=optional)
    kinds = set()
    for body, g in zip(bodies, got):
        want = _restate(body, names, optional, b"=", fs)
        if isinstance(want, int):
            assert g == want, body
            kinds.add("missing")
            continue
        gaps, fields, sep = g
        assert fields == want and sep == b"\n", body
        assert len(gaps) == len(fields) + 1
        assert b"".join(x for pair in zip(gaps, [v for _, v in fields] + [b""]) for x in pair) == body
        for gap, (t, _) in zip(gaps, fields):
            assert gap.endswith(names[t] + b"=")                                           # the key and C are copied bytes
        kinds.add(len(fields))
    req = [n for n in names if n not in optional]
    assert kinds >= ({"missing"} if req else {0}) | {len(names)} | ({1} if len(req) <= 1 else set())


def test_model_quotes_escapes_and_the_running_state():
    m = host.keyed_records_model
    d, o = _pack([b'ts=1 level=info msg="a b" msg=x\n', b'k="a=b",x=1\n', b"a\\=b=c,a=d\n", b'"k"=v k=w\n', b'x="1,a=2",a=3'])
    assert m(d, o[:2], 1, False, [b"msg", b"ts"], b"=", None, b'"', None, True) == [
        ([b"ts=", b" level=info msg=", b" msg=x"], [(1, b"1"), (0, b'"a b"')], b"\n")]
    assert m(d, o[1:3], 1, False, [b"k", b"x"], b"=", b",", b'"') == [([b"k=", b",x=", b""], [(0, b'"a=b"'), (1, b"1")], b"\n")]
    assert m(d, o[2:4], 1, False, [b"a"], b"=", b",", None, b"\\") == [([b"a\\=b=c,a=", b""], [(0, b"d")], b"\n")]   # the key is a\=b
    assert m(d, o[3:5], 1, False, [b"k"], b"=", None, b'"', None, True) == [([b'"k"=v k=', b""], [(0, b"w")], b"\n")]   # keys are raw bytes
    assert m(d, o[3:5], 1, False, [b'"k"'], b"=", None, b'"', None, True) == [([b'"k"=', b" k=w"], [(0, b"v")], b"\n")]
    assert m(d, o[4:], 1, True, [b"a"], b"=", b",", b'"') == [([b'x="1,a=2",a=', b""], [(0, b"3")], b"")]
    assert m(d, o[4:], 1, True, [b"a", b"zz"], b"=", b",", b'"') == [1]
    assert m(b"", [0], 1, False, [b"a"]) == []
    assert m(b"=v\n", [0, 3], 1, False, [b"a"], optional=[b"a"]) == [([b"=v"], [], b"\n")]                  # an empty key matches nothing


def test_model_argument_checks():
    m = host.keyed_records_model
    for bad in (dict(kv=b","), dict(kv=b'"', quote=b'"'), dict(kv=b"\\", escape=b"\\"), dict(names=[b"a=b"]), dict(names=[b"a,b"]), dict(names=[b""]),
                dict(names=[b"n" * 256]), dict(names=[b"a", b"a"]), dict(names=[b"k%d" % i for i in range(17)]), dict(optional=[b"zz"])):
        kw = dict(dict(names=[b"a"], kv=b"=", fs=b","), **bad)
        with pytest.raises(ValueError):
            m(b"a=1\n", [0, 4], 1, False, **kw)
    with pytest.raises(ValueError):
        m(b"a=1\n", [0, 4], 1, False, [b"a"], b" ", None, blanks=True)
    with pytest.raises(ValueError):
        m(b"a=1\n", [0, 4], 1, False, [b"a b"], b"=", None, blanks=True)
    with pytest.raises(ValueError, match="blanks"):
        m(b"a=1\n", [0, 4], 1, False, [b"a"], b"=", b",", blanks=True)
    with pytest.raises(TypeError):
        m(b"a=1\n", [0, 4], 1, False, ["a"])
    with pytest.raises(ValueError, match="optional= needs keys="):
        host.Program._check_keys("t", None, [b"a"], None, [b"a"], None, False, None, None, b"\n", None, 0)
    with pytest.raises(ValueError, match="header"):
        host.Program._check_keys("t", b"=", (), None, [b"a"], None, False, None, None, b"\n", None, 1)
    with pytest.raises(ValueError, match="needs fields="):
        host.Program._check_keys("t", b"=", (), 2, None, None, False, None, None, b"\n", None, 0)
    with pytest.raises(ValueError):
        host.Program._check_keys("t", b"\n", (), None, [b"a"], None, False, None, None, b"\n", None, 0)   # C is the record separator
    with pytest.raises(ValueError):
        host.Program._check_keys("t", b"=", (), None, [b"a;b"], None, False, None, None, b";", None, 0)    # a name holds it
    assert host.Program._check_keys("t", b"=", [b"b"], None, [b"a", b"b", b"a"], None, True, None, None, b"\n", None, 0) == ((b"a", b"b"), 2, (0, 1, 0), 61)


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("reckeys") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"a=b\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


SEVENTEEN = "--field=" + ",".join("k%d" % i for i in range(17))


@pytest.mark.parametrize("args, what", [
    (["--records", "--keys"], b"--keys needs --field"), (["--keys"], b"--keys needs --field"),
    (["--records", "--keys", "--field=a", "--header"], b"--keys cannot be combined with --header"),
    (["--records", "--header=2", "--field=a", "--keys=:"], b"--keys cannot be combined with --header"),
    (["--records", SEVENTEEN, "--keys"], b"more than 16 items"), (["--records", "--keys", "--field=a,,b"], b"an empty name"),
    (["--records", "--keys", "--field=?"], b"an empty name"), (["--records", "--keys", "--field=" + "n" * 256], b"at most 255 bytes"),
    (["--records", "--keys", "--field=a\\q"], b"--field"), (["--records", "--keys=ab", "--field=a"], b"Invalid --keys: ab"),
    (["--records", "--keys=\\t", "--field=a"], b"the --keys character cannot be the field separator"),
    (["--records", "--keys=,", "--field=a", "--fs=,"], b"the --keys character cannot be the field separator"),
    (["--records", "--keys=\\n", "--field=a"], b"the --keys character cannot be the record separator"),
    (["--records=;", "--keys=;", "--field=a"], b"the --keys character cannot be the record separator"),
    (["--records", "--rs=;", "--keys=;", "--field=a"], b"the --keys character cannot be the record separator"),
    (["--records", "--quote", "--keys=\"", "--field=a"], b"the --keys character cannot be the quote character"),
    (["--records", "--escape", "--keys=\\\\", "--field=a"], b"the --keys character cannot be the escape character"),
    (["--records", "--blanks", "--keys= ", "--field=a"], b"the --keys character cannot be a blank"),
    (["--records", "--blanks", "--keys=\\t", "--field=a"], b"the --keys character cannot be a blank"),
    (["--records", "--keys", "--field=a=b"], b"cannot hold the key separator"), (["--records", "--keys=:", "--field=ts,a:b?"], b"cannot hold the key separator"),
    (["--records", "--keys", "--field=a\\tb"], b"cannot hold the field separator"), (["--records", "--keys", "--fs=,", "--field=a\\,b"], b"cannot hold the field separator"),
    (["--records", "--keys", "--blanks", "--field=a b"], b"cannot hold a blank"), (["--records", "--keys", "--field=a\\nb"], b"cannot hold the record separator"),
    (["--keys", "--field=a"], b"--field needs --records"), (["--records", "--keys", "--field=a", "--ofs=,"], b"--ofs needs --only"),
    (["--records", "--keys", "--field=a", "--blanks", "--fs=,"], b"--blanks cannot be combined with --fs"),
    (["--records", "--keys", "--field=a", "--unquote"], b"--unquote needs --quote or --escape"),
    (["--records", "--quote", "--keys", "--field=a,b", "--fs=,", "--unquote", "--only", "--ofs=, "], b"--ofs is exactly one byte"),
    (["--records", "--quote", "--keys", "--field=a,b", "--blanks", "--unquote", "--only", "--ofs=\\t"], b"--ofs cannot be the tab")])
def test_refusals_before_loading(flip_bin, args, what):
    r = _run(flip_bin, *args)
    assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
    assert what in r.stderr and b"cannot load" not in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("args", [
    ["--records", "--keys", "--field=a"], ["--records", "--field=ts,msg?", "--keys", "--blanks"], ["--records", "--keys=:", "--field=200", "--fs=;"],
    ["--records", "--quote", "--blanks", "--keys", "--field=msg", "--unquote"], ["--records", "--keys", "--field=b,a,b", "--only", "--ofs=12345678"],
    ["--records", "--escape", "--keys", "--field=a\\x3F", "--fs=,", "--unquote", "--only", "--chomp", "--ors=\\n"],
    ["--records", "--rs=\\r\\n", "--keys", "--field=a\\rb"], ["--records", "--keys", "--field=" + ",".join("k%d" % i for i in range(16))]])
def test_good_command_lines_reach_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr and r.stdout == b"", (args, r.stderr)


def test_usage(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"With --keys[=C] in place of --header the fields are key=value pairs" in r.stdout


# ---------------------------------------------------------------------------------------------------------- the C entry points
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def test_abi_is_declared_and_exported():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_run_batch_field_keys", "kx_run_records_fd_field_keys"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]   # noqa: E731
    assert args("kx_run_batch_field_keys") == ["prog", "d_in", "d_in_off", "n_docs", "list", "keys", "codec", "proj", "d_out", "cap", "d_out_off",
                                               "d_docs", "d_fail_field", "out_len", "stats", "stream"]
    assert args("kx_run_records_fd_field_keys") == ["p", "in_fd", "out_fd", "o", "keys", "fs", "items", "n_items", "ofs", "ofs_len", "report_fd", "stats"]
    assert ctypes.sizeof(host.KxFieldKeys) == 232 and host.KxFieldKeys.optional_mask.offset == 200 and host.KxFieldKeys.flags.offset == 208
    # the structs that were there keep their layout
    assert ctypes.sizeof(host.KxBatchFieldList) == 124 and ctypes.sizeof(host.KxFieldCodec) == 32 and ctypes.sizeof(host.KxFieldProject) == 168


def spec_list(**kw):
    kw = dict(dict(size=ctypes.sizeof(host.KxBatchFieldList), n_ranges=0, fs=44, quote=-1, escape=-1, sep_len=1, keep_sep=1), **kw)
    return host.KxBatchFieldList(**kw)


def spec_keys(names=(b"a", b"b"), mask=0, kv=61, flags=0, **kw):
    k = host.field_keys_struct(list(names), mask, kv, flags)
    for name, v in kw.items():
        setattr(k, name, v)
    return k


def spec_proj(items, ofs=b";", **kw):
    p = host.KxFieldProject(**dict(dict(size=ctypes.sizeof(host.KxFieldProject), n_items=len(items), ofs_len=len(ofs)), **kw))
    for j, (lo, hi) in enumerate(items[:16]):
        p.items[j].lo, p.items[j].hi = lo, hi
    p.ofs[:min(len(ofs), 8)] = ofs[:8]
    return p


def spec_codec(special=b"\n"):
    c = host.KxFieldCodec(size=ctypes.sizeof(host.KxFieldCodec), n_special=len(special))
    c.special[:len(special)] = special
    return c


def abi_refusals():
    """(list, keys, codec or None, projection or None, a piece of the message) of every call kx_run_batch_field_keys refuses"""
    reserved, padded, null_name = spec_keys(), spec_keys(), spec_keys()
    reserved.reserved[2] = 1
    padded.pad[1] = 1
    null_name.names[1] = None
    ranged = spec_list(n_ranges=1)
    ranged.ranges[0].lo = ranged.ranges[0].hi = 1
    q = dict(quote=34)
    return [
        (spec_list(), spec_keys(size=228), None, None, b"kx_field_keys::size"), (spec_list(), spec_keys(size=0), None, None, b"kx_field_keys::size"),
        (spec_list(size=120), spec_keys(), None, None, b"kx_batch_field_list::size"), (ranged, spec_keys(), None, None, b"n_ranges must be 0"),
        (spec_list(), spec_keys(n_names=0), None, None, b"1 to 16 names"), (spec_list(), spec_keys(n_names=17), None, None, b"1 to 16 names"),
        (spec_list(), reserved, None, None, b"reserved"), (spec_list(), padded, None, None, b"reserved"),
        (spec_list(), spec_keys(flags=2), None, None, b"unknown flag"), (spec_list(), spec_keys(mask=4), None, None, b"optional_mask"),
        (spec_list(), null_name, None, None, b"null name"), (spec_list(), spec_keys((b"a", b"")), None, None, b"1 to 255 bytes"),
        (spec_list(), spec_keys((b"a", b"n" * 256)), None, None, b"1 to 255 bytes"), (spec_list(), spec_keys((b"a", b"b", b"a")), None, None, b"two names are equal"),
        (spec_list(), spec_keys(kv=44), None, None, b"key separator cannot be the field separator"),
        (spec_list(**q), spec_keys(kv=34), None, None, b"key separator cannot be the quote"),
        (spec_list(escape=92), spec_keys(kv=92), None, None, b"key separator cannot be the escape"),
        (spec_list(fs=0), spec_keys(kv=32, flags=1), None, None, b"key separator cannot be a blank"),
        (spec_list(fs=0), spec_keys(kv=9, flags=1), None, None, b"key separator cannot be a blank"),
        (spec_list(), spec_keys(flags=1), None, None, b"fs must be 0"),
        (spec_list(), spec_keys((b"a=b",)), None, None, b"a name cannot hold the key separator"),
        (spec_list(), spec_keys((b"a", b"x,y")), None, None, b"a name cannot hold the field separator"),
        (spec_list(fs=0), spec_keys((b"a b",), flags=1), None, None, b"a name cannot hold a blank"),
        (spec_list(fs=61), spec_keys(), None, None, b"key separator cannot be the field separator"),
        (spec_list(), spec_keys(), spec_codec(), None, b"values need a quote or an escape"),
        (spec_list(sep_len=9), spec_keys(), None, None, b"kx_run_batch_field_keys"),
        (spec_list(), spec_keys(), None, spec_proj([(0, 0)], size=164), b"kx_field_project::size"),
        (spec_list(), spec_keys(), None, spec_proj([]), b"1 to 16 items"), (spec_list(), spec_keys(), None, spec_proj([(0, 2)]), b"the index of a name"),
        (spec_list(), spec_keys(), None, spec_proj([(1, 1)]), b"the index of a name"), (spec_list(), spec_keys(), None, spec_proj([(0, 1)], ofs_len=9), b"at most 8 bytes"),
        (spec_list(**q), spec_keys(), spec_codec(), spec_proj([(0, 1)], ofs=b", "), b"exactly one byte"),
        (spec_list(**q), spec_keys(), spec_codec(), spec_proj([(0, 1)], ofs=b'"'), b"cannot be the quote or the escape"),
        (spec_list(**q), spec_keys(), spec_codec(), spec_proj([(0, 1)], ofs=b"\n"), b"cannot be a special byte")]


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    f, err = lib.kx_run_batch_field_keys, lib.kx_last_error
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.POINTER(host.KxBatchFieldList), ctypes.POINTER(host.KxFieldKeys),
                                          ctypes.POINTER(host.KxFieldCodec), ctypes.POINTER(host.KxFieldProject), ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 6
    err.restype = ctypes.c_char_p
    ol = ctypes.c_size_t()
    tail = (None, 0, None, None, None, ctypes.cast(ctypes.byref(ol), ctypes.c_void_p), None, None)
    # (a program handle that is no program: a call that got past the checks would read it and crash, not return -4)
    fake = ctypes.c_void_p(16)
    assert f(fake, None, None, 0, ctypes.byref(spec_list()), None, None, None, *tail) == -4                   # null keys
    assert f(fake, None, None, 0, None, ctypes.byref(spec_keys()), None, None, *tail) == -4                   # a null list
    for lst, keys, codec, proj, what in abi_refusals():
        assert f(fake, None, None, 0, ctypes.byref(lst), ctypes.byref(keys), ctypes.byref(codec) if codec else None,
                 ctypes.byref(proj) if proj else None, *tail) == -4, what
        assert b"kx_run_batch_field_keys" in err() and what in err(), (what, err())
    g = lib.kx_run_records_fd_field_keys
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(host.KxRecordsOpts), ctypes.POINTER(host.KxFieldKeys), ctypes.c_uint8,
                  ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    o = host.KxRecordsOpts(size=ctypes.sizeof(host.KxRecordsOpts), mode=host.KX_RECORDS_QUOTED, sep=10, quote=34, escape=-1)
    items = (ctypes.c_uint32 * 16)(1, 0, 2)
    for keys, fs, n, ofs, what in ((spec_keys(size=4), 44, 0, b"", b"kx_field_keys::size"), (spec_keys(flags=8), 44, 0, b"", b"unknown flag"),
                                   (spec_keys(kv=10), 44, 0, b"", b"key separator cannot be the record separator"),
                                   (spec_keys((b"a\nb",)), 44, 0, b"", b"a name cannot hold the record separator"),
                                   (spec_keys(), 10, 0, b"", b"field separator cannot be the record separator"),
                                   (spec_keys(kv=34), 44, 0, b"", b"key separator cannot be the quote"),
                                   (spec_keys(flags=4), 44, 0, b";", b"1 to 16 items"), (spec_keys(flags=4), 44, 17, b";", b"1 to 16 items"),
                                   (spec_keys(flags=4), 44, 3, b";", b"an item is the index of a name"), (spec_keys(flags=4), 44, 2, b"123456789", b"at most 8 bytes"),
                                   (spec_keys(flags=6), 44, 2, b", ", b"exactly one byte"), (spec_keys(flags=6), 44, 2, b"\n", b"cannot be the record separator"),
                                   (spec_keys(flags=7), 0, 2, b"\t", b"cannot be the tab")):
        assert g(fake, 0, 1, ctypes.byref(o), ctypes.byref(keys), fs, items, n, ofs, len(ofs), -1, None) == -4, what
        assert b"kx_run_records_fd_field_keys" in err() and what in err(), (what, err())
    o.mode, o.quote = host.KX_RECORDS_BYTE, -1
    assert g(fake, 0, 1, ctypes.byref(o), ctypes.byref(spec_keys(flags=2)), 44, items, 0, b"", 0, -1, None) == -4 and b"values need a quote or an escape" in err()


# ---------------------------------------------------------------------------------------------------------- the lane bodies
def test_lane_bodies_against_a_plain_reference_under_a_sanitizer(tmp_path):
    """tests/native/field_keys.cpp: the parser, and k_kvcount's and k_kvlocate's lane bodies (kx_field_keys_lanes.h, the text the GPU
    runs) one lane at a time over every small body at every start residue, in a stand-alone program built with AddressSanitizer and
    UBSan (a CPU machine's job: skipped where a GPU is present)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = str(tmp_path / "field_keys")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "native", "field_keys.cpp")], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"every lane equal" in r.stdout, (r.stdout[-400:], r.stderr[-3000:])
