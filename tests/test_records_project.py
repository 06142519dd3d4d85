"""CPU: the projection of field mode (`--field=LIST --only [--ofs=STR]`): the written-order parser, the normative model
host.project_records_model against independent Python, what the binary and the C entry point refuse before the engine does any
work, and the two kernels' lane bodies run on the host under a sanitizer (tests/native/project_lanes.cpp)."""
import csv
import ctypes
import io
import os
import random
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "include")


# ---------------------------------------------------------------------------------------------------------- parse_field_order
@pytest.mark.parametrize("text, want", [
    ("4,2", ((4, 4), (2, 2))), ("2,1,2", ((2, 2), (1, 1), (2, 2))), ("3-,1-2", ((3, None), (1, 2))), ("7", ((7, 7),)),
    ("1-", ((1, None),)), ("6-,3-4,1", ((6, None), (3, 4), (1, 1))), ("5-9,5-9", ((5, 9), (5, 9))),
    ("4294967295,1", ((4294967295, 4294967295), (1, 1))),
    (",".join(str(k) for k in range(16, 0, -1)), tuple((k, k) for k in range(16, 0, -1)))])
def test_parse_field_order_keeps_the_text(text, want):
    assert host.parse_field_order(text) == want
    assert host._normal_field_ranges(want, "test") == host.parse_field_list(text)           # its union is the list's normal form
    assert host._check_field_items(want) == (want, host.parse_field_list(text))


@pytest.mark.parametrize("text", [",".join(["1"] * 17), ",".join(str(2 * k) for k in range(1, 10)), "-3", "5-2", "0", "2,,3", "", "2,",
                                  "a", "1-2-3", "4294967296", "2 ,3", "01234567890"])
def test_parse_field_order_refuses(text):
    with pytest.raises(ValueError):
        host.parse_field_order(text)


def test_parse_field_order_counts_items_not_ranges():
    assert len(host.parse_field_order(",".join(["3"] * 16))) == 16                          # 16 items, one range
    assert host.parse_field_list(",".join(["1"] * 17)) == ((1, 1),)                         # (the set has no such limit)
    with pytest.raises(TypeError):
        host.parse_field_order(b"1,2")
    with pytest.raises(ValueError, match="at most 16"):
        host._check_field_items([1] * 17)


# ---------------------------------------------------------------------------------------------------------- the model
def _pack(records):
    data, offs = b"".join(records), [0]
    for r in records:
        offs.append(offs[-1] + len(r))
    return data, offs


def _expand(items, nf):
    """the field numbers a record of nf fields writes, in order: independent of the model's code"""
    out = []
    for lo, hi in items:
        out += list(range(lo, min(nf, nf if hi is None else hi) + 1))
    return out


ITEM_LISTS = ["4,2", "2,1,2", "3-,1-2", "1-", "6-,3-4,1", "2", "3-,5-6,4", ",".join(["2", "1"] * 8)]


@pytest.mark.parametrize("text", ITEM_LISTS)
def test_plain_is_split(text):
    rnd = random.Random(text)
    items = host.parse_field_order(text)
    need = host.field_list_need(host.parse_field_list(text))
    bodies = [bytes(rnd.choice(b"ab,;") for _ in range(rnd.randrange(0, 14))) for _ in range(300)] + [b"", b",", b",,,,,,,"]
    data, offs = _pack([b + b"\r\n" for b in bodies])
    got = host.project_records_model(data, offs, 2, False, items, b",")
    for body, g in zip(bodies, got):
        fields = body.split(b",")
        if len(fields) < need:
            assert g == len(fields)
        else:
            assert g == ([(k, fields[k - 1]) for k in _expand(items, len(fields))], b"\r\n") and g[0]


@pytest.mark.parametrize("text", ITEM_LISTS)
def test_blanks_is_split_without_an_argument(text):
    rnd = random.Random(text)
    items = host.parse_field_order(text)
    need = host.field_list_need(host.parse_field_list(text))
    bodies = [bytes(rnd.choice(b"ab \t") for _ in range(rnd.randrange(0, 16))) for _ in range(300)] + [b"", b" ", b"\t \t"]
    data, offs = _pack([b + b"\n" for b in bodies[:-1]] + [bodies[-1]])
    got = host.project_records_model(data, offs, 1, True, items, None, blanks=True)
    for i, (body, g) in enumerate(zip(bodies, got)):
        words = body.split()
        if len(words) < need:
            assert g == len(words)
        else:
            assert g == ([(k, words[k - 1]) for k in _expand(items, len(words))], b"" if i == len(bodies) - 1 else b"\n")
    with pytest.raises(ValueError, match="blanks"):
        host.project_records_model(data, offs, 1, True, items, b" ", blanks=True)


@pytest.mark.parametrize("ofs", [b"\t", b"|", b","])
def test_quoted_rows_through_the_csv_module(ofs):
    """rows written by csv.writer; the values of the projected fields, spelled with fs = OFS, are read back by csv.reader"""
    rnd = random.Random(ofs)
    alphabet = ["a", "b", ",", '"', "\t", "|", " ", "\n"]
    rows = [["".join(rnd.choice(alphabet) for _ in range(rnd.randrange(0, 6))) for _ in range(rnd.randrange(4, 8))] for _ in range(200)]
    buf = io.StringIO()
    csv.writer(buf, lineterminator="\n").writerows(rows)
    data = buf.getvalue().encode()
    offs = list(host.split_records_model(data, b"\n", b'"'))
    assert len(offs) - 1 == len(rows)
    items = host.parse_field_order("4,2-3,2")
    got = host.project_records_model(data, offs, 1, False, items, b",", quote=b'"')
    lines = []
    for row, (fields, sep) in zip(rows, got):
        assert sep == b"\n" and [k for k, _ in fields] == [4, 2, 3, 2]
        values = [host.unquote_field_model(raw, quote=b'"') for _, raw in fields]
        assert values == [row[k - 1].encode() for k in (4, 2, 3, 2)]
        lines.append(ofs.join(host.requote_field_model(v, raw[:1] == b'"', ofs, quote=b'"') for v, (_, raw) in zip(values, fields)) + sep)
    back = list(csv.reader(io.StringIO(b"".join(lines).decode(), newline=""), delimiter=ofs.decode()))
    assert back == [[row[k - 1] for k in (4, 2, 3, 2)] for row in rows]


def test_no_field_empty_bodies_and_items_the_record_lacks():
    data, offs = _pack([b"\n", b"a\n", b"a;b\n", b"a;b;c;d;e"])
    assert host.project_records_model(data, offs, 1, True, [2, 1], b";") == [1, 1, ([(2, b"b"), (1, b"a")], b"\n"), ([(2, b"b"), (1, b"a")], b"")]
    assert host.project_records_model(data, offs, 1, True, [1], b";")[0] == ([(1, b"")], b"\n")          # the empty body has one empty field
    # an item inside the union's open range whose fields a record does not have writes nothing: need is 3, not 10
    got = host.project_records_model(data, offs, 1, True, host.parse_field_order("9-10,3-,4"), b";")
    assert got == [1, 1, 2, ([(3, b"c"), (4, b"d"), (5, b"e"), (4, b"d")], b"")]
    assert host.project_records_model(b"", [0], 1, False, [1], b";") == []


@pytest.mark.parametrize("quote, escape", [(None, None), (b'"', None), (b'"', b"\\"), (None, b"\\")])
def test_a_one_item_list_is_the_list_models_field(quote, escape):
    rnd = random.Random(7)
    bodies = [bytes(rnd.choice(b'ab;"\\') for _ in range(rnd.randrange(0, 12))) for _ in range(200)]
    data, offs = _pack([b + b"\n" for b in bodies])
    for K in (1, 2, 4):
        want = host.field_list_records_model(data, offs, 1, False, [K], b";", quote, escape)
        got = host.project_records_model(data, offs, 1, False, [(K, K)], b";", quote, escape)
        assert got == [w if isinstance(w, int) else (w[1], w[2]) for w in want]


def test_model_and_wrapper_argument_checks():
    with pytest.raises(TypeError):
        host.project_records_model(b"a\n", [0, 2], 1, False, "2,1", b";")
    with pytest.raises(ValueError):
        host.project_records_model(b"a\n", [0, 2], 1, False, [], b";")
    with pytest.raises(ValueError):
        host.project_records_model(b"a\n", [0, 2], 1, False, [(3, 2)], b";")
    with pytest.raises(TypeError):
        host.project_records_model(b"a\n", [0, 2], 1, False, [1], b";", blanks=1)
    with pytest.raises(ValueError, match="ofs= needs only="):
        host.Program._check_only("t", False, b",", None, [1], None, False)
    with pytest.raises(ValueError, match="only= needs"):
        host.Program._check_only("t", True, None, None, None, None, False)
    assert host.Program._check_only("t", True, None, None, [2, (1, None)], b";", False) == (((2, 2), (1, None)), b";")
    assert host.Program._check_only("t", True, None, 3, None, None, True) == (((3, 3),), b" ")
    assert host.Program._check_only("t", True, b"", None, [1], None, False) == (((1, 1),), b"")
    with pytest.raises(ValueError, match="0 to 8"):
        host.Program._check_only("t", True, b"123456789", None, [1], None, False)
    with pytest.raises(ValueError, match="exactly one byte"):
        host._check_ofs_codec("t", b", ", 34, None, b"\n")
    for bad in (b'"', b"\n"):
        with pytest.raises(ValueError, match="cannot be"):
            host._check_ofs_codec("t", bad, 34, None, b"\n")


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recproject") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


SEVENTEEN = "--field=" + ",".join(["1"] * 17)
NINE_RANGES = "--field=" + ",".join(str(2 * k) for k in range(1, 10))


@pytest.mark.parametrize("args, what", [
    (["--records", "--only"], b"--only needs --field"), (["--only"], b"--only needs --field"),
    (["--records", "--field=2", "--ofs=,"], b"--ofs needs --only"), (["--records", "--ofs=,"], b"--ofs needs --only"),
    (["--records", SEVENTEEN, "--only"], b"--field"), (["--records", "--only", SEVENTEEN, "--fs=,"], b"at most 16 items"),
    (["--records", NINE_RANGES, "--only"], b"more than 8 ranges"),
    (["--records", "--field=2,1", "--only", "--ofs=123456789"], b"Invalid output field separator: 123456789"),
    (["--records", "--field=2,1", "--only", "--ofs=\\q"], b"Invalid output field separator: \\q"),
    (["--records", "--field=-3", "--only"], b"--field"), (["--records", "--field=5-2", "--only"], b"--field"),
    (["--records", "--field=0", "--only"], b"--field"), (["--records", "--field=2,,1", "--only"], b"--field"),
    (["--field=2,1", "--only"], b"--field needs --records"),
    (["--records", "--field=2,1", "--only", "--blanks", "--fs=,"], b"--blanks cannot be combined with --fs"),
    (["--records", "--field=2,1", "--only", "--unquote"], b"--unquote needs --quote or --escape"),
    (["--records=,", "--field=2,1", "--fs=,", "--only"], b"--fs cannot be the record separator"),
    (["--records", "--quote", "--field=2,1", "--fs=,", "--unquote", "--only", "--ofs=, "], b"--ofs is exactly one byte"),
    (["--records", "--quote", "--field=2,1", "--fs=,", "--unquote", "--only", "--ofs="], b"--ofs is exactly one byte"),
    (["--records", "--quote", "--field=2,1", "--fs=,", "--unquote", "--only", "--ofs=\""], b"--ofs cannot be the --quote character"),
    (["--records", "--escape", "--field=2,1", "--fs=,", "--unquote", "--only", "--ofs=\\\\"], b"--ofs cannot be the --escape character"),
    (["--records", "--quote", "--field=2,1", "--fs=,", "--unquote", "--only", "--ofs=\\n"], b"--ofs cannot be the record separator"),
    (["--records=;", "--quote", "--field=2,1", "--fs=,", "--unquote", "--only", "--ofs=;"], b"--ofs cannot be the record separator")])
def test_refusals_before_loading(flip_bin, args, what):
    r = _run(flip_bin, *args)
    assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
    assert what in r.stderr and b"cannot load" not in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("args", [
    ["--records", "--field=4,2", "--fs=,", "--only", "--ofs=\\t"], ["--records", "--field=2,1,2", "--only"], ["--records", "--only", "--field=3"],
    ["--records", "--field=3-,1-2", "--only", "--ofs="], ["--records", "--field=1-", "--only", "--ofs=12345678", "--chomp", "--ors=\\n"],
    ["--records", "--field=" + ",".join(["1"] * 16), "--only"], ["--records", "--field=2,1", "--blanks", "--only"],
    ["--records", "--quote", "--field=2,1", "--fs=,", "--unquote", "--only"], ["--records", "--quote", "--field=2,1", "--fs=,", "--unquote", "--only", "--ofs=\\t"],
    ["--records", "--rs=\\r\\n", "--field=2,1", "--only", "--ofs=\\r"], ["--records", "--quote", "--field=2,1", "--fs=,", "--only", "--ofs=\"\""],
    ["--records", "--escape", "--field=2,1", "--blanks", "--unquote", "--only"]])
def test_good_command_lines_reach_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr and r.stdout == b"", (args, r.stderr)


def test_usage_and_what_stays(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--only [--ofs=STR]\"" in r.stdout
    r = _run(flip_bin, "--records", SEVENTEEN)                                               # without --only a set has no item limit
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr
    r = _run(flip_bin, "--records", "--field=3,2")
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr


# ---------------------------------------------------------------------------------------------------------- the C entry points
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def test_abi_is_declared_and_exported():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_run_batch_field_project", "kx_run_records_fd_field_project"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]   # noqa: E731
    assert args("kx_run_batch_field_project") == ["prog", "d_in", "d_in_off", "n_docs", "list", "codec", "proj", "d_out", "cap", "d_out_off",
                                                  "d_docs", "d_fail_field", "out_len", "stats", "stream"]
    assert args("kx_run_records_fd_field_project") == ["p", "in_fd", "out_fd", "o", "items", "n_items", "fs", "ofs", "ofs_len", "flags",
                                                       "report_fd", "stats"]
    assert ctypes.sizeof(host.KxFieldProject) == 168 and host.KxFieldProject.flags.offset == 148
    # the structs that were there keep their layout
    assert ctypes.sizeof(host.KxBatchFieldList) == 124 and ctypes.sizeof(host.KxFieldCodec) == 32 and ctypes.sizeof(host.KxRecordsOpts) == 64


def spec_list(ranges, **kw):
    kw = dict(dict(size=ctypes.sizeof(host.KxBatchFieldList), fs=59, quote=-1, escape=-1, sep_len=1, keep_sep=1), **kw)
    spec = host.KxBatchFieldList(n_ranges=len(ranges), **kw)
    for j, (lo, hi) in enumerate(ranges):
        spec.ranges[j].lo, spec.ranges[j].hi = lo, hi
    return spec


def spec_proj(items, ofs=b";", n=None, **kw):
    p = host.KxFieldProject(**dict(dict(size=ctypes.sizeof(host.KxFieldProject), n_items=len(items) if n is None else n, ofs_len=len(ofs)), **kw))
    for j, (lo, hi) in enumerate(items[:16]):
        p.items[j].lo, p.items[j].hi = lo, hi
    p.ofs[:min(len(ofs), 8)] = ofs[:8]
    return p


def spec_codec(special=b"\n"):
    c = host.KxFieldCodec(size=ctypes.sizeof(host.KxFieldCodec), n_special=len(special))
    c.special[:len(special)] = special
    return c


def abi_refusals():
    """(list, codec or None, projection, a piece of the message) of every call kx_run_batch_field_project refuses with KX_E_ARG"""
    good_items, good_ranges = [(4, 4), (2, 2)], [(2, 2), (4, 4)]
    reserved = spec_proj(good_items)
    reserved.reserved[3] = 1
    q = dict(quote=34)
    return [
        (spec_list(good_ranges), None, spec_proj(good_items, size=164), b"kx_field_project::size"),
        (spec_list(good_ranges), None, spec_proj(good_items, size=0), b"kx_field_project::size"),
        (spec_list([(1, 1)]), None, spec_proj([(1, 1)] * 16, n=17), b"1 to 16 items"),
        (spec_list([(1, 1)]), None, spec_proj([], n=0), b"1 to 16 items"),
        (spec_list(good_ranges), None, spec_proj([(4, 2), (2, 2)]), b"an item needs"),
        (spec_list(good_ranges), None, spec_proj([(0, 0), (2, 2)]), b"an item needs"),
        (spec_list(good_ranges), None, spec_proj(good_items, ofs_len=9), b"at most 8 bytes"),
        (spec_list(good_ranges), None, spec_proj(good_items, flags=2), b"unknown flag"),
        (spec_list(good_ranges), None, spec_proj(good_items, flags=0x80000000), b"unknown flag"),
        (spec_list(good_ranges), None, reserved, b"reserved"),
        (spec_list([(2, 4)]), None, spec_proj(good_items), b"not the normal form of the items' union"),
        (spec_list([(4, 4), (2, 2)]), None, spec_proj(good_items), b"normal form"),
        (spec_list([(2, 2)]), None, spec_proj(good_items), b"not the normal form of the items' union"),
        (spec_list([(2, 2), (4, 0)]), None, spec_proj(good_items), b"not the normal form of the items' union"),
        (spec_list([(2 * k, 2 * k) for k in range(1, 9)]), None, spec_proj([(2 * k, 2 * k) for k in range(1, 10)]), b"more than 8 ranges"),
        (spec_list(good_ranges, **q), spec_codec(), spec_proj(good_items, ofs=b", "), b"exactly one byte"),
        (spec_list(good_ranges, **q), spec_codec(), spec_proj(good_items, ofs=b""), b"exactly one byte"),
        (spec_list(good_ranges, **q), spec_codec(), spec_proj(good_items, ofs=b'"'), b"cannot be the quote or the escape"),
        (spec_list(good_ranges, quote=34, escape=92), spec_codec(), spec_proj(good_items, ofs=b"\\"), b"cannot be the quote or the escape"),
        (spec_list(good_ranges, **q), spec_codec(), spec_proj(good_items, ofs=b"\n"), b"cannot be a special byte"),
        (spec_list(good_ranges, fs=0, **q), spec_codec(), spec_proj(good_items, ofs=b"\t", flags=1), b"cannot be a special byte"),
        (spec_list(good_ranges, **q), None, spec_proj(good_items, flags=1), b"fs must be 0"),
        (spec_list(good_ranges), spec_codec(), spec_proj(good_items), b"values need a quote or an escape"),
        (spec_list(good_ranges, size=120), None, spec_proj(good_items), b"kx_batch_field_list::size")]


def project_entry(lib):
    f = lib.kx_run_batch_field_project
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.POINTER(host.KxBatchFieldList), ctypes.POINTER(host.KxFieldCodec),
                                          ctypes.POINTER(host.KxFieldProject), ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 6
    lib.kx_last_error.restype = ctypes.c_char_p
    return f


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    f, err = project_entry(lib), lib.kx_last_error
    ol = ctypes.c_size_t()
    tail = (None, 0, None, None, None, ctypes.cast(ctypes.byref(ol), ctypes.c_void_p), None, None)
    # (a program handle that is no program: a call that got past the checks would read it and crash, not return -4)
    fake = ctypes.c_void_p(16)
    assert f(fake, None, None, 0, ctypes.byref(spec_list([(2, 2)])), None, None, *tail) == -4            # a null projection
    assert f(fake, None, None, 0, None, None, ctypes.byref(spec_proj([(2, 2)])), *tail) == -4            # a null list
    for lst, codec, proj, what in abi_refusals():
        assert f(fake, None, None, 0, ctypes.byref(lst), ctypes.byref(codec) if codec else None, ctypes.byref(proj), *tail) == -4, what
        assert b"kx_run_batch_field_project" in err() and what in err(), (what, err())
    g = lib.kx_run_records_fd_field_project
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(host.KxRecordsOpts), ctypes.POINTER(host.KxFieldRange), ctypes.c_uint32,
                  ctypes.c_uint8, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    o = host.KxRecordsOpts(size=ctypes.sizeof(host.KxRecordsOpts), mode=host.KX_RECORDS_QUOTED, sep=10, quote=34, escape=-1)
    items = (host.KxFieldRange * 16)()
    items[0].lo, items[0].hi, items[1].lo, items[1].hi = 4, 4, 2, 0
    for n, fs, ofs, flags, what in ((0, 59, b";", 0, b"1 to 16 items"), (17, 59, b";", 0, b"1 to 16 items"), (2, 59, b"123456789", 0, b"at most 8 bytes"),
                                    (2, 59, b";", 4, b"unknown flag"), (2, 10, b";", 0, b"field separator cannot be the record separator"),
                                    (2, 34, b";", 0, b"field separator cannot be the quote"), (2, 59, b", ", 2, b"exactly one byte"),
                                    (2, 59, b"\n", 2, b"cannot be the record separator"), (2, 59, b'"', 2, b"cannot be the quote"),
                                    (2, 0, b"\t", 3, b"cannot be the tab")):
        assert g(fake, 0, 1, ctypes.byref(o), items, n, fs, ofs, len(ofs), flags, -1, None) == -4, what
        assert b"kx_run_records_fd_field_project" in err() and what in err(), (what, err())
    o.mode, o.quote = host.KX_RECORDS_BYTE, -1
    assert g(fake, 0, 1, ctypes.byref(o), items, 2, 59, b";", 1, 2, -1, None) == -4 and b"values need a quote or an escape" in err()


# ---------------------------------------------------------------------------------------------------------- the lane bodies
def test_lane_bodies_against_a_plain_reference_under_a_sanitizer(tmp_path):
    """tests/native/project_lanes.cpp: k_fpsplen's and k_fpsplice's lane bodies (kx_field_lanes.h, the text the GPU runs) one lane at
    a time over random records, in a stand-alone program built with AddressSanitizer and UBSan (a CPU machine's job: skipped where
    a GPU is present)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = str(tmp_path / "project_lanes")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "native", "project_lanes.cpp")], check=True)
    r = subprocess.run([exe, "60000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"60000 cases" in r.stdout, (r.stdout[-400:], r.stderr[-3000:])
