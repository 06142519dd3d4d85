"""CPU: header rows (`--header[=N]`) and fields by column name: the parser of lists with names, the normative model of a header
record's cell names against the csv module and str.split, what the binary and the C entry points refuse before the engine does any
work, and the host-only header kx_field_names.h against a plain reference under a sanitizer (tests/native/field_names.cpp)."""
import csv
import ctypes
import io
import os
import random
import re
import subprocess

import pytest

import test_records_project as project
from kleenexlang_amd import build, host, program_path

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(os.path.dirname(HERE), "include")


# ---------------------------------------------------------------------------------------------------------- parse_field_names
@pytest.mark.parametrize("text, want", [
    ("name", (b"name",)), ("id,city", (b"id", b"city")), ("2,name,5-", (2, b"name", (5, None))), ("a\\,b", (b"a,b",)),
    ("\\x2c", (b",",)), ("a\\x2Cb,c", (b"a,b", b"c")), ("user-id", (b"user-id",)), ("3-4,x", ((3, 4), b"x")), ("a\\\\,b", (b"a\\", b"b")),
    ("\\n\\t\\r\\0\\\\", (b"\n\t\r\0\\",)), ("café", ("café".encode(),)), (" id ", (b" id ",)), ("1a,-x,2-y", (b"1a", b"-x", b"2-y")),
    ("x" * 255, (b"x" * 255,)), (",".join(["n"] * 16), (b"n",) * 16), ("name,name,1", (b"name", b"name", 1))])
def test_parse_field_names_keeps_the_text(text, want):
    assert host.parse_field_names(text) == want


@pytest.mark.parametrize("text", ["a,,b", "a,", ",a", "", "x" * 256, ",".join(["n"] * 17), ",".join(["1"] * 17), "a\\q", "a\\", "a\\x4", "a\\xg0",
                                  "a,0", "a,5-2", "a,-3", "a,1-2-3", "a,4294967296", "\\,,", ",".join(str(2 * k) for k in range(1, 10))])
def test_parse_field_names_refuses(text):
    with pytest.raises(ValueError):
        host.parse_field_names(text)


@pytest.mark.parametrize("text", ["4,2", "2,1,2", "3-,1-2", "7", "1-", "6-,3-4,1", "5-9,5-9", "4294967295,1"])
def test_number_items_are_parse_field_orders(text):
    got = host.parse_field_names(text)
    assert all(not isinstance(it, bytes) for it in got)
    assert host._check_field_items(list(got)) == (host.parse_field_order(text), host.parse_field_list(text))
    with pytest.raises(TypeError):
        host.parse_field_names(text.encode())


@pytest.mark.parametrize("text", ["-3", "5-2", "0", "2,,3", "2,", "1-2-3", "4294967296", "01234567890"])
def test_number_items_keep_their_refusals(text):
    with pytest.raises(ValueError):
        host.parse_field_order(text)
    with pytest.raises(ValueError):
        host.parse_field_names(text)
    with pytest.raises(ValueError):
        host.parse_field_names("name," + text)


# ---------------------------------------------------------------------------------------------------------- header_names_model
CELL_ALPHABET = ["a", "b", "c", ",", '"', " ", "\\", ";", "é"]


def _rows(seed, n=300):
    rnd = random.Random(seed)
    return [["".join(rnd.choice(CELL_ALPHABET) for _ in range(rnd.randrange(0, 6))) for _ in range(rnd.randrange(1, 9))] for _ in range(n)]


@pytest.mark.parametrize("dialect", ["default", "all", "escape"])
def test_names_are_what_the_csv_module_reads(dialect):
    kw = {"default": {}, "all": dict(quoting=csv.QUOTE_ALL), "escape": dict(escapechar="\\", doublequote=False)}[dialect]
    escape = b"\\" if dialect == "escape" else None
    seen = set()
    for row in _rows(dialect):
        buf = io.StringIO()
        csv.writer(buf, lineterminator="\n", **kw).writerow(row)
        line = buf.getvalue()[:-1]
        want = next(csv.reader([line], **{k: v for k, v in kw.items() if k != "quoting"}))
        assert want == row
        got = host.header_names_model(line.encode(), b",", b'"', escape)
        assert got == [c.encode() for c in want], (line, got)
        seen |= {"quoted"} if '"' in line else set()
        seen |= {"doubled"} if '""' in line.strip('"').replace('","', "") else set()
        seen |= {"escaped"} if "\\" in line else set()
    assert {"quoted", "escaped"} <= seen and (dialect == "escape" or "doubled" in seen)


def test_words_are_what_str_split_gives():
    rnd = random.Random(3)
    for _ in range(300):
        words = [bytes(rnd.choice(b"abc%-1") for _ in range(rnd.randrange(1, 7))) for _ in range(rnd.randrange(0, 12))]
        gap = lambda lo: bytes(rnd.choice(b" \t") for _ in range(rnd.randrange(lo, 4)))   # noqa: E731
        body = gap(0) + b"".join(w + gap(1) for w in words[:-1]) + b"".join(words[-1:]) + gap(0)
        assert host.header_names_model(body, None, blanks=True) == body.split() == words
    assert host.header_names_model(b"USER   PID %CPU\tCOMMAND ", None, blanks=True) == [b"USER", b"PID", b"%CPU", b"COMMAND"]
    assert host.header_names_model(b'a "b c" d', None, b'"', blanks=True) == [b"a", b"b c", b"d"]       # a quoted blank is not live; the name is the value
    assert host.header_names_model(b"", None, blanks=True) == [] and host.header_names_model(b"", b",") == [b""]
    with pytest.raises(ValueError, match="blanks"):
        host.header_names_model(b"a b", b" ", blanks=True)


def test_the_byte_order_mark_duplicates_and_the_resolver():
    bom = b"\xef\xbb\xbf"
    assert host.header_names_model(bom + b"id,name", b",", first=True) == [b"id", b"name"]
    assert host.header_names_model(bom + b"id,name", b",") == [bom + b"id", b"name"]                       # only the stream's first record
    assert host.header_names_model(bom + b'"id",name', b",", b'"', first=True) == [b"id", b"name"]
    assert host.header_names_model(bom + b"id name", None, blanks=True, first=True) == [b"id", b"name"]
    assert host.header_names_model(b"id,name\r", b",") == [b"id", b"name\r"]                               # CRLF is not stripped
    assert host.header_names_model(b'"name",x', b",") == [b'"name"', b"x"]                                 # without a quote byte: the bytes
    assert host.header_names_model(b'"na""me","a,b",x\\,y', b",", b'"', b"\\") == [b'na"me', b"a,b", b"x,y"]
    names = host.header_names_model(b"id,name,city,name,id", b",")
    assert host.resolve_field_names([b"name", 5, b"id", (2, None), b"city", (1, 2)], names) == [2, 5, 1, (2, None), 3, (1, 2)]   # the lowest wins
    with pytest.raises(host.HeaderError) as e:
        host.resolve_field_names([b"id", b"nam"], names)
    assert e.value.name == b"nam" and isinstance(e.value, host.KleenexError)
    with pytest.raises(TypeError):
        host.header_names_model("id,name", b",")
    with pytest.raises(TypeError):
        host.header_names_model(b"id,name", b",", first=1)


def test_the_header_keyword_checks():
    assert host._check_header("t", 0, None) == (0, False) and host._check_header("t", 3, [1, (2, None)]) == (3, False)
    assert host._check_header("t", 1, [b"id", 2]) == (1, True)
    for bad, exc in ((-1, ValueError), (1 << 32, ValueError), (True, TypeError), ("1", TypeError)):
        with pytest.raises(exc):
            host._check_header("t", bad, None)
    for fields, what in (([b"id"], "need header"), ([b""], "1 to 255"), ([b"x" * 256], "1 to 255"), ([b"n"] * 17, "at most 16")):
        with pytest.raises(ValueError, match=what):
            host._check_header("t", 0 if what == "need header" else 1, fields)


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recheader") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


SEVENTEEN = "--field=" + ",".join(["n"] * 17)


@pytest.mark.parametrize("args, what", [
    (["--header"], b"--header needs --records"), (["--header=2", "--field=name"], b"--header needs --records"),
    (["--records", "--header=0"], b"Invalid --header: 0"), (["--records", "--header=x"], b"Invalid --header: x"),
    (["--records", "--header="], b"Invalid --header: "), (["--records", "--header=4294967296"], b"Invalid --header: 4294967296"),
    (["--records", "--header=-1"], b"Invalid --header: -1"),
    (["--records", "--field=abc"], b"Invalid --field: abc (a number from 1 to 4294967295)\n"),
    (["--records", "--field=a,b"], b"Invalid --field: a,b (a number from 1 to 4294967295, or a list such as 2,5-7,9-: a field is a number from 1 to 4294967295)\n"),
    (["--records", "--header", "--field=a\\q"], b"Invalid --field: a\\q"), (["--records", "--field=a\\", "--header"], b"Invalid --field: a\\"),
    (["--records", "--header", "--field=a\\x4"], b"Invalid --field"), (["--records", "--header", "--field=a,,b"], b"Invalid --field: a,,b"),
    (["--records", "--header", "--field=" + "x" * 256], b"at most 255 bytes"), (["--records", "--header", SEVENTEEN], b"more than 16 items"),
    (["--records", SEVENTEEN, "--header", "--only"], b"more than 16 items"),
    (["--records", "--header", "--field=name,0"], b"Invalid --field: name,0"), (["--records", "--header", "--field=5-2,name"], b"A <= B"),
    (["--records", "--header", "--field=0"], b"Invalid --field: 0 (a number from 1 to 4294967295)\n"),
    (["--records", "--header", "--field=2,,3"], b"Invalid --field: 2,,3"),
    (["--records", "--header", "--field=name", "--unquote"], b"--unquote needs --quote or --escape"),
    (["--records", "--header", "--field=name", "--blanks", "--fs=,"], b"--blanks cannot be combined with --fs"),
    (["--records", "--header", "--field=name", "--ofs=,"], b"--ofs needs --only"),
    (["--records", "--quote", "--header", "--field=b,a", "--fs=,", "--unquote", "--only", "--ofs=, "], b"--ofs is exactly one byte")])
def test_refusals_before_loading(flip_bin, args, what):
    r = _run(flip_bin, *args)
    assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
    assert what in r.stderr and b"cannot load" not in r.stderr, (args, r.stderr)
    if what.endswith(b"\n"):
        assert r.stderr == what                                                              # today's exact message


@pytest.mark.parametrize("args", [
    ["--records", "--header"], ["--records", "--header=3"], ["--records", "--header=4294967295", "--chomp", "--ors=\\n"],
    ["--records", "--header", "--field=name", "--fs=,"], ["--records", "--field=name", "--fs=,", "--header"],
    ["--records", "--header", "--field=2"], ["--records", "--header", "--field=2,5-7,9-"], ["--records", "--header", "--field=" + ",".join(["1"] * 17)],
    ["--records", "--quote", "--header", "--field=city,name", "--fs=,", "--unquote", "--only", "--ofs=\\t"],
    ["--records", "--header", "--blanks", "--field=COMMAND"], ["--records", "--header=2", "--field=a\\,b,\\x2c,user-id,3-", "--only"],
    ["--records", "--header", "--field=" + "x" * 255], ["--records", "--header", "--field=" + ",".join(["n"] * 16)],
    ["--records", "--rs=\\r\\n", "--header", "--field=name,1", "--only", "--ofs="], ["--records", "--escape", "--header", "--field=a\\\\,b", "--unquote"]])
def test_good_command_lines_reach_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr and r.stdout == b"", (args, r.stderr)


def test_usage_shows_the_new_line_and_the_old_ones(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--header[=N] [--field=LIST ...]\"" in r.stdout
    for old in (b"--only [--ofs=STR]\"", b"--field=K [--fs=F]\"", b"--blanks [--unquote]\"", b"--records --rs=STR\"", b"Normal usage:"):
        assert old in r.stdout
    assert len(r.stdout.splitlines()) == 16


# ---------------------------------------------------------------------------------------------------------- the C entry points
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def test_abi_is_declared_and_exported():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_run_records_fd_table", "kx_run_batch_field_header"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]   # noqa: E731
    assert args("kx_run_batch_field_header") == ["prog", "d_in", "d_in_off", "n_docs", "list", "codec", "proj", "d_out", "cap", "d_out_off",
                                                 "d_docs", "d_fail_field", "out_len", "stats", "stream"]
    assert args("kx_run_batch_field_header") == args("kx_run_batch_field_project")
    assert args("kx_run_records_fd_table") == ["p", "in_fd", "out_fd", "o", "t", "report_fd", "stats"]
    assert re.search(r"#define\s+KX_E_HEADER\s+\(-6\)", txt) and host.KX_E_HEADER == -6
    for name, value in (("WORDS", 1), ("UNQUOTE", 2), ("ONLY", 4), ("SINGLE", 8)):
        assert re.search(r"#define\s+KX_TABLE_%s\s+%du\b" % (name, value), txt) and getattr(host, "KX_TABLE_" + name) == value
    fields = re.search(r"typedef struct kx_records_table \{(.*?)\} kx_records_table;", txt, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", fields) == [n for n, _ in host.KxRecordsTable._fields_]
    assert ctypes.sizeof(host.KxRecordsTable) == 376 and host.KxRecordsTable.names.offset == 152 and host.KxRecordsTable.ofs.offset == 352
    # the structs that were there keep their sizes
    assert [ctypes.sizeof(c) for c in (host.KxBatchFieldList, host.KxFieldCodec, host.KxRecordsOpts, host.KxFieldProject)] == [124, 32, 64, 168]


def _opts(**kw):
    return host.KxRecordsOpts(**dict(dict(size=ctypes.sizeof(host.KxRecordsOpts), mode=host.KX_RECORDS_BYTE, sep=10, quote=-1, escape=-1), **kw))


def table_refusals():
    """(options, table, a piece of the message) of every call kx_run_records_fd_table refuses with KX_E_ARG"""
    T, W, U, O, S = host.records_table, host.KX_TABLE_WORDS, host.KX_TABLE_UNQUOTE, host.KX_TABLE_ONLY, host.KX_TABLE_SINGLE
    quoted = dict(mode=host.KX_RECORDS_QUOTED, quote=34)

    def edit(t, **kw):
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(t, k)[v[0]] = v[1]
            else:
                setattr(t, k, v)
        return t

    return [
        (_opts(), edit(T(1), size=372), b"kx_records_table::size"), (_opts(), edit(T(0), size=0), b"kx_records_table::size"),
        (_opts(), edit(T(1), pad=(2, 1)), b"reserved words"), (_opts(), edit(T(1), reserved=(3, 1)), b"reserved words"),
        (_opts(), T(1, [2], 16, 59), b"unknown flag"), (_opts(), T(0, [2], 0x80000000, 59), b"unknown flag"),
        (_opts(), T(1, [], W), b"flags need items"),
        (_opts(), T(1, [1] * 17, 0, 59), b"at most 16 items"), (_opts(), edit(T(1, [b"a"], 0, 59), n_names=17), b"at most 16 names"),
        (_opts(), edit(T(1, [b"a"], 0, 59), items=(0, host.KxFieldRange(0, 1))), b"name index"),
        (_opts(), edit(T(1, [b"a"], 0, 59), n_names=0), b"name index"),
        (_opts(), edit(T(1, [b"a"], 0, 59), name_len=(0, 0)), b"1 to 255 bytes"), (_opts(), edit(T(1, [b"a"], 0, 59), name_len=(0, 256)), b"1 to 255 bytes"),
        (_opts(), edit(T(1, [b"a"], 0, 59), names=(0, None)), b"null name pointer"),
        (_opts(), T(0, [b"a"], 0, 59), b"names need header"), (_opts(), T(0, [2, b"a"], O, 59, b";"), b"names need header"),
        (_opts(), T(1, [(5, 2)], 0, 59), b"hi = 0 (open) or hi >= lo"),
        (_opts(), T(1, [2, 3], S, 59), b"KX_TABLE_SINGLE"), (_opts(), T(1, [(2, None)], S, 59), b"KX_TABLE_SINGLE"), (_opts(), T(1, [(2, 3)], S, 59), b"KX_TABLE_SINGLE"),
        (_opts(), T(1, [b"a"], S, 59), b"KX_TABLE_SINGLE"), (_opts(), T(0, [2], S | O, 59, b";"), b"KX_TABLE_SINGLE"), (_opts(), T(1, [2], S | W), b"KX_TABLE_SINGLE"),
        (_opts(), T(1, [2 * k for k in range(1, 10)], 0, 59), b"more than 8 ranges"), (_opts(), T(0, [2 * k for k in range(1, 10)], O, 59, b";"), b"more than 8 ranges"),
        (_opts(), T(1, [2, 4], O, 59, b"123456789"), b"at most 8 bytes"),
        # the refusals of the entry points the flags name
        (_opts(size=60), T(1), b"kx_records_opts::size"), (_opts(mode=7), T(1), b"no such split mode"), (_opts(ors_len=9), T(0), b"at most 8 bytes"),
        (_opts(), T(1, [2], S, 10), b"field separator cannot be the record separator"), (_opts(), T(0, [2, 4], 0, 10), b"field separator cannot be the record separator"),
        (_opts(**quoted), T(1, [b"a"], 0, 34), b"field separator cannot be the quote"),
        (_opts(), T(1, [b"a"], U, 59), b"values need a quote or an escape"), (_opts(), T(0, [2], U | O, 59, b";"), b"values need a quote or an escape"),
        (_opts(sep=32), T(1, [b"a"], W), b"record separator cannot be a blank"), (_opts(quote=9, mode=host.KX_RECORDS_QUOTED), T(0, [2], W), b"quote byte cannot be a blank"),
        (_opts(**quoted), T(1, [b"b", b"a"], U | O, 59, b", "), b"exactly one byte"), (_opts(**quoted), T(1, [2, 1], U | O, 59, b""), b"exactly one byte"),
        (_opts(**quoted), T(1, [2, 1], U | O, 59, b"\n"), b"cannot be the record separator"), (_opts(**quoted), T(1, [2, 1], U | O, 59, b'"'), b"cannot be the quote"),
        (_opts(mode=host.KX_RECORDS_ESCAPED, escape=92), T(1, [2, 1], U | O, 59, b"\\"), b"cannot be the escape"),
        (_opts(**quoted), T(1, [2, 1], U | O | W, 0, b"\t"), b"cannot be the tab")]


def test_table_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    lib.kx_last_error.restype = ctypes.c_char_p
    g = lib.kx_run_records_fd_table
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(host.KxRecordsOpts), ctypes.POINTER(host.KxRecordsTable), ctypes.c_int,
                  ctypes.c_void_p]
    # (a program handle that is no program: a call that got past the checks would read it and crash, not return -4)
    fake = ctypes.c_void_p(16)
    assert g(fake, 0, 1, None, ctypes.byref(host.records_table(1)), -1, None) == -4
    assert g(fake, 0, 1, ctypes.byref(_opts()), None, -1, None) == -4
    for o, t, what in table_refusals():
        assert g(fake, 0, 1, ctypes.byref(o), ctypes.byref(t), -1, None) == -4, what
        assert b"kx_run_records_fd_table" in lib.kx_last_error() and what in lib.kx_last_error(), (what, lib.kx_last_error())


def test_the_header_route_refuses_what_the_projection_refuses():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    lib.kx_last_error.restype = ctypes.c_char_p
    f = lib.kx_run_batch_field_header
    f.argtypes = project.project_entry(lib).argtypes
    ol = ctypes.c_size_t()
    tail = (None, 0, None, None, None, ctypes.cast(ctypes.byref(ol), ctypes.c_void_p), None, None)
    fake = ctypes.c_void_p(16)
    assert f(fake, None, None, 0, ctypes.byref(project.spec_list([(2, 2)])), None, None, *tail) == -4
    assert f(fake, None, None, 0, None, None, ctypes.byref(project.spec_proj([(2, 2)])), *tail) == -4
    for lst, codec, proj, what in project.abi_refusals():
        assert f(fake, None, None, 0, ctypes.byref(lst), ctypes.byref(codec) if codec else None, ctypes.byref(proj), *tail) == -4, what
        assert b"kx_run_batch_field_header" in lib.kx_last_error() and what in lib.kx_last_error(), (what, lib.kx_last_error())


# ---------------------------------------------------------------------------------------------------------- kx_field_names.h
def test_field_names_header_against_a_plain_reference_under_a_sanitizer(tmp_path):
    """tests/native/field_names.cpp: the parser, the cell cutter and the resolver of kx_field_names.h (the text kxrun and the engine
    compile) over seeded random headers, in a stand-alone program built with AddressSanitizer and UBSan (a CPU machine's job:
    skipped where a GPU is present).  The program fails if a population — quoted cells, escaped bytes, doubled quotes, duplicate
    names, byte-order marks, missing names, more than 8 ranges — was never drawn."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    exe = str(tmp_path / "field_names")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "native", "field_names.cpp")], check=True)
    r = subprocess.run([exe, "40000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"40000 cases" in r.stdout, (r.stdout[-400:], r.stderr[-3000:])
