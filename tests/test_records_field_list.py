"""CPU: field mode with a list of fields (`BIN --records … --field=LIST --fs=F`, kx_run_batch_field_list,
kx_run_records_fd_field_list) — host.parse_field_list, the normative model field_list_records_model against independent
restatements, the command line's refusals on the produced binary, the Python binding's argument checks and the ABI.  Nothing here
needs a device."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path

INC = os.path.join(build.ROOT, "include")
GOOD_LISTS = ["2,4", "3-", "1,3-4,6-", "2-2", "2,2", "1-", "4-,2,6", "1,3,5,7,9,11,13,15", "1,3,5,7,9,11,13,15-", "4294967295", "1-4294967295",
              "0000000002,3"]
BAD_LISTS = ["", "x", "1x", "0", "4294967296", "-1", "-", "2,", ",2", "2,,3", "3-2", "1-2-3", "2-x", "0-3", "2-0", "1-4294967296", "2 ,3", "2;3",
             "12345678901,2", "2,+3", "1,3,5,7,9,11,13,15,17", "1,3,5,7,9,11,13,15,17-"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


# ---------------------------------------------------------------------------------------------------------- parse_field_list
def test_parse_normal_forms():
    p = host.parse_field_list
    assert p("3") == ((3, 3),) and p("2-2") == ((2, 2),) and p("2,2") == ((2, 2),)
    assert p("3,2") == ((2, 3),) and p("4-,2,6") == ((2, 2), (4, None))                 # the issue's two examples
    assert p("2,4") == ((2, 2), (4, 4)) and p("3-") == ((3, None),) and p("1-") == ((1, None),)
    assert p("1,3-4,6-") == ((1, 1), (3, 4), (6, None))
    assert p("5-7,1-2,3") == ((1, 3), (5, 7)) and p("1-3,2-5,9,8") == ((1, 5), (8, 9))   # adjacent and overlapping ranges merge
    assert p("3-,5-7,9") == ((3, None),) and p("7-,3-") == ((3, None),) and p("1-2,3-") == ((1, None),)
    assert p("4294967295") == ((4294967295, 4294967295),) and p("1-4294967295") == ((1, 4294967295),)   # closed: not the open 1-
    assert p("4294967294,4294967295-") == ((4294967294, None),) and p("5-4294967295,7-") == ((5, None),)
    assert p("0000000002,3") == ((2, 3),)                                              # ten digits at the most, leading zeros among them
    assert p("1,3,5,7,9,11,13,15") == tuple((k, k) for k in range(1, 16, 2))           # 8 ranges: the cap
    assert p("1,3,5,7,9,11,13,15-") [-1] == (15, None)
    assert p(",".join(str(k) for k in range(1, 40))) == ((1, 39),)                     # many items, one range
    for text in GOOD_LISTS:
        assert 1 <= len(p(text)) <= 8


@pytest.mark.parametrize("text", BAD_LISTS)
def test_parse_refusals(text):
    with pytest.raises(ValueError, match="field list|ranges"):
        host.parse_field_list(text)


def test_parse_nine_ranges_and_types():
    with pytest.raises(ValueError, match="9 ranges"):
        host.parse_field_list("1,3,5,7,9,11,13,15,17")
    assert len(host.parse_field_list("1,3,5,7,9,11,13,15,16")) == 8                    # (the ninth item is adjacent to the eighth)
    for bad in (3, b"2,3", None, ["2"]):
        with pytest.raises(TypeError, match="field list"):
            host.parse_field_list(bad)


@pytest.mark.parametrize("text,need,missing", [
    ("2,4", 4, {0: 2, 1: 2, 2: 4, 3: 4}), ("1-3", 3, {0: 1, 1: 2, 2: 3}), ("3-", 3, {1: 3, 2: 3}), ("1-", 1, {0: 1}),
    ("1,3-4,6-", 6, {1: 3, 2: 3, 3: 4, 4: 6, 5: 6}), ("2,5-7", 7, {1: 2, 2: 5, 3: 5, 4: 5, 5: 6, 6: 7})])
def test_need_and_the_missing_field(text, need, missing):
    """`need` is the largest number the list names; K of the no-field line is the smallest member above the fields a record has."""
    r = host.parse_field_list(text)
    assert host.field_list_need(r) == need
    for nf, k in missing.items():
        assert host.field_list_missing(r, nf) == k, (text, nf)
    for nf in range(1, need + 3):                                                      # … and the model agrees, record by record
        body = b",".join(b"f%d" % k for k in range(1, nf + 1))
        got = host.field_list_records_model(body, [0, len(body)], 0, False, r, b",")[0]
        assert (got == nf) if nf < need else ([k for k, _ in got[1]] == [k for lo, hi in r for k in range(lo, (hi or nf) + 1)]), (text, nf, got)


# ---------------------------------------------------------------------------------------------------------- the model
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


def _want(fields, sep, ranges, fs):
    """What the model must say for a body cut into `fields`: from the selected numbers alone."""
    need = max(hi if hi is not None else lo for lo, hi in ranges)
    if len(fields) < need:
        return len(fields)
    sel = [k for k in range(1, len(fields) + 1) if any(lo <= k and (hi is None or k <= hi) for lo, hi in ranges)]
    f, gaps, prev = bytes([fs]), [], 0
    for k in sel:                                                                      # the fields between two selected ones, with every separator
        gaps.append(b"".join(x + f for x in fields[prev:k - 1]) if prev == 0 else f + b"".join(x + f for x in fields[prev:k - 1]))
        prev = k
    gaps.append(b"".join(f + x for x in fields[prev:]))
    return (gaps, [(k, fields[k - 1]) for k in sel], sep)


def _records(r, alphabet, sep, n):
    recs = [b"".join(r.choice(alphabet) for _ in range(r.randrange(0, 14))) for _ in range(n)]
    recs[0], recs[1], recs[n // 2] = b"", b"", b""
    data, offs = host.pack_batch([b + sep for b in recs])
    return recs, data, offs


LISTS = ["2,4", "1-3", "2-", "1,3-4,6-", "1-", "3", "1,3,5,7,9,11,13,15"]


def test_model_edge_cases():
    m, p = host.field_list_records_model, host.parse_field_list
    assert m(b"", [0], 1, False, p("2,4"), b"\t") == []
    assert m(b"\n", [0, 1], 1, False, p("1-"), b",") == [([b"", b""], [(1, b"")], b"\n")]   # the lone separator: one empty field
    assert m(b"\n", [0, 1], 1, False, p("1-2"), b",") == [1]
    assert m(b"a,b,c,d\nx,y\n", [0, 8, 12], 1, False, p("2,4-"), b",") == [([b"a,", b",c,", b""], [(2, b"b"), (4, b"d")], b"\n"), 2]
    assert m(b"a,b,c\n", [0, 6], 1, False, p("1-"), b",") == [([b"", b",", b",", b""], [(1, b"a"), (2, b"b"), (3, b"c")], b"\n")]
    assert m(b"a,b,c", [0, 5], 1, True, p("2-3"), b",") == [([b"a,", b",", b""], [(2, b"b"), (3, b"c")], b"")]     # the tail has no separator
    assert m(b",,\r\n", [0, 4], 2, False, p("1,3"), b",") == [([b"", b",,", b""], [(1, b""), (3, b"")], b"\r\n")]     # empty fields
    assert m(b'a,"b,c",d\n', [0, 10], 1, False, p("2-3"), b",", quote=b'"') == [([b"a,", b",", b""], [(2, b'"b,c"'), (3, b"d")], b"\n")]
    assert m(b'a,"b""c,",d\n', [0, 12], 1, False, p("1,3"), b",", quote=b'"') == [([b"", b',"b""c,",', b""], [(1, b"a"), (3, b"d")], b"\n")]
    assert m(b'"a,b",c\n', [0, 8], 1, False, p("1-2"), b",", quote=b'"') == [([b"", b",", b""], [(1, b'"a,b"'), (2, b"c")], b"\n")]
    assert m(b'"a,b,c\n', [0, 7], 1, False, p("2"), b",", quote=b'"') == [1]                # a stray quote: the rest is one field
    assert m(b"a\\,b,c\n", [0, 7], 1, False, p("1-2"), b",", escape=b"\\") == [([b"", b",", b""], [(1, b"a\\,b"), (2, b"c")], b"\n")]
    assert m(b"xxa,b\nyy", [2, 6], 1, False, [2], b",") == [([b"a,", b""], [(2, b"b")], b"\n")]   # offsets[0] need not be 0; ints are a list
    assert m(b"a,b,c", [0, 5], 0, False, [3, (1, 1)], b",") == [([b"", b",b,", b""], [(1, b"a"), (3, b"c")], b"")]   # … in any order


@pytest.mark.parametrize("sep", [b"\n", b"\r\n"])
def test_model_is_bytes_split(sep):
    """Quote and escape off: the fields are body.split(fs), whatever else a body holds."""
    r = random.Random(len(sep))
    recs, data, offs = _records(r, [b"a", b"\t", b"\t", sep[:1], b'"', b"\\"], sep, 1500)
    for text in LISTS:
        ranges = host.parse_field_list(text)
        for tail in (b"", b"a\tb\t\tc"):
            d, o = data + tail, offs + ([len(data) + len(tail)] if tail else [])
            bodies = recs + ([tail] if tail else [])
            got = host.field_list_records_model(d, o, len(sep), bool(tail), ranges, b"\t")
            assert len(got) == len(bodies)
            for i, (body, g) in enumerate(zip(bodies, got)):
                assert g == _want(body.split(b"\t"), b"" if tail and i == len(recs) else sep, ranges, 9), (text, body, g)
                if isinstance(g, tuple):                                              # the body is the gaps and the fields, interleaved
                    assert b"".join(x + y for x, (_, y) in zip(g[0], g[1] + [(0, b"")])) == body


@pytest.mark.parametrize("quote,escape", [(b'"', None), (None, b"\\"), (b'"', b"\\")])
def test_model_quoted_and_escaped_against_the_loop(quote, escape):
    r = random.Random(7 + (quote is not None) + 2 * (escape is not None))
    alphabet = [b"a", b",", b",", b"\n"] + ([quote] if quote else []) + ([escape] if escape else [])
    recs, data, offs = _records(r, alphabet, b"\n", 1500)
    q, e = quote and quote[0], escape and escape[0]
    seen = set()
    for text in LISTS:
        ranges = host.parse_field_list(text)
        got = host.field_list_records_model(data, offs, 1, False, ranges, b",", quote=quote, escape=escape)
        for body, g in zip(recs, got):
            fields = _loop_fields(body, 0x2C, q, e)
            assert g == _want(fields, b"\n", ranges, 0x2C), (text, body, g)
            seen.add(len(fields) != len(body.split(b",")))
    assert seen == {False, True}                                                        # some separators were not live


@pytest.mark.parametrize("quote,escape", [(None, None), (b'"', None), (b'"', b"\\")])
def test_a_one_number_list_is_the_single_field_model(quote, escape):
    r = random.Random(3)
    alphabet = [b"a", b";", b";", b'"', b"\\", b"\n"]
    recs, data, offs = _records(r, alphabet, b"\n", 800)
    for tail in (False, True):
        for k in range(1, 7):
            one = host.field_records_model(data, offs, 1, tail, k, b";", quote, escape)
            lst = host.field_list_records_model(data, offs, 1, tail, host.parse_field_list("%d" % k), b";", quote, escape)
            for a, b in zip(one, lst):
                assert b == (a if isinstance(a, int) else ([a[0], a[2]], [(k, a[1])], a[3])), (k, a, b)
    assert host.field_list_records_model(data, offs, 1, False, host.parse_field_list("2-2"), b";") == \
        host.field_list_records_model(data, offs, 1, False, [2], b";")


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recfieldlist") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


@pytest.mark.parametrize("text", GOOD_LISTS)
def test_good_lists_reach_the_engine(flip_bin, text):
    for args in (["--records", "--field=" + text], ["--records", "--quote", "--escape", "--chomp", "--ors=\\n", "--fs=,", "--field", text]):
        r = _run(flip_bin, *args)
        assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("text", BAD_LISTS)
def test_bad_lists_are_refused_before_loading(flip_bin, text):
    r = _run(flip_bin, "--records", "--field=" + text)
    assert r.returncode == 2 and r.stdout == b"", (text, r.returncode, r.stderr)
    assert b"--field" in r.stderr and b"cannot load" not in r.stderr, (text, r.stderr)


@pytest.mark.parametrize("args,names", [
    (["--field=2,4"], b"--field"), (["-t", "--field=3-"], b"--field"),                                          # a list without --records
    (["--records", "--field=2,4", "--fs=ab"], b"--fs"), (["--records", "--field=2,4", "--fs=\\n"], b"--fs"),    # the --fs refusals apply unchanged
    (["--records=,", "--field=1-", "--fs=,"], b"--fs"), (["--records", "--rs=\\t", "--field=2,4"], b"--fs"),
    (["--records", "--quote", "--field=2,4", "--fs=\""], b"--fs"), (["--records", "--escape", "--field=3-", "--fs=\\\\"], b"--fs")])
def test_the_existing_refusals_apply_to_lists(flip_bin, args, names):
    r = _run(flip_bin, *args)
    assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
    assert names in r.stderr and b"cannot load" not in r.stderr, (args, r.stderr)


def test_usage_shows_both_lines(flip_bin):
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--field=LIST [--fs=F]\"" in r.stdout
    assert b"--field=K [--fs=F]\": runs field K (from 1; fields end at F, default a tab) of every record, the rest is copied.\n" in r.stdout


# ---------------------------------------------------------------------------------------------------------- Python argument checks
def test_python_argument_errors_before_any_device():
    import torch
    m = host.field_list_records_model
    with pytest.raises(TypeError, match="bytes"):
        m("a\n", [0, 2], 1, False, [1], b",")
    for bad, exc in (("2,3", TypeError), (3, TypeError), (None, TypeError), ([], ValueError), ([0], ValueError), ([1 << 32], ValueError),
                     ([True], TypeError), (["2"], TypeError), ([(3, 2)], ValueError), ([(1, 2, 3)], ValueError), ([(0, 2)], ValueError),
                     ([(None, 2)], TypeError), (list(range(1, 19, 2)), ValueError)):
        with pytest.raises(exc, match="field"):
            m(b"a\n", [0, 2], 1, False, bad, b",")
    for bad, exc in ((b"ab", ValueError), (b"", ValueError), (",", TypeError), (None, TypeError)):
        with pytest.raises(exc, match="field separator"):
            m(b"a\n", [0, 2], 1, False, [1], bad)
    with pytest.raises(ValueError, match="quote"):
        m(b"a\n", [0, 2], 1, False, [1], b",", quote=b",")
    with pytest.raises(ValueError, match="escape"):
        m(b"a\n", [0, 2], 1, False, [1], b",", escape=b",")
    with pytest.raises(ValueError, match="sep_len"):
        m(b"a\n", [0, 2], 9, False, [1], b",")
    with pytest.raises(ValueError, match="shorter"):
        m(b"a\n\n", [0, 2, 3], 2, False, [1], b",")
    with pytest.raises(TypeError, match="last_whole"):
        m(b"a\n", [0, 2], 1, 0, [1], b",")
    with pytest.raises(ValueError, match="offsets"):
        m(b"a\n", [0, 3], 1, False, [1], b",")
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    v, o = torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 2, 4])
    for ranges, kw, exc, what in (([0], {}, ValueError, "field"), ("2,3", {}, TypeError, "fields"), ([], {}, ValueError, "fields"),
                                  (list(range(1, 19, 2)), {}, ValueError, "ranges"), ([(3, 2)], {}, ValueError, "lo <= hi"),
                                  ([1], {"fs": b"ab"}, ValueError, "field separator"), ([1], {"fs": b",", "quote": b","}, ValueError, "quote"),
                                  ([1], {"fs": b",", "escape": b","}, ValueError, "escape"), ([1], {"quote": b'"', "escape": b'"'}, ValueError, "escape"),
                                  ([1], {"sep_len": 9}, ValueError, "sep_len"), ([1], {"last_whole": 1}, TypeError, "last_whole"),
                                  ([1], {"keep_sep": 1}, TypeError, "keep_sep"), ([1], {"suffix": b"123456789"}, ValueError, "suffix"),
                                  ([1], {"suffix": "\n"}, TypeError, "suffix")):
        with pytest.raises(exc, match=what):
            prog.run_batch_field_list_tensor(v, o, ranges, **kw)
    with pytest.raises(host.EngineError, match="HIP device"):
        prog.run_batch_field_list_tensor(v, o, host.parse_field_list("2,4-"))
    for call in (lambda **kw: prog.run_records(b"a\tb\n", **kw), lambda **kw: prog.run_records_fd(0, 1, **kw)):
        with pytest.raises(ValueError, match="exclude"):
            call(field=1, fields=[2])
        with pytest.raises(TypeError, match="fields"):
            call(fields="2,4")
        with pytest.raises(TypeError, match="field"):
            call(field="2,4")                                                         # field= keeps refusing a str
        with pytest.raises(ValueError, match="field"):
            call(fields=[0])
        with pytest.raises(ValueError, match="ranges"):
            call(fields=list(range(1, 19, 2)))
        with pytest.raises(ValueError, match="record separator"):
            call(fields=[1, 3], fs=b"\n")
        with pytest.raises(ValueError, match="record separator"):
            call(fields=[1, 3], fs=b",", rs=b",")
        with pytest.raises(ValueError, match="quote"):
            call(fields=[(2, None)], fs=b'"', quote=b'"')
        with pytest.raises(ValueError, match="escape"):
            call(fields=[(2, None)], fs=b"\\", escape=b"\\")
    e = host.MatchError(5, 1, 3)
    assert (e.pos, e.stage, e.field) == (5, 1, 3) and host.MatchError(5).field is None and str(e) == str(host.MatchError(5))


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_abi_is_declared_and_exported():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_run_batch_field_list", "kx_run_records_fd_field_list"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]
    assert args("kx_run_batch_field_list") == ["prog", "d_in", "d_in_off", "n_docs", "list", "d_out", "cap", "d_out_off", "d_docs", "d_fail_field",
                                               "out_len", "stats", "stream"]
    assert args("kx_run_records_fd_field_list") == ["p", "in_fd", "out_fd", "o", "ranges", "n_ranges", "fs", "report_fd", "stats"]
    spec = re.search(r"typedef struct kx_batch_field_list \{(.*?)\} kx_batch_field_list;", txt, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", spec) == [f for f, _ in host.KxBatchFieldList._fields_]
    assert re.search(r"typedef struct kx_field_range \{\s*uint32_t lo, hi;\s*\} kx_field_range;", txt)
    assert [f for f, _ in host.KxFieldRange._fields_] == ["lo", "hi"] and ctypes.sizeof(host.KxFieldRange) == 8
    assert ctypes.sizeof(host.KxBatchFieldList) == 8 + 64 + 4 + 8 + 16 + 8 + 16 == 124
    assert host.KxBatchFieldList.ranges.offset == 8 and host.KxBatchFieldList.fs.offset == 72 and host.KxBatchFieldList.suffix.offset == 100
    # the structs and entry points that the list leaves alone
    assert ctypes.sizeof(host.KxBatchFields) == 60 and ctypes.sizeof(host.KxRecordsOpts) == 64
    assert ctypes.sizeof(host.KxBatchDoc) == 16 and ctypes.sizeof(host.KxBatchStats) == 5 * 8 + 6 * 4 + 8 + 4 + 4
    batch = ["prog", "d_in", "d_in_off", "n_docs", "d_out", "cap", "d_out_off", "d_docs", "out_len", "stats", "stream"]
    assert args("kx_run_batch_fields") == batch[:4] + ["fields"] + batch[4:]
    assert args("kx_run_records_fd_fields") == ["p", "in_fd", "out_fd", "o", "field", "fs", "report_fd", "stats"]


def _list(ranges, n=None, **kw):
    kw = dict(dict(size=ctypes.sizeof(host.KxBatchFieldList), fs=9, quote=-1, escape=-1, sep_len=1, keep_sep=1), **kw)
    spec = host.KxBatchFieldList(n_ranges=len(ranges) if n is None else n, **kw)
    for j, (lo, hi) in enumerate(ranges):
        spec.ranges[j].lo, spec.ranges[j].hi = lo, hi
    return spec


NOT_NORMAL = [[(0, 2)], [(3, 2)], [(2, 3), (3, 5)], [(2, 3), (4, 5)], [(4, 5), (1, 2)], [(2, 0), (5, 6)], [(2, 0), (5, 0)], [(1, 1), (3, 3), (2, 0)],
              [(4294967295, 4294967295), (1, 0)], [(2, 4), (1, 0)]]


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    lib.kx_last_error.restype = ctypes.c_char_p
    f = lib.kx_run_batch_field_list
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.POINTER(host.KxBatchFieldList), ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 6
    size = ctypes.sizeof(host.KxBatchFieldList)
    ol = ctypes.c_size_t()
    tail = (None, 0, None, None, None, ctypes.cast(ctypes.byref(ol), ctypes.c_void_p), None, None)
    good = [(2, 2), (4, 0)]
    assert f(None, None, None, 0, ctypes.byref(_list(good)), *tail) == -4                  # a null program
    # (a program handle that is no program: a call that got past the checks would read it and crash, not return -4)
    fake = ctypes.c_void_p(16)
    assert f(fake, None, None, 0, None, *tail) == -4                                       # a null list
    for ranges in NOT_NORMAL:
        assert f(fake, None, None, 0, ctypes.byref(_list(ranges)), *tail) == -4, ranges
        assert b"kx_run_batch_field_list" in lib.kx_last_error() and b"normal form" in lib.kx_last_error(), (ranges, lib.kx_last_error())
    for n in (0, 9, 1 << 31):
        assert f(fake, None, None, 0, ctypes.byref(_list(good, n=n)), *tail) == -4 and b"1 to 8 ranges" in lib.kx_last_error()
    bad = [dict(size=size - 4), dict(size=0), dict(size=ctypes.sizeof(host.KxBatchFields)), dict(quote=9), dict(escape=9), dict(quote=34, escape=34),
           dict(quote=256), dict(escape=-2), dict(sep_len=9), dict(suffix_len=9)]
    for kw in bad:
        assert f(fake, None, None, 0, ctypes.byref(_list(good, **kw)), *tail) == -4, kw
        assert b"kx_run_batch_field_list" in lib.kx_last_error()
    for k in range(4):
        o = _list(good)
        o.reserved[k] = 1
        assert f(fake, None, None, 0, ctypes.byref(o), *tail) == -4 and b"reserved" in lib.kx_last_error()
    o = _list(good)
    o.pad[1] = 1
    assert f(fake, None, None, 0, ctypes.byref(o), *tail) == -4 and b"reserved" in lib.kx_last_error()
    g = lib.kx_run_records_fd_field_list
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(host.KxRecordsOpts), ctypes.POINTER(host.KxFieldRange), ctypes.c_uint32,
                  ctypes.c_uint8, ctypes.c_int, ctypes.c_void_p]
    osz = ctypes.sizeof(host.KxRecordsOpts)
    ro = dict(size=osz, mode=host.KX_RECORDS_BYTE, sep=10, quote=-1, escape=-1)
    arr = lambda ranges: _list(ranges).ranges                                               # noqa: E731
    assert g(None, 0, 1, None, arr(good), 2, 9, -1, None) == -4
    assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**ro)), None, 2, 9, -1, None) == -4
    for ranges in NOT_NORMAL:
        assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**ro)), arr(ranges), len(ranges), 9, -1, None) == -4 and b"normal form" in lib.kx_last_error()
    for n in (0, 9):
        assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**ro)), arr(good), n, 9, -1, None) == -4 and b"normal form" in lib.kx_last_error()
    for kw, fs in ((ro, 10), (dict(ro, mode=host.KX_RECORDS_QUOTED, quote=34), 34), (dict(ro, mode=host.KX_RECORDS_ESCAPED, quote=34, escape=92), 92),
                   (dict(ro, size=osz - 4), 9), (dict(ro, chomp=2), 9)):
        assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**kw)), arr(good), 2, fs, -1, None) == -4, (kw, fs)
        assert b"kx_run_records_fd_field_list" in lib.kx_last_error()
    assert g(None, 0, 1, ctypes.byref(host.KxRecordsOpts(**ro)), arr(good), 2, 9, -1, None) == -4 and b"null argument" in lib.kx_last_error()
