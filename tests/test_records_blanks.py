"""CPU: field mode on words (`BIN --records … --field=K|LIST --blanks [--unquote]`, kx_run_batch_field_words,
kx_run_records_fd_field_words) — the normative model host.blank_field_list_records_model against Python's own bytes.split() and
against a second restatement, the fields found, the command line's refusals on the produced binary, the Python binding's argument
checks and the C entry points' refusals before any device work.  Nothing here needs a device."""
import ctypes
import itertools
import os
import random
import re
import subprocess

import pytest

from kleenexlang_amd import build, host, program_path

INC = os.path.join(build.ROOT, "include")
model = host.blank_field_list_records_model
ALL = [(1, None)]


def _words_of(bodies, quote=None, escape=None):
    """Per body, (its words as the model has them under the list 1-, the gaps around them); ([], None) for a body without any.
    One call of the model for all of them, each body a record of its own without a separator."""
    data, offs = host.pack_batch(bodies)
    res = []
    for body, m in zip(bodies, model(data, offs, 0, False, ALL, quote, escape)):
        if isinstance(m, int):
            assert m == 0
            res.append(([], None))
            continue
        gaps, fields, sep = m
        assert sep == b"" and [K for K, _ in fields] == list(range(1, len(fields) + 1))
        assert b"".join(g + f for g, (_, f) in zip(gaps, fields + [(0, b"")])) == body      # every byte is in a gap or in a word
        res.append(([f for _, f in fields], gaps))
    return res


def _words(body, quote=None, escape=None):
    return _words_of([body], quote, escape)[0]


# ---------------------------------------------------------------------------------------------------------- PLAIN: Python itself
def test_plain_words_are_bytes_split_exhaustively():
    bodies = [bytes(t) for L in range(10) for t in itertools.product(b"a \t", repeat=L)]
    assert len(bodies) == (3 ** 10 - 1) // 2
    for body, (words, gaps) in zip(bodies, _words_of(bodies)):
        assert words == body.split(), body
        if gaps is not None:
            assert all(g.strip(b" \t") == b"" for g in gaps) and all(gaps[1:-1]), body        # the gaps are blanks; the inner ones not empty


def test_plain_words_are_bytes_split_on_long_random_bodies():
    r = random.Random(7)
    alphabet = bytes(b for b in range(256) if b not in b"\n\r\x0b\x0c")                   # (bytes.split() takes those four for blanks too)
    for _ in range(400):
        L = r.randrange(10, 400)
        body = bytes(r.choice(b" \t  ") if r.randrange(3) == 0 else r.choice(alphabet) for _ in range(L))
        assert _words(body)[0] == body.split()
    assert _words(b"a\x1c\x1d\x1e\x1f\x85\xa0b")[0] == [b"a\x1c\x1d\x1e\x1f\x85\xa0b"]      # (str.split()'s extra blanks are none here)


# ---------------------------------------------------------------------------------------------------------- QUOTED, ESCAPED
def _second(body, quote, escape):
    """A restatement written differently: first the positions of the live blanks, as a set; then the slices between them."""
    q = quote[0] if quote else None
    e = escape[0] if escape else None
    live, k, inside = set(), 0, False
    while k < len(body):
        b = body[k]
        if e is not None and b == e:
            k += 2                                                                       # the byte behind it is only data
            continue
        if q is not None and b == q:
            inside = not inside
        elif b in (0x20, 0x09) and not inside:
            live.add(k)
        k += 1
    words, k = [], 0
    while k < len(body):
        if k in live:
            k += 1
            continue
        j = k
        while j < len(body) and j not in live:
            j += 1
        words.append(body[k:j])
        k = j
    return words


MODES = [(b'"', None), (None, b"\\"), (b'"', b"\\")]
HAND = [(b'a "b  c" d', b'"', None, [b"a", b'"b  c"', b"d"]),
        (b"a\\ b c", None, b"\\", [b"a\\ b", b"c"]),
        (b'"a\\" b" c', b'"', b"\\", [b'"a\\" b"', b"c"]),
        (b'"a\\" b" c', b'"', None, [b'"a\\"', b'b" c']),                                  # (without the escape the second quote closes)
        (b'a "b c', b'"', None, [b"a", b'"b c']),                                          # an unbalanced quote: the rest is one word
        (b'a "b c', b'"', b"\\", [b"a", b'"b c']),
        (b"a b\\", None, b"\\", [b"a", b"b\\"]),                                           # a trailing escape
        (b"a b \\", b'"', b"\\", [b"a", b"b", b"\\"]),
        (b"a\\", None, b"\\", [b"a\\"]),
        (b'"GET / HTTP/1.0" 200', b'"', None, [b'"GET / HTTP/1.0"', b"200"]),
        (b' "" \t"" ', b'"', None, [b'""', b'""']),
        (b"\\ ", None, b"\\", [b"\\ "]),                                                   # an escaped blank alone is a word
        (b'" "', b'"', None, [b'" "'])]


@pytest.mark.parametrize("body,quote,escape,want", HAND)
def test_hand_cases(body, quote, escape, want):
    assert _words(body, quote, escape)[0] == want == _second(body, quote, escape)


@pytest.mark.parametrize("quote,escape", MODES)
def test_quoted_and_escaped_against_the_second_restatement(quote, escape):
    r = random.Random(len(quote or b"") + 2 * len(escape or b""))
    bodies = [bytes(t) for L in range(8) for t in itertools.product(b'a "\\', repeat=L)]
    assert len(bodies) == (4 ** 8 - 1) // 3
    bodies += [bytes(r.choice(b'ab \t"\\') for _ in range(r.randrange(8, 60))) for _ in range(300)]
    differs = 0
    for body, (got, _) in zip(bodies, _words_of(bodies, quote, escape)):
        assert got == _second(body, quote, escape), body
        differs += got != body.split()
    assert differs > 100                                                                  # the quote and the escape decide


# ---------------------------------------------------------------------------------------------------------- fields found, lists
def test_fields_found_may_be_zero():
    for body in (b"", b" ", b" \t "):
        assert model(body, [0, len(body)], 0, False, [1]) == [0]
        assert model(body + b"\n", [0, len(body) + 1], 1, False, [(2, None)]) == [0]
        assert model(body, [0, len(body)], 0, False, [1], b'"', b"\\") == [0]
    for text, first in (("1", 1), ("2,4-", 2), ("3-3", 3), ("5-", 5), ("7,9-12", 7)):
        assert host.field_list_missing(host.parse_field_list(text), 0) == first
    assert model(b"a b", [0, 3], 0, False, host.parse_field_list("2,4-")) == [2]
    assert host.field_list_missing(host.parse_field_list("2,4-"), 2) == 4
    assert model(b'" "', [0, 3], 0, False, [1], b'"') == [([b"", b""], [(1, b'" "')], b"")]   # (a quoted blank is no blank: one word)


def test_records_bodies_and_separators():
    data = b"  a   abba\tb \n\n \t\r\nlast  one"
    offs = [0, 14, 15, 19, 28]
    got = model(data, offs, 1, True, [2])
    assert got[0] == ([b"  a   ", b"\tb "], [(2, b"abba")], b"\n")
    assert got[1] == 0 and got[2] == 1                                                     # the empty body; "\r" is no blank: one word
    assert got[3] == ([b"last  ", b""], [(2, b"one")], b"")                                # the tail whole: no separator
    assert model(b" \t\r\n", [0, 4], 2, False, [1]) == [0]                                  # (with the two-byte separator that body is blanks)
    assert model(data[:-1], offs[:-1] + [27], 1, False, [2])[3] == ([b"last  ", b""], [(2, b"o")], b"n")
    assert model(b"a b", [0, 3], 0, False, host.parse_field_list("1,3-4")) == [2]           # need = 4
    assert model(b" a b  c d e ", [0, 12], 0, False, host.parse_field_list("1,3-4,6-")) == [5]   # (need is the open range's 6)
    gaps, fields, _ = model(b" a b  c d e ", [0, 12], 0, False, host.parse_field_list("1,3-4"))[0]
    assert fields == [(1, b"a"), (3, b"c"), (4, b"d")] and gaps == [b" ", b" b  ", b" ", b" e "]
    gaps, fields, _ = model(b" a b  c d e f", [0, 13], 0, False, host.parse_field_list("1,3-4,6-"))[0]
    assert fields == [(1, b"a"), (3, b"c"), (4, b"d"), (6, b"f")] and gaps == [b" ", b" b  ", b" ", b" e ", b""]


@pytest.mark.parametrize("quote,escape", [(None, None)] + MODES)
def test_a_one_number_list_is_a_slice_of_the_open_list(quote, escape):
    r = random.Random(3)
    for _ in range(200):
        body = bytes(r.choice(b'ab \t"\\' if quote or escape else b"ab \t") for _ in range(r.randrange(0, 40)))
        words, gaps = _words(body, quote, escape)
        for m in range(1, 6):
            one = model(body, [0, len(body)], 0, False, [m], quote, escape)[0]
            tail = model(body, [0, len(body)], 0, False, [(m, None)], quote, escape)[0]
            if len(words) < m:
                assert one == tail == len(words)
                continue
            assert tail[1] == [(m + k, w) for k, w in enumerate(words[m - 1:])]
            (g0, g1), [(K, w)], _ = one
            assert (K, w) == tail[1][0] and g0 == tail[0][0] and g0 + w + g1 == body


def test_model_argument_checks():
    for kw, exc, what in ((dict(quote=b" "), ValueError, "quote"), (dict(quote=b"\t"), ValueError, "quote"), (dict(escape=b" "), ValueError, "escape"),
                          (dict(quote=b'"', escape=b'"'), ValueError, "escape"), (dict(quote=b"ab"), ValueError, "quote")):
        with pytest.raises(exc, match=what):
            model(b"a b", [0, 3], 0, False, [1], **kw)
    with pytest.raises(TypeError, match="bytes"):
        model("a b", [0, 3], 0, False, [1])
    with pytest.raises(TypeError, match="last_whole"):
        model(b"a b", [0, 3], 0, 1, [1])
    with pytest.raises(ValueError, match="shorter"):
        model(b"a\n\n", [0, 2, 3], 2, False, [1])
    with pytest.raises(ValueError, match="field"):
        model(b"a b", [0, 3], 0, False, [0])


# ---------------------------------------------------------------------------------------------------------- Python argument checks
def test_python_argument_errors_before_any_device():
    import torch
    prog = host.Program.__new__(host.Program)     # (no engine handle: anything that reached the device would fail differently)
    v, o = torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 2, 4])
    for ranges, kw, exc, what in (([0], {}, ValueError, "field"), ("2,3", {}, TypeError, "fields"), ([1], {"quote": b" "}, ValueError, "quote"),
                                  ([1], {"escape": b"\t"}, ValueError, "escape"), ([1], {"quote": b'"', "escape": b'"'}, ValueError, "escape"),
                                  ([1], {"unquote": True}, ValueError, "quote= or an escape="), ([1], {"unquote": 1}, TypeError, "unquote"),
                                  ([1], {"unquote": True, "quote": b'"', "special": b"\n "}, ValueError, "special"),
                                  ([1], {"unquote": True, "quote": b'"', "special": b"12345678"}, ValueError, "special"),
                                  ([1], {"unquote": True, "quote": b'"', "special": b'"'}, ValueError, "special"),
                                  ([1], {"sep_len": 9}, ValueError, "sep_len"), ([1], {"last_whole": 1}, TypeError, "last_whole"),
                                  ([1], {"keep_sep": 1}, TypeError, "keep_sep"), ([1], {"suffix": b"123456789"}, ValueError, "suffix")):
        with pytest.raises(exc, match=what):
            prog.run_batch_field_words_tensor(v, o, ranges, **kw)
    with pytest.raises(TypeError):
        prog.run_batch_field_words_tensor(v, o, [1], fs=b" ")                               # there is no fs= here
    with pytest.raises(host.EngineError, match="HIP device"):
        prog.run_batch_field_words_tensor(v, o, host.parse_field_list("2,4-"))
    with pytest.raises(host.EngineError, match="HIP device"):
        prog.run_batch_field_words_tensor(v, o, [2], quote=b'"', unquote=True, special=b"\n\r")
    for call in (lambda **kw: prog.run_records(b"a b\n", **kw), lambda **kw: prog.run_records_fd(0, 1, **kw)):
        with pytest.raises(ValueError, match="blanks= cannot be combined with fs="):
            call(field=2, fs=b" ", blanks=True)
        with pytest.raises(ValueError, match="blanks= cannot be combined with fs="):
            call(fields=[2], fs=b"\t", blanks=True)                                         # also the default's value, spelled out
        with pytest.raises(ValueError, match="blanks= needs field"):
            call(blanks=True)
        with pytest.raises(TypeError, match="blanks"):
            call(field=2, blanks=1)
        with pytest.raises(ValueError, match="quote character.*blank"):
            call(field=2, blanks=True, quote=b" ")
        with pytest.raises(ValueError, match="escape character.*blank"):
            call(field=2, blanks=True, escape=b"\t")
        with pytest.raises(ValueError, match="record separator.*blank"):
            call(field=2, blanks=True, sep=b" ")
        with pytest.raises(ValueError, match="record separator.*blank"):
            call(fields=[2], blanks=True, rs=b"\t")
        with pytest.raises(ValueError, match="unquote= needs quote= or escape="):
            call(field=2, blanks=True, unquote=True)
        with pytest.raises(ValueError, match="exclude"):
            call(field=1, fields=[2], blanks=True)
        with pytest.raises(ValueError, match="record separator"):                          # without blanks= the fs rules are what they were
            call(fields=[1, 3], fs=b"\n")
        with pytest.raises(ValueError, match="record separator"):
            call(field=1, sep=b"\t")                                                        # (the default fs is still a tab)


# ---------------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def flip_bin(tmp_path_factory):
    exe = tmp_path_factory.mktemp("recblanks") / "flip"
    r = subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", str(exe)], timeout=300)
    assert r.returncode == 0
    return str(exe)


def _run(exe, *args):
    """The binary with an engine library that cannot load: an argument that passes parsing ends at the load."""
    return subprocess.run([exe, *args], input=b"ab\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60,
                          env=dict(os.environ, KXHIP_LIB="/nonexistent/libkxhip.so"))


@pytest.mark.parametrize("args", [
    ["--records", "--blanks"], ["--blanks"], ["--records", "--chomp", "--blanks"],                                   # without --field
    ["--records", "--field=2", "--blanks", "--fs= "], ["--records", "--field=2,4", "--fs=,", "--blanks"],           # together with --fs
    ["--records", "--field=2", "--blanks", "--fs=\\t"],
    ["--records= ", "--field=2", "--blanks"], ["--records=\\t", "--field=1-", "--blanks"],                           # a blank record separator
    ["--records=\\x20", "--field=2", "--blanks"], ["--records", "--rs= ", "--field=2", "--blanks"],
    ["--records", "--rs=\\t", "--field=2", "--blanks"],
    ["--records", "--quote= ", "--field=2", "--blanks"], ["--records", "--quote=\\t", "--field=2", "--blanks", "--unquote"],   # a blank quote
    ["--records", "--escape= ", "--field=2", "--blanks"], ["--records", "--quote", "--escape=\\t", "--field=2", "--blanks"]])   # a blank escape
def test_refusals_name_blanks_before_loading(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
    assert b"--blanks" in r.stderr and b"cannot load" not in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("args", [
    ["--records", "--field=2", "--blanks"], ["--records", "--field=2,4-", "--blanks"], ["--records", "--blanks", "--field", "1-"],
    ["--records", "--rs= \\n", "--field=2", "--blanks"], ["--records", "--rs=\\t\\t", "--field=2", "--blanks"],       # a byte of a multi-byte --rs may be a blank
    ["--records=;", "--quote", "--escape", "--chomp", "--ors=\\n", "--field=6", "--blanks", "--unquote"],
    ["--records", "--escape", "--field=1,3", "--blanks", "--unquote"]])
def test_good_command_lines_reach_the_engine(flip_bin, args):
    r = _run(flip_bin, *args)
    assert r.returncode == 1 and b"cannot load the HIP engine" in r.stderr and r.stdout == b"", (args, r.stderr)


def test_the_other_refusals_and_the_usage(flip_bin):
    r = _run(flip_bin, "--records", "--field=2", "--blanks", "--unquote")
    assert r.returncode == 2 and b"--unquote needs --quote or --escape" in r.stderr
    r = _run(flip_bin, "--field=2", "--blanks")
    assert r.returncode == 2 and b"--field needs --records" in r.stderr
    r = _run(flip_bin, "--records", "--field=0", "--blanks")
    assert r.returncode == 2 and b"--field" in r.stderr
    r = _run(flip_bin, "--records=\\t", "--field=2")                                          # without --blanks: what it printed
    assert r.returncode == 2 and r.stderr.endswith(b"--fs cannot be the record separator\n")
    r = _run(flip_bin, "-h")
    assert r.returncode == 1 and b"--field=K|LIST --blanks [--unquote]\"" in r.stdout
    assert b"--field=K [--fs=F]\": runs field K (from 1; fields end at F, default a tab) of every record, the rest is copied.\n" in r.stdout


# ---------------------------------------------------------------------------------------------------------- the C entry points
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "kxhip.h")).read(), flags=re.S)


def test_abi_is_declared_and_exported():
    txt = _header()
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    for name in ("kx_run_batch_field_words", "kx_run_records_fd_field_words"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(r"int\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]   # noqa: E731
    assert args("kx_run_batch_field_words") == ["prog", "d_in", "d_in_off", "n_docs", "list", "codec", "d_out", "cap", "d_out_off", "d_docs",
                                                "d_fail_field", "out_len", "stats", "stream"] == args("kx_run_batch_field_values")
    assert args("kx_run_records_fd_field_words") == ["p", "in_fd", "out_fd", "o", "ranges", "n_ranges", "unquote", "report_fd", "stats"]
    # the structs keep their layout
    assert ctypes.sizeof(host.KxBatchFieldList) == 124 and ctypes.sizeof(host.KxFieldCodec) == 32 and ctypes.sizeof(host.KxRecordsOpts) == 64


def _list(ranges, n=None, **kw):
    kw = dict(dict(size=ctypes.sizeof(host.KxBatchFieldList), fs=0, quote=-1, escape=-1, sep_len=1, keep_sep=1), **kw)
    spec = host.KxBatchFieldList(n_ranges=len(ranges) if n is None else n, **kw)
    for j, (lo, hi) in enumerate(ranges):
        spec.ranges[j].lo, spec.ranges[j].hi = lo, hi
    return spec


def _codec(special=b"\n", **kw):
    c = host.KxFieldCodec(**dict(dict(size=ctypes.sizeof(host.KxFieldCodec), n_special=len(special)), **kw))
    c.special[:len(special)] = special
    return c


def test_abi_refusals_before_any_device():
    lib = ctypes.CDLL(os.path.join(build.OUT, "libkxhip.so"))
    lib.kx_last_error.restype = ctypes.c_char_p
    f = lib.kx_run_batch_field_words
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.POINTER(host.KxBatchFieldList), ctypes.POINTER(host.KxFieldCodec), ctypes.c_void_p,
                                          ctypes.c_size_t] + [ctypes.c_void_p] * 6
    ol = ctypes.c_size_t()
    tail = (None, 0, None, None, None, ctypes.cast(ctypes.byref(ol), ctypes.c_void_p), None, None)
    good = [(2, 2), (4, 0)]
    assert f(None, None, None, 0, ctypes.byref(_list(good)), None, *tail) == -4             # a null program
    # (a program handle that is no program: a call that got past the checks would read it and crash, not return -4)
    fake = ctypes.c_void_p(16)
    assert f(fake, None, None, 0, None, None, *tail) == -4                                  # a null list
    err = lib.kx_last_error
    for kw, what in ((dict(fs=32), b"fs must be 0"), (dict(fs=9), b"fs must be 0"), (dict(fs=59), b"fs must be 0"),
                     (dict(quote=32), b"quote byte cannot be a blank"), (dict(quote=9), b"quote byte cannot be a blank"),
                     (dict(quote=34, escape=32), b"escape byte cannot be a blank"), (dict(escape=9), b"escape byte cannot be a blank"),
                     (dict(size=120), b"size"), (dict(size=0), b"size"), (dict(quote=34, escape=34), b"escape byte cannot be the quote"),
                     (dict(quote=256), b"quote"), (dict(escape=-2), b"escape"), (dict(sep_len=9), b"separator"), (dict(suffix_len=9), b"suffix")):
        for codec in (None, ctypes.byref(_codec())):
            assert f(fake, None, None, 0, ctypes.byref(_list(good, **kw)), codec, *tail) == -4, kw
            assert b"kx_run_batch_field_words" in err() and what in err(), (kw, err())
    for ranges in ([(0, 2)], [(3, 2)], [(2, 3), (4, 5)], [(2, 0), (5, 6)]):
        assert f(fake, None, None, 0, ctypes.byref(_list(ranges)), None, *tail) == -4 and b"normal form" in err(), ranges
    for n in (0, 9):
        assert f(fake, None, None, 0, ctypes.byref(_list(good, n=n)), None, *tail) == -4 and b"1 to 8 ranges" in err()
    for k in range(4):
        o = _list(good)
        o.reserved[k] = 1
        assert f(fake, None, None, 0, ctypes.byref(o), None, *tail) == -4 and b"reserved" in err()
    q = dict(quote=34)
    for codec, what in ((_codec(b"\n "), b"special byte cannot be a blank"), (_codec(b"\t"), b"special byte cannot be a blank"),
                        (_codec(b"12345678"), b"at most 7 special"), (_codec(n_special=9), b"at most 7 special"),
                        (_codec(size=28), b"kx_field_codec::size"), (_codec(b'\n"'), b"cannot be the quote or the escape")):
        assert f(fake, None, None, 0, ctypes.byref(_list(good, **q)), ctypes.byref(codec), *tail) == -4, what
        assert b"kx_run_batch_field_words" in err() and what in err(), (what, err())
    c = _codec()
    c.reserved[2] = 1
    assert f(fake, None, None, 0, ctypes.byref(_list(good, **q)), ctypes.byref(c), *tail) == -4 and b"reserved" in err()
    assert f(fake, None, None, 0, ctypes.byref(_list(good)), ctypes.byref(_codec()), *tail) == -4 and b"need a quote or an escape" in err()
    # the records entry point
    g = lib.kx_run_records_fd_field_words
    g.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(host.KxRecordsOpts), ctypes.POINTER(host.KxFieldRange), ctypes.c_uint32,
                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    osz = ctypes.sizeof(host.KxRecordsOpts)
    ro = dict(size=osz, mode=host.KX_RECORDS_BYTE, sep=10, quote=-1, escape=-1)
    arr = lambda ranges: _list(ranges).ranges                                               # noqa: E731
    opts = lambda **kw: ctypes.byref(host.KxRecordsOpts(**dict(ro, **kw)))                    # noqa: E731
    assert g(None, 0, 1, None, arr(good), 2, 0, -1, None) == -4
    assert g(None, 0, 1, opts(), None, 2, 0, -1, None) == -4
    assert g(None, 0, 1, opts(), arr([(2, 3), (4, 5)]), 2, 0, -1, None) == -4 and b"normal form" in err()
    rs1 = lambda b: dict(mode=host.KX_RECORDS_RS, rs=(ctypes.c_uint8 * 8)(b), rs_len=1)      # noqa: E731
    for kw, what in ((dict(sep=32), b"record separator cannot be a blank"), (dict(sep=9), b"record separator cannot be a blank"),
                     (rs1(32), b"record separator cannot be a blank"), (rs1(9), b"record separator cannot be a blank"),
                     (dict(mode=host.KX_RECORDS_QUOTED, quote=32), b"quote byte cannot be a blank"),
                     (dict(mode=host.KX_RECORDS_ESCAPED, quote=34, escape=9), b"escape byte cannot be a blank"),
                     (dict(mode=host.KX_RECORDS_ESCAPED, quote=9, escape=92), b"quote byte cannot be a blank"),
                     (dict(size=osz - 4), b"size"), (dict(chomp=2), b"chomp")):
        assert g(None, 0, 1, opts(**kw), arr(good), 2, 0, -1, None) == -4, kw
        assert b"kx_run_records_fd_field_words" in err() and what in err(), (kw, err())
    assert g(None, 0, 1, opts(), arr(good), 2, 1, -1, None) == -4 and b"values need a quote or an escape" in err()   # unquote in BYTE mode
    two = dict(mode=host.KX_RECORDS_RS, rs=(ctypes.c_uint8 * 8)(32, 10), rs_len=2)           # a byte of a multi-byte rs may be a blank
    assert g(None, 0, 1, opts(**two), arr(good), 2, 0, -1, None) == -4 and b"null argument" in err()
    assert g(None, 0, 1, opts(), arr(good), 2, 0, -1, None) == -4 and b"null argument" in err()
