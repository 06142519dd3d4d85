"""GPU: header rows and fields by column name — kx_run_batch_field_header (Program.run_batch_field_header_tensor),
Program.run_records(header=, fields=names), kx_run_records_fd_table and `BIN --records --header[=N] --field=LIST`.  A header
record's expected bytes come from the models (host.project_records_model, host.header_names_model); from record N + 1 on the
expectation is the same call with the numbers written out.  The programs, the packers and the bodies are the other field tests',
by import."""
import ctypes
import os
import random

import pytest
from conftest import blob_of

import test_records_field_gpu as single
import test_records_field_list_gpu as lst
import test_records_project_gpu as proj
from kleenexlang_amd import host
from kleenexlang_amd.host import EngineError, HeaderError, MatchError, NoFieldError, Program

pytestmark = pytest.mark.gpu

COPY, FIELDS, WHOLE, FS = single.COPY, single.FIELDS, single.WHOLE, single.FS
O = host.parse_field_order
ITEMS, OFS = proj.ITEMS, proj.OFS


# ---------------------------------------------------------------------------------------------------------- 1. the identity route
def _identity(data, offs, items, ofs, fs=FS, quote=None, escape=None, sep_len=0, last_whole=False, keep_sep=True, suffix=b"", blanks=False,
              unquote=False, special=b"\n"):
    """(output bytes, output offsets, status, fail_pos, fail_stage, fail_field): the model's cells joined here, the identity in the
    program's place; with `unquote` each cell as requote(unquote(cell)) with fs = OFS"""
    ranges = host._check_field_items(items)[1]
    out, ooff, status, fpos, ffield = [], [0], [], [], []
    for m in host.project_records_model(data, offs, sep_len, last_whole, items, None if blanks else fs, quote, escape, blanks=blanks):
        if isinstance(m, int):
            status.append(2); fpos.append(m); ffield.append(host.field_list_missing(ranges, m))
            ooff.append(ooff[-1])
            continue
        cells = [c for _, c in m[0]]
        if unquote:
            sp = special + (b"\t" if blanks else b"")
            cells = [host.requote_field_model(host.unquote_field_model(c, quote, escape), quote is not None and c[:1] == quote, ofs, quote, escape, sp)
                     for c in cells]
        status.append(0); fpos.append(0); ffield.append(0)
        out.append(ofs.join(cells) + (m[1] if keep_sep else b"") + suffix)
        ooff.append(ooff[-1] + len(out[-1]))
    return b"".join(out), ooff, status, fpos, [0] * len(status), ffield


def _check_identity(prog, data, offs, items, ofs, lead=0, **kw):
    import torch
    want = _identity(data, offs, items, ofs, **kw)
    v, o = single._device(data, offs, lead)
    if not kw.get("blanks"):
        kw.setdefault("fs", FS)
    res = prog.run_batch_field_header_tensor(v, o, items, ofs, **kw)
    torch.cuda.synchronize()
    got = (res[0].cpu().numpy().tobytes(),) + tuple(t.tolist() for t in res[1:])
    for name, k in (("status", 2), ("fail_pos", 3), ("fail_stage", 4), ("fail_field", 5), ("out_off", 1)):
        assert got[k] == want[k], (name, items, ofs, lead, kw, next(i for i in range(len(want[k])) if got[k][i] != want[k][i]))
    assert got[0] == want[0], (items, ofs, lead, kw, next((i, data[offs[i]:offs[i + 1]][:80]) for i in range(len(offs) - 1)
                                                          if got[0][want[1][i]:want[1][i + 1]] != want[0][want[1][i]:want[1][i + 1]]))
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.docs_routed, st.docs_replayed, st.out_bytes) == (len(offs) - 1, sum(1 for s in want[2] if s), 0, 0, len(want[0]))
    return want


def _hundred(kind, seed=1):
    """100 bodies with a short record first and last"""
    r = random.Random(seed)
    if kind == "plain":
        mid = lst._bodies(r, "copy", 98)
    elif kind == "quoted":
        mid = lst._liveness_bodies()[:60] + [FS.join(r.choice([b'"a;b"', b'"x""y"', b"k", b"", b'p"q;r"', b'"\n"', b'a\\;b', b'\\"z']) for _ in range(r.randrange(1, 9)))
                                             for _ in range(38)]
    else:
        mid = [b"".join(r.choice([b"w", b"xy", b" ", b"  ", b"\t", b'"a b"', b'""', b"z\\ q", b'k"l m"']) for _ in range(r.randrange(0, 14))) for _ in range(98)]
    return [b"s"] + mid + [b""]


@pytest.mark.parametrize("text", ITEMS)
def test_identity_every_list_with_every_ofs(text):
    prog = Program(blob_of(COPY))
    bodies = _hundred("plain")
    for n, ofs in enumerate(OFS):
        sep_len = (0, 1, 2, 8)[(n + len(text)) % 4]
        data, offs = single._pack(bodies, sep_len)
        want = _check_identity(prog, data, offs, O(text), ofs, lead=(5 * n + len(text)) % 16, sep_len=sep_len, last_whole=bool(n & 1), keep_sep=bool(n & 2),
                               suffix=(b"", b"\n", b"<<eor>>\n")[n % 3])
        if host.field_list_need(host.parse_field_list(text)) > 1:
            assert want[2][0] == 2 and want[2][-1] == 2 and 0 in want[2]                     # short records first and last


@pytest.mark.parametrize("mode", ["plain", "quote", "escape", "quote+escape", "blanks", "blanks+quote", "unquote", "unquote+escape", "blanks+unquote"])
def test_identity_every_mode_separator_length_and_alignment(mode):
    prog = Program(blob_of(COPY))
    blanks, unquote = "blanks" in mode, "unquote" in mode
    quote = b'"' if "quote" in mode else None                                              # (unquote: with a quote)
    escape = b"\\" if "escape" in mode else None
    bodies = _hundred("blanks" if blanks else "plain" if mode == "plain" else "quoted", seed=len(mode))
    kw = dict(quote=quote, escape=escape, blanks=blanks)
    if unquote:
        kw["unquote"] = True
    seen = set()
    for lead in range(16):                                                                 # all 16 input alignments; sep_len 0, 1, 2, 8
        sep_len = (0, 1, 2, 8)[(lead + lead // 4) % 4]
        text = ("2,1", "3-,1", "1-", "2,1,2", "4,2")[lead % 5]
        ofs = b" " if unquote and blanks else b"|" if unquote else OFS[lead % 4]
        data, offs = single._pack(bodies, sep_len)
        want = _check_identity(prog, data, offs, O(text), ofs, lead=lead, sep_len=sep_len, last_whole=bool(lead & 1), keep_sep=not lead & 2,
                               suffix=(b"", b"|", b"12345678")[lead % 3], **kw)
        seen |= {("sep", sep_len), ("status", 0 in want[2]), ("short", 2 in want[2])}
    # (every call has accepted records and, but for 1- on fields that are no words, short ones)
    assert seen - {("short", False)} == {("sep", 0), ("sep", 1), ("sep", 2), ("sep", 8), ("status", True), ("short", True)}


def test_identity_hand_cases():
    prog = Program(blob_of(FIELDS))                                                        # (a program that would reject the digits)
    assert _check_identity(prog, b"id;name;city7\r\n", [0, 15], O("3,1"), b"\t", sep_len=2, keep_sep=False, suffix=b"$")[0] == b"city7\tid$"
    assert _check_identity(prog, b'"a;b";"c""d";e\n', [0, 15], O("2,1"), b",", quote=b'"', sep_len=1)[0] == b'"c""d","a;b"\n'
    assert _check_identity(prog, b'"a;b";"c""d";e\n', [0, 15], O("3,2,1"), b",", quote=b'"', unquote=True, sep_len=1)[0] == b'e,"c""d","a;b"\n'
    assert _check_identity(prog, b"a;b\n", [0, 4], O("3,1"), b",", sep_len=1)[2:] == ([2], [2], [0], [3])
    assert _check_identity(prog, b"", [0], O("2"), b",")[1] == [0]


# ---------------------------------------------------------------------------------------------------------- 2. equivalence
def _norm(res):
    return [("nofield", g.fields) if isinstance(g, NoFieldError) else (g.pos, g.stage, g.field) if isinstance(g, MatchError) else g for g in res]


def _header_model(data, offs, n, tail, sep_len, items=None, ofs=None, chomp=False, ors=b"", fs=FS, quote=None, escape=None, blanks=False,
                  unquote=False, special=b"\n"):
    """the entries of the first n records as header records: copied, or with `items` projected by the identity"""
    n = min(n, len(offs) - 1)
    last_whole = tail and n == len(offs) - 1
    if items is None:
        out = []
        for i in range(n):
            cut = 0 if tail and i == len(offs) - 2 else sep_len
            out.append(data[offs[i]:offs[i + 1] - cut] + (b"" if chomp else data[offs[i + 1] - cut:offs[i + 1]]) + ors)
        return out
    want = _identity(data[:offs[n]], offs[:n + 1], items, ofs, fs, quote, escape, sep_len, last_whole, not chomp, ors, blanks, unquote, special)
    return [want[0][want[1][i]:want[1][i + 1]] if want[2][i] == 0 else ("nofield", want[3][i]) for i in range(n)]


NAMES = [b"id", b"name", b"city", b"name", b"k5", b"zip code", b"k7", b"k8", b"k9"]      # (a duplicate: the lowest wins)


@pytest.mark.parametrize("N", [1, 2, 3])
def test_names_resolve_to_the_numeric_call(N):
    prog = Program(blob_of(FIELDS))
    r = random.Random(N)
    rows = [b"# a comment", b"x;y"][:N - 1] + [FS.join(NAMES)] + lst._bodies(r, "fields", 200)
    data = b"".join(b + b"\n" for b in rows)
    offs = list(host.split_records_model(data, b"\n"))
    seen = set()
    for named, numbers, kw in (
            ([b"name", b"city"], [2, 3], {}), ([b"city", b"id", b"city"], [3, 1, 3], dict(only=True)), ([b"k5", (7, None), b"name"], [5, (7, None), 2], dict(only=True, ofs=b", ")),
            ([b"zip code"], [(6, 6)], dict(chomp=True, ors=b"\r\n")), ([b"id", 2, b"name"], [1, 2, 2], dict(only=True, chomp=True, ors=b"|")),
            ([b"name"], [(2, 2)], dict(ors=b"!"))):
        got = _norm(prog.run_records(data, header=N, fields=named, fs=FS, **kw))
        want = _norm(prog.run_records(data, fields=numbers, fs=FS, **kw))
        assert len(got) == len(want) == len(rows) and got[N:] == want[N:], (named, kw, next(i for i in range(N, len(rows)) if got[i] != want[i]))
        items = host._check_field_items(numbers)[0] if kw.get("only") else None
        assert got[:N] == _header_model(data, offs, N, False, 1, items, kw.get("ofs", FS), kw.get("chomp", False), kw.get("ors", b"")), (named, kw, got[:N])
        assert _norm(prog.run_records(data, header=N, fields=numbers, fs=FS, **kw)) == got                 # numbers with a header: the same
        seen |= {type(g) for g in want[N:]} | {("head", type(g)) for g in got[:N]}
    assert {bytes, tuple} <= seen and (N == 1 or ("head", tuple) in seen)                  # accepted and rejected data; a short header under only


def test_quoted_header_cells_values_blanks_and_the_byte_order_mark():
    prog = Program(blob_of(COPY))
    bom = b"\xef\xbb\xbf"
    quoted = [b.replace(b"\n", b" ") + (b'"' if b.count(b'"') % 2 else b"") for b in _hundred("quoted") * 2]    # (one record a line)
    data = bom + b'"id";"na;me";"ci""ty";plain;na;me\n' + b"".join(b + b"\n" for b in quoted)
    offs = list(host.split_records_model(data, b"\n", b'"'))
    assert len(offs) - 1 == 201
    for named, numbers, kw in (([b"na;me", b"id"], [2, 1], {}), ([b'ci"ty', b"plain"], [3, 4], dict(only=True, ofs=b"|")),
                               ([b"plain", b"id", b"na;me"], [4, 1, 2], dict(only=True, unquote=True, ofs=b","))):
        got = _norm(prog.run_records(data, header=1, fields=named, fs=FS, quote=b'"', **kw))
        want = _norm(prog.run_records(data, fields=numbers, fs=FS, quote=b'"', **kw))
        assert got[1:] == want[1:]
        items = host._check_field_items(numbers)[0] if kw.get("only") else None
        assert got[:1] == _header_model(data, offs, 1, False, 1, items, kw.get("ofs"), quote=b'"', unquote=kw.get("unquote", False)), got[:1]
    assert got[0] == b"plain," + bom + b'id,"na;me"\n'                                     # (the mark is copied like any other byte)
    with pytest.raises(HeaderError):
        prog.run_records(data, header=1, fields=[bom + b"id"], fs=FS, quote=b'"')
    assert _norm(prog.run_records(data[3:], header=1, fields=[b"id"], fs=FS, quote=b'"'))[1:] == _norm(prog.run_records(data[3:], fields=[(1, 1)], fs=FS, quote=b'"'))[1:]
    # words: a `ps` listing
    lines = [b"USER       PID %CPU COMMAND"] + [b"u%d  %d\t%d.0  cmd%s" % (i % 7, i, i % 100, b" -x" * (i % 3)) for i in range(200)] + [b"short"]
    data = b"".join(x + b"\n" for x in lines)
    offs = list(host.split_records_model(data, b"\n"))
    for kw in ({}, dict(only=True), dict(only=True, ofs=b"\t", chomp=True, ors=b"\n")):
        got = _norm(prog.run_records(data, header=1, fields=[b"COMMAND", b"PID"], blanks=True, **kw))
        want = _norm(prog.run_records(data, fields=[4, 2], blanks=True, **kw))
        assert got[1:] == want[1:] and got[-1] == ("nofield", 1)
        items = ((4, 4), (2, 2)) if kw.get("only") else None
        assert got[:1] == _header_model(data, offs, 1, False, 1, items, kw.get("ofs", b" "), kw.get("chomp", False), kw.get("ors", b""), fs=None, blanks=True)


def test_fewer_records_than_the_header_and_the_tail():
    prog = Program(blob_of(FIELDS))
    assert prog.run_records(b"", header=2, fields=[b"x"], fs=FS) == []
    assert prog.run_records(b"a;b\nc;d", header=5, fields=[b"x"], fs=FS, chomp=True, ors=b"|") == [b"a;b|", b"c;d|"]      # nothing resolves: all copied
    assert prog.run_records(b"a;b\nc;d", header=5, fields=[b"x"], fs=FS, only=True) == [b"", b""]                           # … or held for good
    assert prog.run_records(b"a;b\nc;d", header=5, fields=[2, 1], fs=FS, only=True) == [b"b;a\n", b"d;c"]
    assert prog.run_records(b"id;name", header=1, fields=[b"name"], fs=FS) == [b"id;name"]                                   # the header is the tail
    assert prog.run_records(b"id;name", header=1, fields=[b"name", b"id"], fs=FS, only=True, ors=b"\n") == [b"name;id\n"]
    assert _norm(prog.run_records(b"id;name\nab;c1\nab;cd\n", header=1, fields=[b"name"], fs=FS)) == [b"id;name\n", (1, 0, 2), b"ab;<cd>\n"]
    with pytest.raises(HeaderError) as e:
        prog.run_records(b"x\nid;name\nab;cd\n", header=2, fields=[b"id", b"nam"], fs=FS)
    assert e.value.name == b"nam"
    with pytest.raises(HeaderError, match="ranges"):
        prog.run_records(FS.join(b"c%d" % k for k in range(20)) + b"\n", header=1, fields=[b"c%d" % (2 * k) for k in range(9)], fs=FS)
    with pytest.raises(ValueError, match="need header"):
        prog.run_records(b"id\n", fields=[b"id"], fs=FS)


# ---------------------------------------------------------------------------------------------------------- 3. streams
def _stream_want(prog, data, N, header_kw, numbers, single_style=False, **kw):
    """stdout and stderr of `BIN --records --header=N …`: the header records by the model, the rest by the numeric call"""
    res = _norm(prog.run_records(data, fields=numbers, fs=FS, **kw))
    if "rs" in kw:
        offs, _, tail_len = host.split_rs_records_model(data, kw["rs"])
        tail = tail_len > 0
    else:
        offs = host.split_records_model(data, b"\n", kw.get("quote"))
        tail = bool(data) and not data.endswith(b"\n")
    offs = list(offs)
    sep_len = len(kw.get("rs", b"\n"))
    head = _header_model(data, offs, N, tail, sep_len, chomp=kw.get("chomp", False), ors=kw.get("ors", b""), **header_kw)
    ranges = host._check_field_ranges(numbers)
    out, err = [], []
    for i, g in enumerate(head + res[len(head):]):
        if isinstance(g, bytes):
            out.append(g)
        elif g[0] == "nofield":
            err.append("Record %d has no field %d!\n" % (i + 1, host.field_list_missing(ranges, g[1])))
        elif single_style:
            err.append("Match error at input symbol %d in record %d!\n" % (g[0], i + 1))
        else:
            err.append("Match error at input symbol %d in field %d of record %d!\n" % (g[0], g[2], i + 1))
    return b"".join(out), "".join(err).encode()


def _wide(ncols, nrows, seed):
    """a header of `ncols` 8-byte columns and rows of a few cells, some with a digit (rejected), some short"""
    r = random.Random(seed)
    header = FS.join(b"col%04d" % k for k in range(ncols))
    rows = [FS.join(r.choice([b"ab", b"c", b"", b"xyz", b"q1"]) for _ in range(r.randrange(1, 8))) for _ in range(nrows)]
    return header, rows


@pytest.mark.parametrize("case", ["one window", "two windows", "edge inside record 2", "carried and projected", "rs", "chomp ors", "single number"])
def test_binary_header_records_across_small_windows(tmp_path_factory, case):
    blob, exe = blob_of(WHOLE), single._bin(tmp_path_factory, WHOLE)
    prog = Program(blob)
    args, N, kw, header_kw, style = ["--records"], 1, {}, {}, False
    if case in ("one window", "two windows"):
        header, rows = _wide(600 if case == "one window" else 1100, 300, 1)
        assert (4096 < len(header) < 8192) if case == "one window" else (8192 < len(header) < 12288)
        recs, names, numbers = [header] + rows, "col0003,col0001,5-", [4, 2, (5, None)]
    elif case == "edge inside record 2":
        header, rows = _wide(40, 300, 2)
        recs, names, numbers, N = [b"# generated", b"# " + b"filler " * 700, header] + rows, "col0002,col0004", [3, 5], 3
        assert len(recs[0]) < 4096 < len(recs[0]) + len(recs[1])
    elif case == "carried and projected":
        header, rows = _wide(700, 300, 3)
        recs, names, numbers = [header] + rows, "col0004,col0002,col0004", [5, 3, 5]
        args += ["--only", "--ofs=, "]
        kw, header_kw = dict(only=True, ofs=b", "), dict(items=((5, 5), (3, 3), (5, 5)), ofs=b", ")
    elif case == "rs":
        header, rows = _wide(600, 200, 4)
        recs, names, numbers = [header] + rows, "col0002,col0599", [3, 600]
        args, kw = ["--records", "--rs=\\r\\n"], dict(rs=b"\r\n")
    elif case == "chomp ors":
        header, rows = _wide(30, 300, 5)
        recs, names, numbers, N = [b"first", header] + rows, "col0001,col0003", [2, 4], 2
        args += ["--chomp", "--ors=\\n"]
        kw = dict(chomp=True, ors=b"\n")
    else:
        header, rows = _wide(600, 300, 6)
        recs, names, numbers, style = [header] + rows, "2", [2], True
    sep = kw.get("rs", b"\n")
    data = sep.join(recs) + (b"" if case == "chomp ors" else sep)                          # (one stream ends in a tail)
    if style:
        res = _norm(prog.run_records(data, field=2, fs=FS))
        out = data[:len(header) + 1] + b"".join(g for g in res[1:] if isinstance(g, bytes))
        err = "".join("Record %d has no field 2!\n" % (i + 1) if g[0] == "nofield" else "Match error at input symbol %d in record %d!\n" % (g[0], i + 1)
                      for i, g in enumerate(res) if i and isinstance(g, tuple)).encode()
    else:
        out, err = _stream_want(prog, data, N, header_kw, numbers, **kw)
    assert err and out
    cmd = args + ["--header" if N == 1 else "--header=%d" % N, "--field=" + names, "--fs=;"]
    r = single._run_bin(exe, cmd, data, 4096)
    assert (r.returncode, r.stderr) == (1, err), (case, r.returncode, r.stderr[:300], err[:300])
    assert r.stdout == out, (case, len(r.stdout), len(out), next(i for i in range(min(len(out), len(r.stdout)) + 1) if r.stdout[i:i + 1] != out[i:i + 1]))


def test_binary_short_streams(tmp_path_factory):
    exe = single._bin(tmp_path_factory, WHOLE)
    run = lambda args, data: (lambda r: (r.returncode, r.stdout, r.stderr))(single._run_bin(exe, ["--records"] + args, data, 4096))   # noqa: E731
    assert run(["--header=5", "--field=name", "--fs=;"], b"a;b\nc;d\ne") == (0, b"a;b\nc;d\ne", b"")           # fewer than N records: all header
    assert run(["--header=5", "--field=name", "--fs=;", "--chomp", "--ors=|"], b"a;b\nc;d\ne") == (0, b"a;b|c;d|e|", b"")
    assert run(["--header=5", "--field=2,1", "--fs=;", "--only"], b"a;b\nc;d\n") == (0, b"b;a\nd;c\n", b"")
    assert run(["--header=5", "--field=name", "--fs=;", "--only"], b"a;b\nc;d\n") == (0, b"", b"")             # held until record 5, which never comes
    assert run(["--header", "--field=name", "--fs=;"], b"") == (0, b"", b"") and run(["--header=3"], b"") == (0, b"", b"")
    assert run(["--header", "--field=name", "--fs=;"], b"id;name") == (0, b"id;name", b"")                     # the header is the stream's tail
    assert run(["--header", "--field=name,id", "--fs=;", "--only", "--chomp", "--ors=\\n"], b"id;name") == (0, b"name;id\n", b"")


def test_binary_small_examples(tmp_path_factory):
    exe = single._bin(tmp_path_factory, WHOLE)
    run = lambda args, data: (lambda r: (r.returncode, r.stdout, r.stderr))(single._run_bin(exe, ["--records"] + args, data, 4096))   # noqa: E731
    assert run(["--header"], b"Id\nab\n1\n") == (1, b"Id\n[ab]\\n", b"Match error at input symbol 0 in record 3!\n")   # no field mode at all
    assert run(["--header", "--field=name", "--fs=;"], b"id;name\nab;cd\n") == (0, b"id;name\nab;[cd]\n", b"")
    assert run(["--quote", "--header", "--field=city,name", "--fs=,", "--unquote", "--only", "--ofs=\\t"],
               b'id,"name",city\n1,"ab,c",x\n') == (0, b'city\t"name"\n[x]\t"[ab,c]"\n', b"")
    assert run(["--rs=\\r\\n", "--header", "--field=name", "--fs=;"], b"id;name\r\nab;cd\r\n") == (0, b"id;name\r\nab;[cd]\r\n", b"")
    assert run(["--header", "--field=name", "--fs=;"], b"id;name\r\nab;cd\r\n")[0] == 2                          # CRLF is not stripped: the cell is name\r
    assert run(["--header", "--field=name\\r", "--fs=;"], b"id;name\r\nab;cd\r\n") == (0, b"id;name\r\nab;[cd]\\r\n", b"")


# ---------------------------------------------------------------------------------------------------------- 4. failures
def test_a_missing_name_ends_the_run(tmp_path_factory):
    exe = single._bin(tmp_path_factory, WHOLE)
    data = b"id;name\n" + b"ab;cd\n" * 50
    r = single._run_bin(exe, ["--records", "--header", "--field=id,nam\\0e", "--fs=;"], data, 4096)
    assert (r.returncode, r.stdout) == (2, b"")
    assert r.stderr == exe.encode() + b': kx_run_records_fd_table: no cell of header record 1 is named "nam\\x00e"\n'
    r = single._run_bin(exe, ["--records", "--header=2", "--field=city", "--fs=;"], b"first\n" + data, 4096)
    assert r.returncode == 2 and not r.stdout.startswith(b"first\nid") and b'header record 2 is named "city"' in r.stderr
    r = single._run_bin(exe, ["--records", "--header", "--field=" + ",".join("c%d" % (2 * k) for k in range(9)), "--fs=;"],
                        FS.join(b"c%d" % k for k in range(20)) + b"\nab\n", 4096)
    assert (r.returncode, r.stdout) == (2, b"") and b"more than 8 ranges" in r.stderr
    r = single._run_bin(exe, ["--records", "--header", "--field=3,1", "--fs=;", "--only"], b"id;name\nab;cd;e\n", 4096)   # a short header, numbers
    assert (r.returncode, r.stdout, r.stderr) == (1, b"[e];[ab]\n", b"Record 1 has no field 3!\n")
    prog = Program(blob_of(WHOLE))
    with pytest.raises(HeaderError) as e:
        prog.run_records(data, header=1, fields=[b"id", b"nam\0e"], fs=FS)
    assert e.value.name == b"nam\0e"
    rd, wr = os.pipe()
    os.write(wr, data)
    os.close(wr)
    ord_, owr = os.pipe()
    with pytest.raises(EngineError, match=r'kx_run_records_fd_table: no cell of header record 1 is named "nam\\x00e"'):
        prog.run_records_fd(rd, owr, header=1, fields=[b"id", b"nam\0e"], fs=FS)
    os.close(owr); os.close(rd)
    assert os.read(ord_, 100) == b""
    os.close(ord_)
    rd, wr = os.pipe()
    os.write(wr, data)
    os.close(wr)
    ord_, owr = os.pipe()
    st = prog.run_records_fd(rd, owr, header=1, fields=[b"name"], fs=FS)
    os.close(owr); os.close(rd)
    assert os.read(ord_, 1000) == b"id;name\n" + b"ab;[cd]\n" * 50 and not st["rejected"] and st["records"] == 51
    os.close(ord_)


# ---------------------------------------------------------------------------------------------------------- 5. unchanged ground
def _fd_call(tmp_path, data, call):
    """`call(in_fd, out_fd, report_fd)` over files → (its result, stdout bytes, report bytes)"""
    (tmp_path / "in").write_bytes(data)
    fin = os.open(str(tmp_path / "in"), os.O_RDONLY)
    fout = os.open(str(tmp_path / "out"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    frep = os.open(str(tmp_path / "rep"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    try:
        res = call(fin, fout, frep)
    finally:
        for fd in (fin, fout, frep):
            os.close(fd)
    return res, (tmp_path / "out").read_bytes(), (tmp_path / "rep").read_bytes()


@pytest.mark.parametrize("flags", [None, 8, 0, 2, 1, 3, 4, 5, 6, 7])
def test_table_without_a_header_is_the_entry_point_its_flags_name(tmp_path, flags):
    prog = Program(blob_of(WHOLE))
    W, U, ONLY = host.KX_TABLE_WORDS, host.KX_TABLE_UNQUOTE, host.KX_TABLE_ONLY
    r = random.Random(flags or 0)
    words = bool(flags and flags & W and flags != 8)
    cells = [b"ab", b"c", b"", b'"x y"', b"q1", b'"k;l"', b"z"]
    join = b" " if words else FS
    data = b"".join(join.join(r.choice(cells) for _ in range(r.randrange(1, 7))) + b"\n" for _ in range(300)) + b"ab" + join + b"cd"
    kw = dict(quote=b'"', chomp=True, ors=b"|\n")
    if flags is None:
        items = []
    elif flags == 8:
        items, kw = [2], dict(kw, field=2, fs=FS)
    else:
        items = [3, 1, (2, 2)] if flags & ONLY else [1, (2, 3)]
        kw = dict(kw, fields=items, blanks=words, unquote=bool(flags & U), only=bool(flags & ONLY), **({} if words else dict(fs=FS)))
        if flags & ONLY:
            kw["ofs"] = b"," if flags & U else b"<>"
    want = _fd_call(tmp_path, data, lambda i, o, rep: prog.run_records_fd(i, o, report_fd=rep, **kw))
    opts = host.KxRecordsOpts(size=ctypes.sizeof(host.KxRecordsOpts), mode=host.KX_RECORDS_QUOTED, sep=10, quote=34, escape=-1, chomp=1, ors_len=2)
    opts.ors[:2] = b"|\n"
    table = host.records_table(0, items, flags or 0, 0 if words else FS[0], kw.get("ofs", b""))
    st = host.KxRecordsStats()

    def call(i, o, rep):
        with prog._batch_actions_for_call(True):
            return prog._lib.kx_run_records_fd_table(prog._h, i, o, ctypes.byref(opts), ctypes.byref(table), rep, ctypes.byref(st))

    got = _fd_call(tmp_path, data, call)
    assert got[0] == (1 if want[0]["rejected"] else 0) and got[1:] == want[1:] and want[1] and want[2], (flags, got[0], got[2][:200], want[2][:200])
    assert (st.records, st.records_rejected, st.out_bytes) == (want[0]["records"], want[0]["records_rejected"], want[0]["out_bytes"])
