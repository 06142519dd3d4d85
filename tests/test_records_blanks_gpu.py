"""GPU: field mode on words — kx_run_batch_field_words (Program.run_batch_field_words_tensor), Program.run_records(blanks=True),
Program.run_records_fd(blanks=True) and `BIN --records … --field=K|LIST --blanks [--unquote]`.  Every record's expected result is
built in Python: host.blank_field_list_records_model cuts the record into gaps and words, the CPU oracle runs on each selected word
alone (with `unquote` on its value, host.unquote_field_model, and the output is spelled by host.requote_field_model with the space
for the field separator and the tab among the special bytes), and gaps + outputs + separator + suffix are spliced here."""
import itertools
import os
import random

import pytest
from conftest import blob_of

import test_records_field_gpu as single
import test_records_field_list_gpu as listed
from kleenexlang_amd import build, host, program_path
from kleenexlang_amd.host import MatchError, NoFieldError, Program

pytestmark = pytest.mark.gpu

GROW = 'main := "<" /[^\\n]*/ ">"\n'                                                  # every word grows by two bytes
SOME = 'main := ~/a/ | /aa/ | /aaa/ | /aaaaa+/\n'                                     # "a" gives the empty output, "aaaa" is rejected
MAP = 'main := (~/_/ " " | ~/-/ "\\t" | ~/=/ "\\"" | ~/%/ "\\\\" | /[a-z]/)*\n'         # outputs with a space, a tab, a quote, a backslash
LEAD, TRAIL = b" \ta \t  a\t \t a  \t", b" \t a"                                      # in front of off[0] and behind off[n]: blanks and words too
P = host.parse_field_list
_want = single._want
model = host.blank_field_list_records_model


def _expected(blob, data, offs, ranges, quote=None, escape=None, unquote=False, special=b"\n", sep_len=0, last_whole=False, keep_sep=True,
              suffix=b""):
    """(output bytes, output offsets, status, fail_pos, fail_stage, fail_field) from the model, the oracle and a splice in Python."""
    out, ooff, status, fpos, fstage, ffield = [], [0], [], [], [], []
    for m in model(data, offs, sep_len, last_whole, ranges, quote, escape):
        if isinstance(m, int):
            s = (m, 2, 0, host.field_list_missing(ranges, m))
        else:
            gaps, fields, sep = m
            res = [_want(blob, host.unquote_field_model(f, quote, escape) if unquote else f) for _, f in fields]
            bad = next((j for j, w in enumerate(res) if isinstance(w, tuple)), None)         # the lowest rejected word
            s = (res[bad][0], 1, res[bad][1], fields[bad][0]) if bad is not None else None
            if s is None and unquote:
                res = [host.requote_field_model(w, quote is not None and f[:1] == quote, b" ", quote, escape, special + b"\t")
                       for w, (_, f) in zip(res, fields)]
        if s is not None:
            fpos.append(s[0]); status.append(s[1]); fstage.append(s[2]); ffield.append(s[3])
            ooff.append(ooff[-1])
        else:
            status.append(0); fpos.append(0); fstage.append(0); ffield.append(0)
            out.append(b"".join(g + w for g, w in zip(gaps, res + [b""])) + (sep if keep_sep else b"") + suffix)
            ooff.append(ooff[-1] + len(out[-1]))
    return b"".join(out), ooff, status, fpos, fstage, ffield


def _device(data, offs, lead):
    """data at `lead` bytes into a buffer of blanks and letters (so that off[0] = lead), more of them behind it."""
    import torch
    v = torch.frombuffer(bytearray(LEAD[:lead] + data + TRAIL), dtype=torch.uint8).cuda()
    assert v.data_ptr() % 16 == 0
    o = torch.tensor([x + lead for x in offs], dtype=torch.int64).cuda()
    return v, o


def _check(prog, blob, data, offs, ranges, lead=0, **kw):
    import torch
    want = _expected(blob, data, offs, ranges, **kw)
    v, o = _device(data, offs, lead)
    res = prog.run_batch_field_words_tensor(v, o, ranges, **kw)
    torch.cuda.synchronize()
    got = (res[0].cpu().numpy().tobytes(),) + tuple(t.tolist() for t in res[1:])
    ctx = (ranges, lead, kw)
    rec = lambda i: data[offs[min(i, len(offs) - 2)]:offs[min(i, len(offs) - 2) + 1]][:100]   # noqa: E731
    for name, k in (("status", 2), ("fail_pos", 3), ("fail_stage", 4), ("fail_field", 5), ("out_off", 1)):
        if got[k] != want[k]:
            i = next(j for j in range(len(want[k])) if got[k][j] != want[k][j])
            raise AssertionError("%s[%d]: got %r, want %r (record %r, %r)" % (name, i, got[k][i], want[k][i], rec(i), ctx))
    assert got[0] == want[0], (ctx, next((i, rec(i), got[0][want[1][i]:want[1][i + 1]][:100]) for i in range(len(offs) - 1)
                                         if got[0][want[1][i]:want[1][i + 1]] != want[0][want[1][i]:want[1][i + 1]]))
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.out_bytes) == (len(offs) - 1, sum(1 for s in want[2] if s), len(want[0]))
    return want


def _pack(bodies, sep_len):
    """The bodies, each with sep_len bytes behind it that are no blanks (and that every program here but SOME takes in a word: with
    last_whole they are part of the last body)."""
    return host.pack_batch([b + (b"\r;\r;\r;\r;")[:sep_len] for b in bodies])


# ---------------------------------------------------------------------------------------------------------- 1. every small body
SMALL = [bytes(t) for L in range(8) for t in itertools.product(b"a \t", repeat=L)]
LISTS = ["1", "2", "1-", "2,4-", "3-3"]


@pytest.mark.parametrize("name,src", [("grow", GROW), ("some", SOME)])
def test_every_small_body_at_every_residue(name, src):
    assert len(SMALL) == 3280
    blob = blob_of(src)
    prog = Program(blob)
    seen, n = set(), 0
    for lead in (0, 1, 15):
        for text in LISTS:
            sep_len, keep_sep, last_whole, suffix = (0, 1, 2)[n % 3], (n // 3) % 2 == 0, n % 2 == 1, (b"", b"|", b" \t\n")[(n // 2) % 3]
            data, offs = _pack(SMALL, sep_len)                                          # back to back: the starts fall on every residue
            want = _check(prog, blob, data, offs, P(text), lead=lead, sep_len=sep_len, last_whole=last_whole, keep_sep=keep_sep, suffix=suffix)
            assert {(o + lead) % 16 for o in offs[:-1]} == set(range(16))
            seen |= {("sep", sep_len), ("keep", keep_sep), ("lw", last_whole), ("sfx", suffix)} | {("status", s) for s in want[2]}
            seen |= {("found", p) for s, p in zip(want[2], want[3]) if s == 2}
            n += 1
    statuses = {0, 2} if name == "grow" else {0, 1, 2}
    assert {v for k, v in seen if k == "status"} == statuses and {v for k, v in seen if k == "found"} >= {0, 1, 2, 3}
    assert len({x for x in seen if x[0] in ("sep", "keep", "lw", "sfx")}) == 3 + 2 + 2 + 3
    if name == "some":                                                                  # a word that maps to nothing leaves its blanks
        assert _check(prog, blob, b" a  aa\ta ", [0, 9], P("1-"))[0] == b"   aa\t "


# ---------------------------------------------------------------------------------------------------------- 2. granule seams
def _seam_bodies(r):
    """Bodies of 0 to 80 bytes: a run of 1 to 20 blanks that ends at, begins at and straddles each 16-byte boundary; a word that
    ends on a granule's last byte; a word that begins on a granule's first byte; a last granule of only blanks; the second word —
    where the lists `2` and `1-2` stop — beginning and ending at and around a boundary."""
    letters = lambda k: bytes(r.choice(b"abcdefgh") for _ in range(k))                   # noqa: E731
    blanks = lambda k: bytes(r.choice(b" \t") for _ in range(k))                         # noqa: E731

    def text(k):                                                                         # k bytes of words with single blanks, letters at both ends
        t = bytearray(letters(k))
        for i in range(1, k - 1):
            if r.randrange(5) == 0 and t[i - 1] not in b" \t":
                t[i] = r.choice(b" \t")
        return bytes(t)

    out = []
    for B in (16, 32, 48, 64):
        for n in range(1, 21):
            for start in (B - n, B, B - (n + 1) // 2):
                if start >= 0 and start + n <= 80:
                    out.append(text(start) + blanks(n) + text(r.randrange(0, 81 - start - n)))
        for k in (1, 2, 5, 15):
            out.append(text(B - k - 1) + b" " + letters(k) + b"\t" + text(r.randrange(0, 12)))    # a word in [B - k, B), a blank at B
            out.append(text(B - k - 1) + b" " + letters(k))                                      # … and the body ends with it
            out.append(text(B - 1) + b"\t" + letters(k) + b" " + text(r.randrange(0, 4)))         # a blank at B - 1, a word from B
        out.append(letters(B) + b" " + letters(3))                                               # one word over every granule so far
        for t in range(1, 17):
            out.append(text(B - 16) + blanks(t))                                                 # the last granule: blanks only
            out.append(blanks(B) + text(t))                                                      # the first granules: blanks only
    for b2 in (15, 16, 17):
        for e2 in (b2 + 1, 31, 32, 33):
            head = b"aaa" + b" " * (b2 - 3) + letters(e2 - b2)
            out += [head, head + b" ", head + b"\tcc  dd e"]
    return out


def test_granule_seams():
    blob = blob_of(GROW)
    prog = Program(blob)
    r = random.Random(16)
    bodies, pos, shaped = [], 0, []
    for b in _seam_bodies(r):
        assert len(b) <= 80 and pos % 16 == 0
        shaped.append(len(bodies))
        bodies.append(b)
        pos += len(b) + 1
        k = (-pos - 1) % 16                                                              # a filler record: the next one starts a granule
        bodies.append(b"x" * k)
        pos += k + 1
    data, offs = _pack(bodies, 1)
    assert all(offs[i] % 16 == 0 for i in shaped) and len(shaped) > 400
    for lead in (0, 1, 15):
        for text in LISTS + ["1-2"]:
            want = _check(prog, blob, data, offs, P(text), lead=lead, sep_len=1, suffix=b"|")
            assert set(want[2]) == {0, 2}


# ---------------------------------------------------------------------------------------------------------- 3. QUOTED, ESCAPED
HAND = [b'a "b  c" d', b"a\\ b c", b'"a\\" b" c', b'a "b c', b"a b\\", b"a b \\", b'"GET / HTTP/1.0" 200', b' "" \t"" ', b"\\ ", b'" "', b'"', b"\\"]


@pytest.mark.parametrize("quote,escape", [(b'"', None), (None, b"\\"), (b'"', b"\\")])
def test_quoted_and_escaped_words(quote, escape):
    blob = blob_of(GROW)
    prog = Program(blob)
    r = random.Random(48)
    bodies = HAND + [bytes(r.choice(b'ab \t"\\') for _ in range(r.randrange(0, 49))) for _ in range(1500)]
    data, offs = _pack(bodies, 1)
    plain = model(data, offs, 1, False, P("1-"))
    mine = model(data, offs, 1, False, P("1-"), quote, escape)
    assert sum(1 for a, b in zip(plain, mine) if a != b) > 300                            # the quote and the escape decide
    for lead, text in ((0, "1-"), (5, "2"), (11, "2,4-"), (15, "1,3")):
        want = _check(prog, blob, data, offs, P(text), lead=lead, quote=quote, escape=escape, sep_len=1)
        assert set(want[2]) == {0, 2}
    w = _check(prog, blob, b'a "b  c" d', [0, 10], P("2"), quote=quote, escape=escape)
    assert w[0] == (b'a <"b  c"> d' if quote else b'a <"b>  c" d')
    w = _check(prog, blob, b"a\\ b c", [0, 6], P("1"), quote=quote, escape=escape)
    assert w[0] == (b"<a\\ b> c" if escape else b"<a\\> b c")


# ---------------------------------------------------------------------------------------------------------- 4. long lists, long records
def test_eight_ranges_and_an_open_range_over_three_thousand_words():
    blob = blob_of(GROW)
    prog = Program(blob)
    r = random.Random(40)
    word = lambda: bytes(r.choice(b"abcxyz") for _ in range(r.randrange(1, 9)))          # noqa: E731
    gap = lambda: bytes(r.choice(b" \t") for _ in range(r.choice((1, 1, 1, 2, 3, 17))))   # noqa: E731
    line = lambda n: gap() * r.randrange(2) + b"".join(word() + gap() for _ in range(n - 1)) + word() + gap() * r.randrange(2)   # noqa: E731
    eight = "1,3,5-6,8,10,12,14-20,30-"
    bodies = [line(40), line(29), line(30), line(3), line(2), b"", line(3000), line(40)]
    data, offs = _pack(bodies, 1)
    want = _check(prog, blob, data, offs, P(eight), lead=3, sep_len=1)
    assert want[2] == [0, 2, 0, 2, 2, 2, 0, 0] and want[5] == [0, 30, 0, 5, 3, 1, 0, 0] and want[3][5] == 0
    assert want[0].count(b"<") == 2 * (14 + 11) + (14 + 1) + (14 + 2971)                   # 14 words in the closed ranges, then 30-
    want = _check(prog, blob, data, offs, P("3-"), lead=9, sep_len=1, keep_sep=False, suffix=b"\n")
    assert want[2] == [0, 0, 0, 0, 2, 2, 0, 0] and want[5] == [0, 0, 0, 0, 3, 3, 0, 0]
    assert want[0][want[1][6]:want[1][7]].count(b"<") == 2998


def test_one_long_word_takes_the_route():
    blob = blob_of(GROW)
    prog = Program(blob)
    r = random.Random(3)
    long_word = bytes(r.choice(b"abc,") for _ in range(70 << 10))                        # above batch_doc_max (64 KiB)
    bodies = [b"ab  c,d e f", b" x y", b"k"] * 20 + [b"pre \t" + long_word + b"  mid post "] + [b"ab c,d e ", b"", b" x  z "] * 20
    data, offs = _pack(bodies, 1)
    want = _check(prog, blob, data, offs, P("2,4-"), lead=7, sep_len=1, suffix=b"|")
    assert prog.last_batch_stats.docs_routed == 1 and set(want[2]) == {0, 2}
    assert want[0][want[1][60]:want[1][61]] == b"pre \t<" + long_word + b">  mid <post> \r|"


# ---------------------------------------------------------------------------------------------------------- 5. --unquote
def test_unquoted_words_are_spelled_with_the_space_and_the_tab():
    blob = blob_of(MAP)
    prog = Program(blob)
    Q, E = b'"', b"\\"
    one = lambda body, text, **kw: _check(prog, blob, body, [0, len(body)], P(text), unquote=True, **kw)[0]   # noqa: E731
    # quote mode: an output with a blank is wrapped; a word that was quoted stays quoted; the empty output of a quoted word is ""
    assert one(b'x  a_b\t"c" "" y', "2-4", quote=Q) == b'x  "a b"\t"c" "" y'
    assert one(b"x a-b y", "2", quote=Q) == b'x "a\tb" y'                                  # (the tab is a special byte)
    assert one(b'x a=b "c=d" y', "2-3", quote=Q) == b'x "a""b" "c""d" y'
    assert _check(prog, blob, b'x "a b"  c', [0, 10], P("2"), unquote=True, quote=Q)[2:] == ([1], [1], [0], [2])   # S counts inside the value: a b
    assert one(b' "a_b" ', "1", quote=Q) == b' "a b" '
    # escape only: every blank of the output gets an escape byte; nothing is wrapped
    assert one(b"x  a_b\ty", "2", escape=E) == b"x  a\\ b\ty"
    assert one(b"x a-b a%b", "2-", escape=E) == b"x a\\\tb a\\\\b"
    assert one(b"x a\\_b y", "2", escape=E) == b"x a\\ b y"                                # (the value is a_b)
    # quote and escape: wrapped for a blank, quotes escaped
    assert one(b'x a_b "c" a=b y', "2-4", quote=Q, escape=E) == b'x "a b" "c" a\\"b y'
    # the record separator is special as before (here: the default, a newline, which no word of a line can hold; and an explicit one)
    assert one(b"x a_b y", "2", quote=Q, special=b";") == b'x "a b" y'
    r = random.Random(5)
    for quote, escape, pieces in ((Q, None, [b"ab", b"a_b", b'"x"', b'""', b'"a_b"', b"a=b", b"a-b", b"9", b'"a""b"', b"z"]),
                                  (None, E, [b"ab", b"a_b", b"a\\_b", b"a%b", b"a-b", b"9", b"\\a", b"z\\"]),
                                  (Q, E, [b"ab", b"a_b", b'"x"', b'""', b'"a\\"b"', b"a=b", b"a%b", b"a-b", b"9", b"z"])):
        bodies = [b"".join(r.choice(pieces) + bytes(r.choice(b" \t") for _ in range(r.choice((1, 1, 2, 5)))) for _ in range(r.randrange(0, 8)))
                  + r.choice(pieces) * r.randrange(2) for _ in range(400)]
        data, offs = _pack(bodies, 1)
        for lead, text in ((0, "1-"), (7, "2"), (13, "2,4-")):
            want = _check(prog, blob, data, offs, P(text), lead=lead, quote=quote, escape=escape, unquote=True, sep_len=1)
            assert set(want[2]) == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------- 6. windows, the binary
FLIP = open(program_path("flip_ab")).read()


def _stream():
    """About 13 KiB of lines of words over {a, b}: one line, and a run of blanks inside it, straddles the first 4 KiB boundary;
    lines with a rejected word, with too few words and without any word in every window."""
    r = random.Random(4096)
    word = lambda: bytes(r.choice(b"ab") for _ in range(r.randrange(1, 7)))               # noqa: E731
    gap = lambda: bytes(r.choice(b" \t") for _ in range(r.choice((1, 1, 2, 4))))           # noqa: E731
    lines, n = [], 0
    while n < 13000:
        k = r.randrange(12)
        line = (b"" if k == 0 else b" \t " if k == 1 else word() if k == 2 else word() + b"c" + gap() + word() + b"c" + gap() + word() + b"c" if k == 3
                else gap() * r.randrange(2) + b"".join(word() + gap() for _ in range(r.randrange(2, 9))) + word())
        if n < 4096 - 30 <= n + len(line) + 1:                                          # the straddling line: blanks over the boundary
            line = b"ab" + b" " * (4096 - n - 2 - 10) + b" \t" * 10 + b"abba b  a"
            assert n + 2 < 4096 - 8 and n + len(line) > 4096 + 8
        lines.append(line)
        n += len(line) + 1
    return b"\n".join(lines) + b"\n" + b"a  abba"                                          # a tail without a separator


def _want_stream(blob, data, ranges, chomp=False, ors=b""):
    offs = host.split_records_model(data, b"\n")
    tail = not data.endswith(b"\n")
    out, err, res = [], [], []
    for i, m in enumerate(model(data, offs, 1, tail, ranges)):
        if isinstance(m, int):
            err.append("Record %d has no field %d!\n" % (i + 1, host.field_list_missing(ranges, m)))
            res.append(("nofield", m))
            continue
        w = [_want(blob, f) for _, f in m[1]]
        bad = next((j for j, x in enumerate(w) if isinstance(x, tuple)), None)
        if bad is not None:
            err.append("Match error at input symbol %d in field %d of record %d!\n" % (w[bad][0], m[1][bad][0], i + 1))
            res.append((w[bad][0], w[bad][1], m[1][bad][0]))
        else:
            out.append(b"".join(g + x for g, x in zip(m[0], w + [b""])) + (b"" if chomp else m[2]) + ors)
            res.append(out[-1])
    return b"".join(out), "".join(err).encode(), res


def test_run_records_fd_in_small_windows(tmp_path):
    blob = blob_of(FLIP)
    data = _stream()
    (tmp_path / "in").write_bytes(data)
    for kw, ranges in ((dict(field=2), P("2")), (dict(fields=P("2-")), P("2-")), (dict(fields=[1, 3], chomp=True, ors=b";\n"), P("1,3"))):
        out, err, res = _want_stream(blob, data, ranges, kw.get("chomp", False), kw.get("ors", b""))
        kinds = {r[0] == "nofield" and ("nofield", r[1]) or "rejected" if isinstance(r, tuple) else "ok" for r in res}
        assert kinds >= {"ok", "rejected", ("nofield", 0), ("nofield", 1)} and b"in field" in err and b"has no field" in err
        for window in (4096, 1 << 20):
            prog = Program(blob, window_bytes=window)
            with open(tmp_path / "in", "rb") as fi, open(tmp_path / "out", "wb") as fo, open(tmp_path / "err", "wb") as fe:
                st = prog.run_records_fd(fi.fileno(), fo.fileno(), report_fd=fe.fileno(), blanks=True, **kw)
            assert (tmp_path / "err").read_bytes() == err, (kw, window)
            assert (tmp_path / "out").read_bytes() == out, (kw, window)
            assert st["rejected"] and st["records"] == len(res) and st["records_rejected"] == sum(1 for r in res if isinstance(r, tuple))
            assert window > 4096 or st["windows"] >= 3
        got = Program(blob).run_records(data, blanks=True, **kw)
        got = [("nofield", g.fields) if isinstance(g, NoFieldError) else (g.pos, g.stage, g.field) if isinstance(g, MatchError) else g for g in got]
        assert got == res, (kw, next((i, g, w) for i, (g, w) in enumerate(zip(got, res)) if g != w))
    assert Program(blob).run_records(b"", field=2, blanks=True) == []


LOG = (b'192.0.2.7 - alice [20/Oct/2026:19:09:00 +0000] "GET /a/b.html?session=41 HTTP/1.1" 200 5120 "http://example.org/start page" '
       b'"Mozilla/5.0 (X11; Linux x86_64)"\n'
       b'192.0.2.9  -  -  [20/Oct/2026:19:09:01 +0000]\t"POST /form HTTP/1.0" 302 - "-" "curl/8.0"\n'
       b'192.0.2.9 - - [20/Oct/2026:19:09:02 +0000] "BREW /pot HTCPCP/1.0" 418 - "-" "-"\n'
       b'192.0.2.9 - -\n')


def test_the_produced_binary(tmp_path_factory):
    flip = single._bin(tmp_path_factory, FLIP)
    r = single._run_bin(flip, ["--records", "--field=2", "--blanks"], b"  a   abba\tb \n", 1 << 30)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"  a   baab\tb \n", b"")
    r = single._run_bin(flip, ["--records", "--field=2,4-", "--blanks", "--chomp", "--ors=|"], b"a b  a\tab\n\n \nb ab a b\nb ac a ab", 4096)
    assert (r.returncode, r.stdout) == (1, b"a a  a\tba|b ba a a|")
    assert r.stderr == b"Record 2 has no field 2!\nRecord 3 has no field 2!\nMatch error at input symbol 1 in field 2 of record 5!\n"
    data = _stream()
    out, err, _ = _want_stream(blob_of(FLIP), data, P("2-"))
    for window in (4096, 1 << 30):
        r = single._run_bin(flip, ["--records", "--field=2-", "--blanks"], data, window)
        assert (r.returncode, r.stderr, r.stdout) == (1, err, out), window
    # the example: the request of a combined-format log line is its word 6
    src = open(os.path.join(build.PKG, "examples", "request_line.kex")).read()
    exe = single._bin(tmp_path_factory, src)
    r = single._run_bin(exe, ["--records", "--quote", "--blanks", "--field=6", "--unquote"], LOG, 1 << 30)
    lines = LOG.split(b"\n")
    assert r.stdout == (lines[0].replace(b"GET /a/b.html?session=41", b"get /a/b.html") + b"\n" + lines[1].replace(b"POST", b"post") + b"\n")
    assert r.stderr == b"Match error at input symbol 0 in field 6 of record 3!\nRecord 4 has no field 6!\n" and r.returncode == 1
    blob = blob_of(src)
    want = _expected(blob, LOG, host.split_records_model(LOG, b"\n"), P("6"), quote=b'"', unquote=True, sep_len=1)
    assert r.stdout == want[0] and want[2] == [0, 0, 1, 2] and want[3][3] == 3


# ---------------------------------------------------------------------------------------------------------- 7. nothing moved
def test_without_blanks_a_space_separates_single_fields_as_before(tmp_path_factory):
    blob = blob_of(GROW)
    prog = Program(blob)
    data, offs = _pack(SMALL, 1)
    for lead, text in ((0, "1-"), (15, "2,4-")):
        want = listed._check(prog, blob, data, offs, P(text), lead=lead, fs=b" ", sep_len=1)   # the parent's model: field_list_records_model
        words = _expected(blob, data, offs, P(text), sep_len=1)
        assert want[0] != words[0] and want[2] != words[2]
    assert listed._check(prog, blob, b"  a   abba\tb \n", [0, 14], P("1-"), fs=b" ", sep_len=1)[0] == b"<> <> <a> <> <> <abba\tb> <>\n"
    flip = single._bin(tmp_path_factory, FLIP)
    r = single._run_bin(flip, ["--records", "--field=2", "--fs= "], b"  a   abba\tb \n", 1 << 30)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"  a   abba\tb \n", b"")               # field 2 is the empty field between the two spaces
    r = single._run_bin(flip, ["--records", "--field=3-", "--fs= "], b"  a   abba b \n", 1 << 30)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"  b   baab a \n", b"")
