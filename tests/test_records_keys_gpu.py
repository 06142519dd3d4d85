"""GPU: field mode by key — kx_run_batch_field_keys (Program.run_batch_field_keys_tensor), Program.run_records(keys=…),
Program.run_records_fd(keys=…) and `BIN --records … --field=LIST --keys[=C]`.  Every record's expected result is built in Python:
host.keyed_records_model cuts the record into gaps and selected values, the CPU oracle runs on each value alone (with `unquote` on
host.unquote_field_model of it, and the output is spelled by host.requote_field_model), and gaps + outputs + separator + suffix —
with `only` the outputs in written order joined by OFS — are spliced here."""
import itertools
import os
import random

import pytest
from conftest import blob_of

import test_records_field_gpu as single
from kleenexlang_amd import build, host, program_path
from kleenexlang_amd.host import EngineError, MatchError, NoFieldError, Program

pytestmark = pytest.mark.gpu

GROW = 'main := "<" /[^\\n]*/ ">"\n'                                                  # every value grows by two bytes
SOME = 'main := ~/a/ | /aa/ | /b*/ | /ab/\n'                                          # "a" gives the empty output, "ba", "aaa", "a,…" are rejected
MAP = 'main := (~/_/ " " | ~/-/ "," | ~/%/ "\\"" | /[a-z0-9]/)*\n'                     # outputs with a space, a comma, a quote
LEAD, TRAIL = b"a=b,b=a a=1\tb=", b",a=b b=a"                                         # in front of off[0] and behind off[n]: pairs too
_want = single._want
model = host.keyed_records_model


def _lowbit(x):
    return (x & -x).bit_length() - 1


def _expected(blob, data, offs, names, optional=(), kv=b"=", fs=b",", blanks=False, quote=None, escape=None, unquote=False, special=b"\n",
              only=None, ofs=None, sep_len=0, last_whole=False, keep_sep=True, suffix=b""):
    """(output bytes, output offsets, status, fail_pos, fail_stage, fail_field) from the model, the oracle and a splice in Python."""
    out, ooff, status, fpos, fstage, ffield = [], [0], [], [], [], []
    required = sum(1 << t for t, n in enumerate(names) if n not in optional)
    if only is not None and ofs is None:
        ofs = b" " if blanks else fs
    for m in model(data, offs, sep_len, last_whole, names, kv, None if blanks else fs, quote, escape, blanks, optional):
        if isinstance(m, int):
            s = (m, 2, 0, 1 + _lowbit(required & ~m))
        else:
            gaps, fields, sep = m
            res = [_want(blob, host.unquote_field_model(f, quote, escape) if unquote else f) for _, f in fields]
            bad = next((j for j, w in enumerate(res) if isinstance(w, tuple)), None)         # the rejected value at the lowest address
            s = (res[bad][0], 1, res[bad][1], 1 + fields[bad][0]) if bad is not None else None
            if s is None and unquote:
                res = [host.requote_field_model(w, quote is not None and f[:1] == quote, ofs if only is not None else b" " if blanks else fs,
                                                quote, escape, special + (b"\t" if blanks else b"")) for w, (_, f) in zip(res, fields)]
        if s is not None:
            fpos.append(s[0]); status.append(s[1]); fstage.append(s[2]); ffield.append(s[3])
            ooff.append(ooff[-1])
            continue
        status.append(0); fpos.append(0); fstage.append(0); ffield.append(0)
        if only is None:
            body = b"".join(g + w for g, w in zip(gaps, res + [b""]))
        else:
            by_name = {t: w for (t, _), w in zip(fields, res)}
            body = ofs.join(by_name[t] for t in only if t in by_name)
        out.append(body + (sep if keep_sep else b"") + suffix)
        ooff.append(ooff[-1] + len(out[-1]))
    return b"".join(out), ooff, status, fpos, fstage, ffield


def _device(data, offs, lead):
    import torch
    v = torch.frombuffer(bytearray((LEAD * 2)[:lead] + data + TRAIL), dtype=torch.uint8).cuda()
    assert v.data_ptr() % 16 == 0
    o = torch.tensor([x + lead for x in offs], dtype=torch.int64).cuda()
    return v, o


def _check(prog, blob, data, offs, names, lead=0, **kw):
    import torch
    want = _expected(blob, data, offs, names, **kw)
    v, o = _device(data, offs, lead)
    kw = dict(kw)
    kw.setdefault("fs", b",")
    if kw.get("blanks"):
        kw.pop("fs")
    res = prog.run_batch_field_keys_tensor(v, o, names, **kw)
    torch.cuda.synchronize()
    got = (res[0].cpu().numpy().tobytes(),) + tuple(t.tolist() for t in res[1:])
    ctx = (names, lead, kw)
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
    """The bodies, each with sep_len bytes behind it that are neither C, F nor a blank."""
    return host.pack_batch([b + (b"\r;\r;\r;\r;")[:sep_len] for b in bodies])


# ---------------------------------------------------------------------------------------------------------- 1. every small body
SMALL = [bytes(t) for L in range(7) for t in itertools.product(b"ab=,", repeat=L)]
LISTS = [([b"a"], ()), ([b"ab"], ()), ([b"a", b"b"], (b"b",)), ([b"b"], (b"b",)), ([b"a", b"b"], (b"a", b"b"))]


@pytest.mark.parametrize("name,src", [("grow", GROW), ("some", SOME)])
def test_every_small_body_at_every_residue(name, src):
    assert len(SMALL) == 5461
    blob = blob_of(src)
    prog = Program(blob)
    seen, n = set(), 0
    for lead in (0, 1, 15):
        for names, optional in LISTS:
            sep_len, keep_sep, last_whole, suffix = (0, 1, 2)[n % 3], (n // 3) % 2 == 0, n % 2 == 1, (b"", b"|", b"=,\n")[(n // 2) % 3]
            data, offs = _pack(SMALL, sep_len)                                          # back to back: the starts fall on every residue
            only = [None, list(range(len(names)))[::-1]][n % 2] if name == "some" else None
            want = _check(prog, blob, data, offs, names, lead=lead, optional=optional, only=only, sep_len=sep_len, last_whole=last_whole,
                          keep_sep=keep_sep, suffix=suffix)
            assert {(o + lead) % 16 for o in offs[:-1]} == set(range(16))
            seen |= {("sep", sep_len), ("keep", keep_sep), ("lw", last_whole), ("sfx", suffix)} | {("status", s) for s in want[2]}
            docs = model(data, offs, sep_len, last_whole, names, b"=", b",", optional=optional)
            seen |= {("docs", len(m[1])) for m, s in zip(docs, want[2]) if s == 0}
            n += 1
    assert {v for k, v in seen if k == "status"} == ({0, 2} if name == "grow" else {0, 1, 2})
    assert {v for k, v in seen if k == "docs"} == {0, 1, 2}
    assert len({x for x in seen if x[0] in ("sep", "keep", "lw", "sfx")}) == 3 + 2 + 2 + 3


def test_every_small_body_as_words():
    blob = blob_of(GROW)
    prog = Program(blob)
    bodies = [bytes(t) for L in range(7) for t in itertools.product(b"ab= ", repeat=L)] + [b"a=1\tb=2", b"\ta=\t", b"b=a\t \ta=b\t"]
    data, offs = _pack(bodies, 1)
    for lead, (names, optional) in zip((0, 3, 15, 9, 1), LISTS):
        want = _check(prog, blob, data, offs, names, lead=lead, optional=optional, blanks=True, sep_len=1, suffix=b"|")
        assert 0 in want[2]


# ---------------------------------------------------------------------------------------------------------- 2. keys at granule seams
def test_keys_against_granule_seams():
    blob = blob_of(GROW)
    prog = Program(blob)
    for klen in (1, 15, 16, 17, 31, 32, 33, 255):
        name = bytes(97 + k % 23 for k in range(klen))
        last, first = name[:-1] + b"Z", b"Z" + name[1:]
        near = [last + b"=1", first + b"=2", name + b"x=4"] + ([name[:-1] + b"=3"] if klen > 1 else [])
        bodies = []
        for res in range(16):
            pad = b"p" * res                                                          # (a first field without C: the key begins at residue res + 1)
            bodies.append(b",".join([pad] + near + [name + b"=v" + bytes([48 + res]), name + b"=second"]))
            bodies.append(b",".join([pad] + near + [name + b"="]))                    # an empty value at the body's end
            bodies.append(b",".join([pad] + near + [name, b"=", b"=" + name, name + b"=,x"]))   # no C; only C; an empty key; then an empty value
            bodies.append(b",".join([pad] + near))                                    # near misses alone: the name is missing
        recs, pos = [], 0
        for b in bodies:                                                              # every body begins a granule
            recs.append(b)
            pos += len(b) + 1
            k = (-pos - 1) % 16
            recs.append(b"x" * k)
            pos += k + 1
        data, offs = _pack(recs, 1)
        assert all(offs[i] % 16 == 0 for i in range(0, len(recs), 2))
        for lead in (0, 7):
            want = _check(prog, blob, data, offs, [name], lead=lead, sep_len=1)
            assert want[2][:8:2] == [0, 0, 0, 2] and want[5][6] == 1 and want[3][6] == 0
        w = _check(prog, blob, bodies[0], [0, len(bodies[0])], [name])
        assert w[0].endswith(name + b"=<v0>," + name + b"=second")


# ---------------------------------------------------------------------------------------------------------- 3. the name table
def test_sixteen_names_duplicates_missing_and_rejected():
    names = [b"k%02d" % i + b"x" * (i % 5) for i in range(16)]
    blob = blob_of(SOME)
    prog = Program(blob)
    rev = b",".join(n + b"=" + (b"aa", b"bb", b"a", b"")[i % 4] for i, n in enumerate(names[::-1]))
    dup = rev + b"," + names[3] + b"=ba," + names[0] + b"=ba"                         # the second ones are copied, whatever they hold
    no7 = b",".join(n + b"=b" for i, n in enumerate(names) if i not in (7, 11))
    bad = b",".join(n + (b"=ba" if i in (5, 9) else b"=ab") for i, n in enumerate(names[::-1]))   # names 10 and 6, 10 at the lower address
    data, offs = _pack([rev, dup, no7, bad, b""], 1)
    want = _check(prog, blob, data, offs, names, lead=5, sep_len=1)
    assert want[2] == [0, 0, 2, 1, 2] and want[5] == [0, 0, 8, 11, 1]
    assert want[3][2] == 0xFFFF & ~(1 << 7) & ~(1 << 11) and want[3][4] == 0 and want[3][3] == 1
    assert want[0][want[1][1]:want[1][2]].endswith(names[3] + b"=ba," + names[0] + b"=ba\r")
    want = _check(prog, blob, data, offs, names, lead=5, sep_len=1, optional=[names[7]], only=list(range(16)), ofs=b"|")
    assert want[2] == [0, 0, 2, 1, 2] and want[5] == [0, 0, 12, 11, 1]
    assert want[0][:want[1][1]] == b"|".join((b"aa", b"bb", b"", b"")[(15 - i) % 4] for i in range(16)) + b"\r"


# ---------------------------------------------------------------------------------------------------------- 4. zero-document records
@pytest.mark.parametrize("only", [None, [1, 0]])
def test_records_without_a_document(only):
    blob = blob_of(GROW)
    prog = Program(blob)
    names, opt = [b"a", b"bb"], [b"a", b"bb"]
    none = [b"", b"x=1,y=2", b"a,bb", b"=a,aa=1,b=2", b"x" * 40]
    some = [b"a=1", b"x=0,bb=22,a=", b"bb=,q"]
    bodies = [some[0], none[0], none[1], some[1], none[2], none[3], some[2], none[4], none[1]]      # between, and as the last record
    for sep_len, keep_sep, suffix in ((1, True, b""), (1, False, b""), (2, True, b"!\n"), (0, True, b"")):
        data, offs = _pack(bodies, sep_len)
        want = _check(prog, blob, data, offs, names, lead=3, optional=opt, only=only, ofs=b"--" if only else None, sep_len=sep_len,
                      keep_sep=keep_sep, suffix=suffix)
        assert set(want[2]) == {0}
        tail = lambda b: (b"\r;"[:sep_len] if keep_sep else b"") + suffix               # noqa: E731
        assert want[0][want[1][1]:want[1][3]] == ((tail(b"") * 2) if only else none[0] + tail(b"") + none[1] + tail(b""))
        data, offs = _pack(none * 3, sep_len)                                           # a whole call without a document
        want = _check(prog, blob, data, offs, names, lead=11, optional=opt, only=only, ofs=b"--" if only else None, sep_len=sep_len,
                      keep_sep=keep_sep, suffix=suffix)
        assert set(want[2]) == {0} and (want[0] == b"".join(b + tail(b) for b in none * 3) if not only else len(want[0]) == 15 * len(tail(b"")))
    data, offs = _pack(none, 1)
    assert set(_check(prog, blob, data, offs, names, optional=[b"a"], only=only, sep_len=1)[2]) == {2}   # … and one in which every record is refused


# ---------------------------------------------------------------------------------------------------------- 5. quotes and escapes
def test_quotes_escapes_and_unquote():
    Q, E = b'"', b"\\"
    grow, mp = blob_of(GROW), blob_of(MAP)
    pg, pm = Program(grow), Program(mp)
    one = lambda p, b, body, names, **kw: _check(p, b, body, [0, len(body)], names, **kw)[0]   # noqa: E731
    assert one(pg, grow, b'msg="a b" k=v', [b"msg", b"k"], blanks=True, quote=Q) == b'msg=<"a b"> k=<v>'
    assert one(pg, grow, b'k="a=b,k=c",x=1', [b"k", b"x"], quote=Q) == b'k=<"a=b,k=c">,x=<1>'
    assert one(pg, grow, b'x="1,a=2",a=3', [b"a"], quote=Q) == b'x="1,a=2",a=<3>'          # C and F inside quotes
    assert one(pg, grow, b"a\\=b=c,a=d\\,e,f", [b"a"], escape=E) == b"a\\=b=c,a=<d\\,e>,f"   # … and behind escapes
    assert one(pg, grow, b'"k"=v k=w', [b"k"], blanks=True, quote=Q) == b'"k"=v k=<w>'      # keys are raw bytes
    assert one(pg, grow, b'"k"=v k=w', [b'"k"'], blanks=True, quote=Q) == b'"k"=<v> k=w'    # a key that is itself quoted
    assert one(pg, grow, b'a="x,\ny",b=2', [b"b"], quote=Q) == b'a="x,\ny",b=<2>'
    # --unquote: the program runs on the value's value, and outputs that need it are wrapped
    assert one(pm, mp, b'msg="a_b" k=x_y z=q', [b"msg", b"k"], blanks=True, quote=Q, unquote=True) == b'msg="a b" k="x y" z=q'
    assert one(pm, mp, b"k=a-b,m=a%b,n=ab", [b"k", b"m", b"n"], quote=Q, unquote=True) == b'k="a,b",m="a""b",n=ab'
    assert one(pm, mp, b"k=a-b,m=a_b", [b"k", b"m"], escape=E, unquote=True) == b"k=a\\,b,m=a b"
    assert one(pm, mp, b'k="a-b",m=a_b', [b"m", b"k"], quote=Q, unquote=True, only=[0, 1], ofs=b" ") == b'"a b" "a,b"'
    assert _check(pm, mp, b'k="a b"', [0, 7], [b"k"], quote=Q, unquote=True)[2:] == ([1], [1], [0], [1])   # S counts inside the value: a b
    r = random.Random(61)
    for quote, escape, blanks, pieces in ((Q, None, False, [b"a=1", b'a="x,y"', b'b="a=1"', b"b=a_b", b'"a"=1', b"ab", b'a=""', b"b=a%b", b"=", b'"']),
                                          (None, E, False, [b"a=1", b"a\\=b=2", b"b=x\\,y", b"b=a-b", b"\\a=1", b"a=\\", b"ab", b"b=a%b"]),
                                          (Q, E, True, [b"a=1", b'a="x y"', b"b=x\\ y", b'b="a\\"b"', b"b=a_b", b'"a b"=1', b"ab", b"a=", b"\\"])):
        glue = (b" ", b"\t", b"  ") if blanks else (b",",)
        bodies = [b"".join(r.choice(pieces) + r.choice(glue) for _ in range(r.randrange(0, 7))) + r.choice(pieces) * r.randrange(2) for _ in range(500)]
        data, offs = _pack(bodies, 1)
        for lead, unquote, optional, only in ((0, False, (), None), (7, True, (b"b",), None), (13, True, (b"a", b"b"), [1, 0, 1])):
            want = _check(pm, mp, data, offs, [b"a", b"b"], lead=lead, optional=optional, blanks=blanks, quote=quote, escape=escape, unquote=unquote,
                          only=only, ofs=b";" if only else None, sep_len=1)
            assert set(want[2]) >= {0, 1}


# ---------------------------------------------------------------------------------------------------------- 6. --only
def test_only_orders_repeats_and_skips():
    blob = blob_of(GROW)
    prog = Program(blob)
    names, opt = [b"ts", b"msg", b"lvl"], [b"msg"]
    bodies = [b"lvl=i,msg=hello,ts=1", b"ts=2,x=y,lvl=w", b"msg=m,ts=3", b"lvl=e,ts=4,msg=,msg=again"]
    data, offs = _pack(bodies, 1)
    for ofs in (b"", b" ", b"12345678"):
        want = _check(prog, blob, data, offs, names, lead=9, optional=opt, only=[0, 1, 2, 1, 0], ofs=ofs, sep_len=1)
        assert want[2] == [0, 0, 2, 0] and want[5][2] == 3
        assert want[0][:want[1][1]] == ofs.join([b"<1>", b"<hello>", b"<i>", b"<hello>", b"<1>"]) + b"\r"
        assert want[0][want[1][1]:want[1][2]] == ofs.join([b"<2>", b"<w>", b"<2>"]) + b"\r"      # the absent one in the middle: no doubled OFS
        assert want[0][want[1][3]:] == ofs.join([b"<4>", b"<>", b"<e>", b"<>", b"<4>"]) + b"\r"


# ---------------------------------------------------------------------------------------------------------- 7. sizes
def test_record_counts_around_the_block_and_scan_sizes():
    blob = blob_of(SOME)
    prog = Program(blob)
    r = random.Random(512)
    piece = lambda: r.choice([b"a=aa", b"b=ab", b"a=ba", b"b=", b"c=1", b"ab", b"a=a", b"=", b"b=bbb"])   # noqa: E731
    for n in (1, 63, 64, 65, 511, 512, 513, 1025):
        bodies = [b",".join(piece() for _ in range(r.randrange(0, 6))) for _ in range(n)]
        data, offs = _pack(bodies, 1)
        _check(prog, blob, data, offs, [b"a", b"b"], lead=n % 16, optional=[b"b"], sep_len=1, suffix=b"\n")
        _check(prog, blob, data, offs, [b"b", b"a"], lead=n % 16, optional=[b"a", b"b"], only=[1, 0], sep_len=1, keep_sep=False, suffix=b"\n")


def test_one_long_value_takes_the_route():
    blob = blob_of(GROW)
    prog = Program(blob)
    r = random.Random(3)
    long_value = bytes(r.choice(b"abc=") for _ in range(70 << 10))                       # above batch_doc_max (64 KiB)
    bodies = [b"k=1,m=2", b"m=3", b"k="] * 20 + [b"pre,m=0,k=" + long_value + b",post=1"] + [b"m=,k=9", b"", b"k=7,k=8"] * 20
    data, offs = _pack(bodies, 1)
    want = _check(prog, blob, data, offs, [b"k", b"m"], lead=7, optional=[b"m", b"k"], sep_len=1, suffix=b"|")
    assert prog.last_batch_stats.docs_routed == 1 and set(want[2]) == {0}
    assert want[0][want[1][60]:want[1][61]] == b"pre,m=<0>,k=<" + long_value + b">,post=1\r|"


# ---------------------------------------------------------------------------------------------------------- 8. caller buffers
@pytest.mark.parametrize("only", [None, [1, 0, 1]])
def test_size_query_capacity_and_an_unaligned_output(only):
    import torch
    blob = blob_of(SOME)
    prog = Program(blob)
    bodies = [b"a=aa,b=ab", b"x", b"b=bb,a=ba", b"", b"a=,b=", b"q=1,b=b", b"a=ab"] * 9
    data, offs = _pack(bodies, 2)
    kw = dict(optional=[b"a"], only=only, ofs=b", " if only else None, sep_len=2, suffix=b"\r\n!")
    want = _expected(blob, data, offs, [b"a", b"b"], **kw)
    need = len(want[0])
    assert set(want[2]) == {0, 1, 2} and need > 100
    v, o = _device(data, offs, 5)
    res = prog.run_batch_field_keys_tensor(v, o, [b"a", b"b"], fs=b",", **kw)           # out=None: the size query, then the exact size
    assert res[0].numel() == need and res[0].cpu().numpy().tobytes() == want[0] and res[1].tolist() == want[1]
    short = torch.full((need - 1,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(EngineError, match="too small: need %d bytes" % need):           # one byte short: KX_E_CAPACITY, nothing written
        prog.run_batch_field_keys_tensor(v, o, [b"a", b"b"], fs=b",", out=short, **kw)
    torch.cuda.synchronize()
    assert short.cpu().numpy().tobytes() == b"\xee" * (need - 1)
    for at in (0, 3, 13):                                                               # the exact capacity between guard bytes
        buf = torch.full((at + need + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        res = prog.run_batch_field_keys_tensor(v, o, [b"a", b"b"], fs=b",", out=buf[at:at + need], **kw)
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == b"\xee" * at + want[0] + b"\xee" * 64 and res[1].tolist() == want[1]
        assert res[2].tolist() == want[2] and res[5].tolist() == want[5]


# ---------------------------------------------------------------------------------------------------------- 9. windows, the binary
FLIP = open(program_path("flip_ab")).read()


def _stream():
    """About 13 KiB of logfmt-like lines over {a, b}; one line, and the selected value inside it, straddles the first 4 KiB boundary;
    lines with a rejected value, without a required key and without any pair in every window."""
    r = random.Random(4096)
    word = lambda: bytes(r.choice(b"ab") for _ in range(r.randrange(0, 7)))               # noqa: E731
    lines, n = [], 0
    while n < 13000:
        k = r.randrange(10)
        line = (b"" if k == 0 else b"ts=" + word() if k == 1 else b"msg=" + word() + b" ts=abc" if k == 2 else b"msg=" + word() + b"c ts=" + word() if k == 3
                else b" ".join(r.choice([b"ts=", b"msg=", b"lvl=", b"x", b"msg"]) + word() for _ in range(r.randrange(1, 8))) + b" msg=" + word())
        if n < 4096 - 30 <= n + len(line) + 1:
            line = b"ts=ab  msg=" + b"ab" * ((4096 - n) // 2) + b" lvl=b"
            assert n + 11 < 4096 - 8 and n + len(line) > 4096 + 8
        lines.append(line)
        n += len(line) + 1
    return b"\n".join(lines) + b"\n" + b"lvl=a  msg=abba"                                  # a tail without a separator


def _want_stream(blob, data, names, optional, only=None, ofs=None, chomp=False, ors=b""):
    offs = host.split_records_model(data, b"\n")
    tail = not data.endswith(b"\n")
    w = _expected(blob, data, offs, names, optional=optional, blanks=True, only=only, ofs=ofs, sep_len=1, last_whole=tail, keep_sep=not chomp, suffix=ors)
    err, res = [], []
    for i, (s, p, st, ff) in enumerate(zip(*w[2:])):
        if s == 2:
            err.append("Record %d has no field %s!\n" % (i + 1, names[ff - 1].decode()))
            res.append(("nofield", p, names[ff - 1]))
        elif s:
            err.append("Match error at input symbol %d in field %s of record %d!\n" % (p, names[ff - 1].decode(), i + 1))
            res.append((p, st, names[ff - 1]))
        else:
            res.append(w[0][w[1][i]:w[1][i + 1]])
    return w[0], "".join(err).encode(), res


def test_run_records_fd_in_small_windows(tmp_path):
    blob = blob_of(FLIP)
    data = _stream()
    (tmp_path / "in").write_bytes(data)
    for kw in (dict(fields=[b"msg"]), dict(fields=[b"ts", b"msg"], optional=[b"ts"]), dict(fields=[b"msg", b"ts", b"msg"], optional=[b"ts"], only=True, ofs=b"|", chomp=True, ors=b";\n")):
        names = list(dict.fromkeys(kw["fields"]))
        only = [names.index(n) for n in kw["fields"]] if kw.get("only") else None
        out, err, res = _want_stream(blob, data, names, kw.get("optional", ()), only, kw.get("ofs"), kw.get("chomp", False), kw.get("ors", b""))
        kinds = {"nofield" if r[0] == "nofield" else "rejected" if isinstance(r, tuple) else "ok" for r in res}
        assert kinds == {"ok", "rejected", "nofield"} and b"in field" in err and b"has no field msg!" in err
        for window in (4096, 1 << 20):
            prog = Program(blob, window_bytes=window)
            with open(tmp_path / "in", "rb") as fi, open(tmp_path / "out", "wb") as fo, open(tmp_path / "err", "wb") as fe:
                st = prog.run_records_fd(fi.fileno(), fo.fileno(), report_fd=fe.fileno(), blanks=True, keys=b"=", **kw)
            assert (tmp_path / "err").read_bytes() == err, (kw, window)
            assert (tmp_path / "out").read_bytes() == out, (kw, window)
            assert st["rejected"] and st["records"] == len(res) and st["records_rejected"] == sum(1 for r in res if isinstance(r, tuple))
            assert window > 4096 or st["windows"] >= 3
        got = Program(blob).run_records(data, blanks=True, keys=b"=", **kw)
        got = [("nofield", g.fields, g.field) if isinstance(g, NoFieldError) else (g.pos, g.stage, g.field) if isinstance(g, MatchError) else g for g in got]
        assert got == res, (kw, next((i, g, w) for i, (g, w) in enumerate(zip(got, res)) if g != w))
    assert Program(blob).run_records(b"", fields=[b"a"], keys=b"=") == []


LOG = (b'ts=2026-10-20T19:09:00Z level=info msg="cache  MISS for /a/b" dur=12ms\n'
       b'ts=2026-10-20T19:09:01Z level=warn dur=7ms msg=Retry msg="not this one"\n'
       b'ts=2026-10-20T19:09:02Z level=info msg="caf\xc3\xa9"\n'
       b'ts=2026-10-20T19:09:03Z level=info dur=1ms\n')


def test_the_produced_binary(tmp_path_factory):
    flip = single._bin(tmp_path_factory, FLIP)
    r = single._run_bin(flip, ["--records", "--keys", "--field=k", "--fs=,"], b"x=1,k=abba,k=ab\n", 1 << 30)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"x=1,k=baab,k=ab\n", b"")
    r = single._run_bin(flip, ["--records", "--field=m,k?,m", "--keys=:", "--blanks", "--only", "--ofs=|", "--chomp", "--ors=;"],
                        b"k:a m:ab\nm:b\nk:a\n\nm:abc k:b\nm:", 4096)
    assert (r.returncode, r.stdout) == (1, b"ba|b|ba;a|a;|;")
    assert r.stderr == b"Record 3 has no field m!\nRecord 4 has no field m!\nMatch error at input symbol 2 in field m of record 5!\n"
    r = single._run_bin(flip, ["--records", "--keys", "--field=\\x01k", "--fs=,"], b"k=a\n", 4096)
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"Record 1 has no field \\x01k!\n")
    data = _stream()
    out, err, _ = _want_stream(blob_of(FLIP), data, [b"ts", b"msg"], [b"ts"])
    for window in (4096, 1 << 30):
        r = single._run_bin(flip, ["--records", "--field=ts?,msg", "--keys", "--blanks"], data, window)
        assert (r.returncode, r.stderr, r.stdout) == (1, err, out), window
    # the example: the msg of a logfmt line, unquoted, rewritten and quoted again as it needs
    src = open(os.path.join(build.PKG, "examples", "logfmt_msg.kex")).read()
    exe = single._bin(tmp_path_factory, src)
    r = single._run_bin(exe, ["--records", "--quote", "--blanks", "--keys", "--field=msg", "--unquote"], LOG, 1 << 30)
    blob = blob_of(src)
    want = _expected(blob, LOG, host.split_records_model(LOG, b"\n"), [b"msg"], blanks=True, quote=b'"', unquote=True, sep_len=1)
    assert r.stdout == want[0] and want[2] == [0, 0, 1, 2]
    assert r.stdout == (b'ts=2026-10-20T19:09:00Z level=info msg="cache MISS for /a/b" dur=12ms\n'
                        b'ts=2026-10-20T19:09:01Z level=warn dur=7ms msg=Retry msg="not this one"\n')
    assert r.stderr == b"Match error at input symbol 3 in field msg of record 3!\nRecord 4 has no field msg!\n" and r.returncode == 1
