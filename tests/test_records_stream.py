"""CPU: the composed model of record mode (recstream.stream_model) and the generators of the record-stream tests.  The model is
held against what the repository already states literally — the README's examples and the stdout / stderr triples of the per-feature
tests — and against host.py's models on single-option streams; every option set passes the argument checks of the drivers; what the
streams and the seam probes hold is counted from the model and asserted against recstream.FLOORS."""
import collections
import os

import pytest
import recstream as rs
from conftest import blob_of

from kleenexlang_amd import build, host
from kleenexlang_amd.host import Program

SETS = rs.option_sets()
WHOLE = 'main := ("[" /[a-z,;"]+/ "]" | /\\\\/ | ~/\\n/ "\\\\n" | ~/\\r/ "\\\\r")*\n'    # (test_records_field_gpu.WHOLE)
LOGFMT = open(os.path.join(build.PKG, "examples", "logfmt_msg.kex")).read()
LOG = (b'ts=2026-10-20T19:09:00Z level=info msg="cache  MISS for /a/b" dur=12ms\n'
       b'ts=2026-10-20T19:09:01Z level=warn dur=7ms msg=Retry msg="not this one"\n'
       b'ts=2026-10-20T19:09:02Z level=info msg="caf\xc3\xa9"\n'
       b'ts=2026-10-20T19:09:03Z level=info dur=1ms\n')
O = rs.Options


def _blob(opt):
    return blob_of(rs.PROGRAMS[opt.prog])


def _model(opt, data):
    return rs.stream_model(_blob(opt), data, opt)


# ---------------------------------------------------------------------------------------------------------- 1. literal cases
# (source, keywords, stdin, stdout, stderr): the README's examples of record mode, then the triples that test_the_produced_binary,
# test_binary_short_streams and test_binary_small_examples of the per-feature GPU files state for the binary
LITERAL = [
    (rs.FLIP, dict(field=2, fs=b","), b"id1,abba,x\nid2,bab,y\n", b"id1,baab,x\nid2,aba,y\n", b""),
    (rs.FLIP, dict(fields=[2, (4, None)], fs=b","), b"a,abba,b,bab,ab\n", b"a,baab,b,aba,ba\n", b""),
    (rs.FLIP, dict(quote=b'"', field=2, fs=b",", unquote=True), b'"id1","abba","x"\n', b'"id1","baab","x"\n', b""),
    (rs.FLIP, dict(quote=b'"', field=2, fs=b","), b'"id1","abba","x"\n', b"", b"Match error at input symbol 0 in record 1!\n"),
    (rs.FLIP, dict(field=2, blanks=True), b"  a   abba\tb \n", b"  a   baab\tb \n", b""),
    (rs.FLIP, dict(fields=[4, 2], fs=b",", only=True, ofs=b"\t"), b"a,abba,b,bab\n", b"aba\tbaab\n", b""),
    (rs.FLIP, dict(header=1, fields=[b"name"], fs=b","), b"id,name,city\n1,abba,x\n2,bab,y\n", b"id,name,city\n1,baab,x\n2,aba,y\n", b""),
    (LOGFMT, dict(quote=b'"', blanks=True, keys=b"=", fields=[b"msg"], unquote=True), b'ts=1 level=info msg="a  b" msg=x\n',
     b'ts=1 level=info msg="a b" msg=x\n', b""),
    (LOGFMT, dict(quote=b'"', blanks=True, keys=b"=", fields=[b"msg"], unquote=True), LOG,
     b'ts=2026-10-20T19:09:00Z level=info msg="cache MISS for /a/b" dur=12ms\nts=2026-10-20T19:09:01Z level=warn dur=7ms msg=Retry msg="not this one"\n',
     b"Match error at input symbol 3 in field msg of record 3!\nRecord 4 has no field msg!\n"),
    (rs.FLIP, dict(keys=b"=", fields=[b"k"], fs=b","), b"x=1,k=abba,k=ab\n", b"x=1,k=baab,k=ab\n", b""),
    (rs.FLIP, dict(fields=[b"m", b"k", b"m"], optional=(b"k",), keys=b":", blanks=True, only=True, ofs=b"|", chomp=True, ors=b";"),
     b"k:a m:ab\nm:b\nk:a\n\nm:abc k:b\nm:", b"ba|b|ba;a|a;|;",
     b"Record 3 has no field m!\nRecord 4 has no field m!\nMatch error at input symbol 2 in field m of record 5!\n"),
    (rs.FLIP, dict(keys=b"=", fields=[b"\x01k"], fs=b","), b"k=a\n", b"", b"Record 1 has no field \\x01k!\n"),
    (WHOLE, dict(header=5, fields=[b"name"], fs=b";"), b"a;b\nc;d\ne", b"a;b\nc;d\ne", b""),
    (WHOLE, dict(header=5, fields=[b"name"], fs=b";", chomp=True, ors=b"|"), b"a;b\nc;d\ne", b"a;b|c;d|e|", b""),
    (WHOLE, dict(header=5, fields=[2, 1], fs=b";", only=True), b"a;b\nc;d\n", b"b;a\nd;c\n", b""),
    (WHOLE, dict(header=5, fields=[b"name"], fs=b";", only=True), b"a;b\nc;d\n", b"", b""),
    (WHOLE, dict(header=1, fields=[b"name"], fs=b";"), b"", b"", b""),
    (WHOLE, dict(header=3), b"", b"", b""),
    (WHOLE, dict(header=1, fields=[b"name"], fs=b";"), b"id;name", b"id;name", b""),
    (WHOLE, dict(header=1, fields=[b"name", b"id"], fs=b";", only=True, chomp=True, ors=b"\n"), b"id;name", b"name;id\n", b""),
    (WHOLE, dict(header=1), b"Id\nab\n1\n", b"Id\n[ab]\\n", b"Match error at input symbol 0 in record 3!\n"),
    (WHOLE, dict(header=1, fields=[b"name"], fs=b";"), b"id;name\nab;cd\n", b"id;name\nab;[cd]\n", b""),
    (WHOLE, dict(quote=b'"', header=1, fields=[b"city", b"name"], fs=b",", unquote=True, only=True, ofs=b"\t"), b'id,"name",city\n1,"ab,c",x\n',
     b'city\t"name"\n[x]\t"[ab,c]"\n', b""),
    (WHOLE, dict(rs=b"\r\n", header=1, fields=[b"name"], fs=b";"), b"id;name\r\nab;cd\r\n", b"id;name\r\nab;[cd]\r\n", b""),
    (WHOLE, dict(header=1, fields=[b"name\r"], fs=b";"), b"id;name\r\nab;cd\r\n", b"id;name\r\nab;[cd]\\r\n", b""),
    (WHOLE, dict(header=1, fields=[3, 1], fs=b";", only=True), b"id;name\nab;cd;e\n", b"[e];[ab]\n", b"Record 1 has no field 3!\n"),
]


@pytest.mark.parametrize("k", range(len(LITERAL)))
def test_the_model_gives_the_literal_expectations(k):
    src, kw, data, out, err = LITERAL[k]
    got = rs.stream_model(blob_of(src), data, O(**kw))
    assert (got[0], got[1]) == (out, err)
    assert got[3]["rejected"] == bool(err) and got[3]["records_rejected"] == err.count(b"\n") and got[3]["header_error"] is None


def test_the_model_gives_the_literal_header_errors():
    """a name that no cell has: nothing for record N or behind it; the records in front of it are copied — or, projected, held"""
    data = b"id;name\n" + b"ab;cd\n" * 50
    blob = blob_of(WHOLE)
    out, err, res, st = rs.stream_model(blob, data, O(header=1, fields=[b"id", b"nam\0e"], fs=b";"))
    assert (out, err, res, st["header_error"]) == (b"", b"", None, b"nam\0e") and rs._printable(b"nam\0e") == "nam\\x00e"
    opt = O(header=2, fields=[b"city"], fs=b";")
    out, err, res, st = rs.stream_model(blob, b"first\n" + data, opt)
    assert (out, res, st["header_error"]) == (b"first\n", None, b"city")
    assert rs.written_before(b"first\n" + data, opt, 4096, st) == b""                    # (record 2 ends in the first window: nothing is written)
    long = b"first\n" + b"#" * 5000 + b"\nid;name\n" + b"ab;cd\n" * 50                     # … but here record 1 is done a window earlier
    for only, want in ((False, b"first\n"), (True, b"")):
        opt = O(header=3, fields=[b"city"], fs=b";", only=only)
        st = rs.stream_model(blob, long, opt)[3]
        assert st["header_error"] == b"city" and rs.written_before(long, opt, 4096, st) == want
        assert rs.written_before(long, opt, 8192, st) == b""


# ---------------------------------------------------------------------------------------------------------- 2. single options
def _direct(blob, docs):
    out = [rs._run(blob, d) for d in docs]
    return [w if isinstance(w, bytes) else ("match", w[0], w[1], None) for w in out]


@pytest.mark.parametrize("name", ["byte", "quote", "escape", "quote+escape", "rs", "chomp", "ors", "field", "fields", "blanks", "unquote", "only", "header", "keys"])
def test_single_option_streams_are_the_feature_model(name):
    """one option at a time (with what it cannot come without): the model's record list is what the feature's own host model gives"""
    Q, E = b'"', b"\\"
    kw = {"byte": {}, "quote": dict(quote=Q), "escape": dict(escape=E), "quote+escape": dict(quote=Q, escape=E), "rs": dict(rs=b";:"),
          "chomp": dict(chomp=True), "ors": dict(ors=b"<<eor>>\n"), "field": dict(field=2, fs=b","), "fields": dict(fields=[2, (4, None)], fs=b","),
          "blanks": dict(fields=[1, 3], blanks=True), "unquote": dict(quote=Q, fields=[1, 3], fs=b",", unquote=True),
          "only": dict(fields=[3, 1, 3], fs=b",", only=True), "header": dict(header=3), "keys": dict(fields=[b"k", b"m"], keys=b"=", fs=b",")}[name]
    opt = O("map" if name == "unquote" else "grow" if name == "rs" else "flip", **kw)
    blob = _blob(opt)
    for seed in (0, 1):
        data = rs.stream(opt, seed, 6000)
        out, err, res, st = _model(opt, data)
        offs, tail = st["offsets"], st["tail"]
        sl = len(opt.sep_bytes)
        if name in ("byte", "quote", "escape", "quote+escape", "rs", "ors", "chomp", "header"):
            want_offs = (host.split_rs_records_model(data, b";:")[0] if name == "rs" else
                         host.split_escaped_records_model(data, b"\n", kw.get("quote"), E)[0] if "escape" in name else
                         host.split_records_model(data, b"\n", kw.get("quote")))
            assert offs == list(want_offs) and tail == (seed == 1)
            docs = host.chomp_records_model(data, offs, 1 if name == "chomp" else 0, tail)
            want = _direct(blob, docs)
            want = [w + opt.ors if isinstance(w, bytes) else w for w in want]
            if name == "header":
                want[:3] = [data[offs[i]:offs[i + 1]] for i in range(3)]
            assert res == want
            continue
        want = []
        if name == "field":
            for m in host.field_records_model(data, offs, sl, tail, 2, b","):
                w = rs._run(blob, m[1]) if isinstance(m, tuple) else None
                want.append(("nofield", m, None) if w is None else ("match", w[0], w[1], None) if isinstance(w, tuple) else m[0] + w + m[2] + m[3])
        elif name == "keys":
            for m in host.keyed_records_model(data, offs, sl, tail, [b"k", b"m"], b"=", b","):
                if isinstance(m, int):
                    want.append(("nofield", m, [b"k", b"m"][rs._lowbit(3 & ~m)]))
                    continue
                ws = [rs._run(blob, v) for _, v in m[1]]
                bad = next((j for j, w in enumerate(ws) if isinstance(w, tuple)), None)
                want.append(("match", ws[bad][0], ws[bad][1], [b"k", b"m"][m[1][bad][0]]) if bad is not None else
                            b"".join(g + w for g, w in zip(m[0], ws + [b""])) + m[2])
        else:
            ranges = host._check_field_ranges(kw["fields"])
            recs = (host.blank_field_list_records_model(data, offs, sl, tail, ranges) if name == "blanks" else
                    host.field_list_records_model(data, offs, sl, tail, ranges, b",", kw.get("quote")))
            for m in recs:
                if isinstance(m, int):
                    want.append(("nofield", m, None))
                    continue
                ws = [rs._run(blob, host.unquote_field_model(f, Q) if name == "unquote" else f) for _, f in m[1]]
                bad = next((j for j, w in enumerate(ws) if isinstance(w, tuple)), None)
                if bad is not None:
                    want.append(("match", ws[bad][0], ws[bad][1], m[1][bad][0]))
                    continue
                if name == "unquote":
                    ws = [host.requote_field_model(w, f[:1] == Q, b",", Q, None, b"\n") for w, (_, f) in zip(ws, m[1])]
                if name == "only":
                    by = {K: w for (K, _), w in zip(m[1], ws)}
                    want.append(by[3] + b"," + by[1] + b"," + by[3] + m[2])
                else:
                    want.append(b"".join(g + w for g, w in zip(m[0], ws + [b""])) + m[2])
        assert res == want, next((i, a, b) for i, (a, b) in enumerate(zip(res, want)) if a != b)
        kinds = {type(r) if isinstance(r, bytes) else r[0] for r in res}
        assert kinds == ({bytes, "match", "nofield"})


def test_only_is_the_projection_model():
    """…and beside the inline projection: host.project_records_model gives the cells the model joins"""
    opt = O("flip", fields=[(4, None), 1, (1, 2)], fs=b",", only=True, ofs=b"|", chomp=True)
    data = rs.stream(opt, 0, 6000)
    _, _, res, st = _model(opt, data)
    blob = _blob(opt)
    n = 0
    for r, m in zip(res, host.project_records_model(data, st["offsets"], 1, st["tail"], opt.fields, b",")):
        if isinstance(m, int):
            assert r == ("nofield", m, None)
        elif all(isinstance(rs._run(blob, c), bytes) for _, c in m[0]):
            assert r == b"|".join(rs._run(blob, c) for _, c in m[0])
            n += 1
    assert n > 20


# ---------------------------------------------------------------------------------------------------------- 3. validity
def check_arguments(opt):
    """the argument checks of Program.run_records_fd, in its order, up to the call into the library: the static methods of Program
    and the checks of host.py, none of which needs a GPU"""
    what = "run_records_fd"
    sep, quote, escape, rs_, fs, field, fields = opt.sep, opt.quote, opt.escape, opt.rs, opt.fs, opt.field, opt.fields
    keyed = Program._check_keys(what, opt.keys, opt.optional, field, fields, fs, opt.blanks, quote, escape, sep, rs_, opt.header)
    if keyed is not None:
        fields = [1] * len(keyed[2])
    header, named = host._check_header(what, opt.header, fields)
    if named:
        fields = [1 if isinstance(it, (bytes, bytearray)) else it for it in fields]
    items, ofs = Program._check_only(what, opt.only, opt.ofs, field, fields, fs, opt.blanks)
    if items is not None:
        field, fields = None, list(items)
    field, fields = Program._check_unquote(what, opt.unquote, field, fields, quote, escape)
    field, fields, fs = Program._check_blanks(what, opt.blanks, field, fields, fs, sep, quote, escape, rs_)
    if rs_ is not None:
        Program._check_rs_alone(rs_, sep, quote, escape, what)
    s = host._check_sep(sep)
    q = None if quote is None else host._check_quote(quote, sep)
    e = None if escape is None else host._check_escape(escape, sep, quote)
    host._check_chomp(opt.chomp), host._check_ors(opt.ors)
    assert not (field is not None and fields is not None)
    if field is not None:
        host._check_field(field)
    if fields is not None:
        host._check_field_ranges(fields)
    if (field is not None or fields is not None) and not opt.blanks:
        host._check_fs(fs, quote, escape, sep if rs_ is None else rs_ if len(rs_) == 1 else None)
    if items is not None and opt.unquote:
        host._check_ofs_codec(what, ofs, q, e, bytes([s]) + (b"\t" if opt.blanks else b""))
    if keyed is None and opt.optional:
        raise ValueError("optional= needs keys=")


def test_every_option_set_passes_the_argument_checks():
    for opt in SETS + rs.sweep_sets():
        check_arguments(opt)                                                            # (a refusal raises: nothing is skipped or filtered)
        text = opt._list_text() if opt.fields is not None else None
        if opt.keys is not None:                                                        # … and the binary's spelling reads back as the keywords
            names, mask, items = host.parse_field_keys(text)
            assert [names[i] for i in items] == list(opt.fields) and {n for t, n in enumerate(names) if mask >> t & 1} == set(opt.optional)
        elif opt.named:
            assert list(host.parse_field_names(text)) == [tuple(it) if isinstance(it, list) else it for it in opt.fields]
        elif opt.fields is not None:
            assert host.parse_field_list(text) == host._check_field_ranges(opt.fields)
        assert opt.args()[0] == "--records" and all(a.startswith("--") for a in opt.args())
    with pytest.raises(ValueError):
        check_arguments(O(rs=b";:", quote=b'"'))                                        # (the checks do refuse)
    with pytest.raises(ValueError):
        check_arguments(O(fields=[b"k"], keys=b"=", fs=b",", header=1))


def test_the_product_holds_every_pairing_and_a_pairwise_overlay():
    assert len(SETS) == 163 and len({id(o) for o in SETS}) == len(SETS)
    pairs = collections.Counter((o.splitter, o.route) for o in SETS)
    splitters = [s for s, _ in rs.SPLITTERS]
    assert splitters == ["byte", "quoted", "escq", "esc", "rs1", "rsn", "rso"]
    for route, needs, kw in rs.ROUTES:
        ok = [s for s, skw in rs.SPLITTERS if not needs or "quote" in skw or "escape" in skw]
        assert len(ok) == (3 if needs else 7) and all(pairs[s, route] >= 1 for s in ok)
        mine = [o for o in SETS[:-3] if o.route == route]
        dims = lambda o: (o.chomp, len(o.ors), o.header, o.named)                         # noqa: E731
        have = {(a, dims(o)[a], b, dims(o)[b]) for o in mine for a in range(4) for b in range(a + 1, 4)}
        chomps, orss = (False, True), (0, 1, 8)
        headers = (0,) if "keys" in kw else (0, 1, 3)
        for c in chomps:
            for s in orss:
                assert (0, c, 1, s) in have, (route, c, s)
                for h in headers:
                    assert (0, c, 2, h) in have and (1, s, 2, h) in have, (route, c, s, h)
                    if h and "fields" in kw:
                        for nm in (False, True):
                            assert (2, h, 3, nm) in have and (0, c, 3, nm) in have and (1, s, 3, nm) in have, (route, c, s, h, nm)
    assert len(pairs) == 7 * 10 + 3 * 6
    flat = [it for o in SETS if o.fields for it in o.fields]
    assert any(isinstance(it, tuple) and it[1] is None for it in flat)                   # an open range
    assert any(o.only and len(set(map(str, o.fields))) < len(o.fields) for o in SETS)    # a repeated item
    assert any(o.only and o.fields == [(4, 5), (5, 6)] for o in SETS)                    # overlapping items
    assert {o.prog for o in SETS} == set(rs.PROGRAMS)
    sweep = rs.sweep_sets()
    assert {(o.splitter, o.route) for o in sweep} >= set(pairs) and len(sweep) == len(pairs) + 14
    assert {(o.splitter, o.header) for o in sweep if o.named} == {(s, N) for s in splitters for N in (1, 3)}


def test_the_programs_are_the_ones_the_record_tests_use():
    import test_records_keys_gpu as keys
    assert (rs.GROW, rs.SOME, rs.MAP, rs.FLIP) == (keys.GROW, keys.SOME, keys.MAP, keys.FLIP)
    assert "@" in rs.ACTION and "!" in rs.ACTION                                         # a register and its output action


# ---------------------------------------------------------------------------------------------------------- 4. populations
def test_populations(capsys):
    """What the product's streams hold, counted from the model (MEASURED: the minimum over the 160 option sets that end without a header error, and both seeds when
    the floors were set — 90 accepted, 72 with a rejected value, 93 too short or without a key, 26 empty records a stream; in the
    poorest 4 KiB window 3 accepted and 9 rejected ones, the too short among them).  Every window of every stream has an accepted and a rejected record."""
    low = collections.defaultdict(lambda: 10 ** 9)
    for opt in SETS:
        for seed in (0, 1):
            data = rs.stream(opt, seed)
            assert data == rs.stream(opt, seed) and data != rs.stream(opt, seed + 2) and 13000 <= len(data) < 13400    # deterministic
            out, err, res, st = _model(opt, data)
            assert st["tail"] == bool(seed)
            if st["header_error"] is not None:
                assert opt in SETS[-3:] and res is None
                continue
            total, per = rs.populations(data, opt, res, st)
            assert len(per) == 4 and total.get("header", 0) == opt.header
            for k in ("accepted", "rejected", "empty") + (("short",) if opt.route != "whole" else ()):
                low[k] = min(low[k], total.get(k, 0))
            for w, p in enumerate(per):
                low["window accepted"] = min(low["window accepted"], p.get("accepted", 0))
                low["window rejected"] = min(low["window rejected"], p.get("rejected", 0) + p.get("short", 0))
            win = rs.window_of(st["offsets"], st["tail"], len(data), 4096)
            assert any(a // 4096 < w for a, w in zip(st["offsets"], win))                 # a record straddles an edge
    with capsys.disabled():
        print("\nrecord-stream populations (minimum over the option sets):", dict(low))
    for k, floor in rs.FLOORS["streams"].items():
        assert floor >= 1 and low[k] >= floor, (k, low[k], floor)
    assert set(rs.FLOORS["streams"]) == {"accepted", "rejected", "short", "empty", "window accepted", "window rejected"}


def test_probe_populations(capsys):
    """At how many positions of each probe the state matters (MEASURED in FLOORS["probes"]): `cut`, positions at which the edge
    falls inside a record, which must then be carried; `split`, positions at which the second window's split differs when the carry
    — parity, escape state, separator context — is dropped.  Every probe has a cut position; every probe of a splitter's own
    construct has a split position.  The filler's last record ends directly before the probe."""
    low, lengths, streams = {}, {}, 0
    for opt in rs.sweep_sets():
        for probe in rs.seam_probes(opt):
            if opt.named and probe[1] != "header":
                continue
            ss = rs.seam_streams(opt, probe)
            assert [p for p, _ in ss] == list(range(len(probe[2]) + 1)) and len(probe[2]) <= 48
            assert ss == rs.seam_streams(opt, probe)
            streams += len(ss)
            for pos, data in ss:
                assert data[4096 - pos:4096 - pos + len(probe[2])] == probe[2] and 9216 <= len(data) < 9400
                if probe[1] == "records":
                    assert 4096 - pos in rs.split_model(data, opt)[0], (opt, probe[0], pos)
            split, cut = rs.carry_positions(opt, ss)
            a, b = low.get(probe[0], (10 ** 9, 10 ** 9))
            low[probe[0]] = (min(a, split), min(b, cut))
            lengths[probe[0]] = max(lengths.get(probe[0], 0), len(probe[2]))
    with capsys.disabled():
        print("\nseam probes (minimum split / cut positions):", low, "longest:", lengths, "streams:", streams)
    assert set(low) == set(rs.FLOORS["probes"])
    for name, (split, cut) in rs.FLOORS["probes"].items():
        assert cut >= 1 and low[name][0] >= split and low[name][1] >= cut, (name, low[name])
        assert split >= 1 or name in ("blanks", "key and value", "header names", "plain record")


def test_the_split_model_carries_what_the_windows_carry():
    """window by window from the carry of the window before, the model's split is the whole stream's: what RecordsRun::window hands on"""
    for opt in SETS[::7] + rs.sweep_sets()[::9]:
        data = rs.stream(opt, 1, 9000)
        whole, tail, _ = rs.split_model(data, opt)
        bounds, carry = set(), None
        for at in range(0, len(data), 4096):
            offs, t, carry = rs.split_model(data[at:at + 4096], opt, carry)
            bounds |= {at + x for x in (offs[1:] if not t else offs[1:-1])}
        assert bounds == set(whole[1:-1]) and tail
