"""GPU: field mode on unquoted values — kx_run_batch_field_values (Program.run_batch_field_values_tensor),
Program.run_records(unquote=True) and `BIN --records … --quote|--escape --field=K|LIST --unquote`.  Every record's expected result
is built in Python: host.field_list_records_model cuts the record, host.unquote_field_model gives each selected field's value,
the CPU oracle runs on the VALUE (test_records_field_gpu's cache), host.requote_field_model spells its output, and gaps +
spellings + separator + suffix are spliced here."""
import csv
import ctypes
import io
import os
import random

import pytest
from conftest import blob_of

import test_records_field_gpu as single
import test_records_field_list_gpu as flist
from kleenexlang_amd import host
from kleenexlang_amd.host import MatchError, NoFieldError, Program

pytestmark = pytest.mark.gpu

FS, P, _want = single.FS, host.parse_field_list, single._want
Q, E = b'"', b"\\"
MODES = {"quoted": dict(quote=Q), "both": dict(quote=Q, escape=E), "escaped": dict(escape=E)}
# outputs that need quoting: a quote, the field separator, the record separator, the escape byte; a digit is rejected
QPROG = 'main := (~/a/ "\\"" | ~/b/ ";" | ~/c/ "\\n" | ~/d/ "\\\\" | /[e-z ]/)*\n'
COPY = single.COPY
IDENT = 'main := (/[^\\n]/ | /\\n/)*\n'
U, R = host.unquote_field_model, host.requote_field_model


def _expected(blob, data, offs, ranges, fs=FS, quote=None, escape=None, special=b"\n", sep_len=0, last_whole=False, keep_sep=True, suffix=b""):
    """(output bytes, output offsets, status, fail_pos, fail_stage, fail_field): test_records_field_list_gpu's, on values."""
    out, ooff, status, fpos, fstage, ffield = [], [0], [], [], [], []
    for m in host.field_list_records_model(data, offs, sep_len, last_whole, ranges, fs, quote, escape):
        if isinstance(m, int):
            s = (m, 2, 0, host.field_list_missing(ranges, m))
        else:
            gaps, fields, sep = m
            res = [_want(blob, U(f, quote, escape)) for _, f in fields]
            bad = next((j for j, w in enumerate(res) if isinstance(w, tuple)), None)         # the lowest rejected field
            s = (res[bad][0], 1, res[bad][1], fields[bad][0]) if bad is not None else None
        if s is not None:
            fpos.append(s[0]); status.append(s[1]); fstage.append(s[2]); ffield.append(s[3])
            ooff.append(ooff[-1])
        else:
            status.append(0); fpos.append(0); fstage.append(0); ffield.append(0)
            sp = [R(w, quote is not None and f[:1] == quote, fs, quote, escape, special) for w, (_, f) in zip(res, fields)]
            out.append(b"".join(g + w for g, w in zip(gaps, sp + [b""])) + (sep if keep_sep else b"") + suffix)
            ooff.append(ooff[-1] + len(out[-1]))
    return b"".join(out), ooff, status, fpos, fstage, ffield


def _check(prog, blob, data, offs, ranges, lead=0, **kw):
    import torch
    want = _expected(blob, data, offs, ranges, **kw)
    v, o = single._device(data, offs, lead)
    kw.setdefault("fs", FS)
    res = prog.run_batch_field_values_tensor(v, o, ranges, **kw)
    torch.cuda.synchronize()
    got = (res[0].cpu().numpy().tobytes(),) + tuple(t.tolist() for t in res[1:])
    ctx = (ranges, lead, kw)
    rec = lambda i: data[offs[min(i, len(offs) - 2)]:offs[min(i, len(offs) - 2) + 1]][:80]   # noqa: E731
    for name, k in (("status", 2), ("fail_pos", 3), ("fail_stage", 4), ("fail_field", 5), ("out_off", 1)):
        if got[k] != want[k]:
            i = next(j for j in range(len(want[k])) if got[k][j] != want[k][j])
            raise AssertionError("%s[%d]: got %r, want %r (record %r, %r)" % (name, i, got[k][i], want[k][i], rec(i), ctx))
    assert got[0] == want[0], (ctx, next((i, rec(i), got[0][want[1][i]:want[1][i + 1]][:80], want[0][want[1][i]:want[1][i + 1]][:80])
                                         for i in range(len(offs) - 1) if got[0][want[1][i]:want[1][i + 1]] != want[0][want[1][i]:want[1][i + 1]]))
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.out_bytes) == (len(offs) - 1, sum(1 for s in want[2] if s), len(want[0]))
    return want


def _raw_fields(r, mode):
    """Spellings of one field for QPROG, as a writer and as a careless hand would leave them: 0, 1 and 2 bytes; values whose outputs
    need quoting; "" and \\" pairs at the start, in the middle and at the end; a quote in the middle of a field, an unclosed one,
    a last escape byte alone; one field in 12 holds a digit, which QPROG rejects."""
    q, e = "quote" in MODES[mode], "escape" in MODES[mode]
    L = r.choice((0, 0, 1, 2, 3, 5, 9, 14, 15, 16, 17, 31, 33))
    v = bytes(r.choice(b"abcdefgh xyz") for _ in range(L))
    if r.randrange(12) == 0:
        v += b"7" + v[:3]
    kind = r.randrange(8)
    if kind < 3:
        return v if not (q and b'"' in v) else b""                                       # as it is
    if kind == 3 and q:
        return b'"' + v + b'"'                                                          # quoted
    if kind == 4 and q:
        pair = b'\\"' if e and r.randrange(2) else b'""'
        at = r.choice((0, len(v) // 2, len(v)))
        return b'"' + v[:at] + pair + v[at:] + (pair if r.randrange(3) == 0 else b"") + b'"'
    if kind == 5 and e:
        at = r.choice((0, len(v) // 2, len(v)))
        return v[:at] + r.choice((b"\\;", b"\\\\", b"\\\n", b"\\e")) + v[at:]
    if kind == 6:
        return r.choice(((b'e"f;g"h', b'"efg', b'""', b'""""', b'"') if q else ()) + ((b"\\", b"e\\", b"\\\\") if e else ()))
    return v[:2]


def _bodies(r, mode, n):
    bodies = [FS.join(_raw_fields(r, mode) for _ in range(r.choice((1, 2, 3, 3, 4, 5, 6)))) for _ in range(n)]
    bodies[0] = bodies[-1] = FS.join([b"e", b'"1"' if "quote" in MODES[mode] else b"1", b"f", b"g"])   # rejected first and last
    bodies[n // 2:n // 2 + 3] = [b"", b"", FS * 3]
    return bodies


# ---------------------------------------------------------------------------------------------------------- 1. model + oracle
@pytest.mark.parametrize("mode", sorted(MODES))
def test_values_against_models_and_oracle(mode):
    blob = blob_of(QPROG)
    prog = Program(blob)
    kw = MODES[mode]
    r = random.Random(40 + len(mode))
    bodies = _bodies(r, mode, 700)
    seen, pairs, edges = set(), set(), set()
    for lead in range(16):                                                              # every alignment of the values tensor's first byte
        text = ("2,4", "1-3", "2-", "1-", "1,3-4,6-", "3")[lead % 6]
        sep_len, suffix = (1, 0, 1, 2)[lead % 4], (b"", b"|", b"12345678")[lead % 3]
        last_whole, keep_sep = bool(lead & 1), bool(lead & 2) ^ bool(lead & 8)
        data, offs = host.pack_batch([b + b"\n\r"[:sep_len] for b in bodies])
        want = _check(prog, blob, data, offs, P(text), lead=lead, sep_len=sep_len, last_whole=last_whole, keep_sep=keep_sep, suffix=suffix, **kw)
        assert prog.last_batch_stats.docs_routed == 0
        seen |= {("status", s) for s in want[2]} | {("list", text)}
        # where the SELECTED raw fields of this call begin and end in the values tensor, and where they hold their pairs
        for i, m in enumerate(host.field_list_records_model(data, offs, sep_len, last_whole, P(text), FS, **kw)):
            if isinstance(m, int):
                continue
            at = offs[i] + lead
            for gap, (_, f) in zip(m[0], m[1]):
                at += len(gap)
                if f:
                    edges |= {("begin", at % 16), ("end", (at + len(f)) % 16)}
                for pair in (b'""', b'\\"', b"\\\\"):
                    k = f.find(pair)
                    while k >= 0:
                        pairs.add((pair, (at + k) % 16))
                        k = f.find(pair, k + 1)
                at += len(f)
        for m in host.field_list_records_model(data, offs, sep_len, last_whole, P("1-"), FS, **{k: v for k, v in kw.items()}):
            if isinstance(m, tuple):
                seen |= {("len", min(len(f), 3)) for _, f in m[1]}
    assert seen >= {("status", 0), ("status", 1), ("status", 2)} | {("len", k) for k in range(4)}, sorted(seen, key=str)
    for pair in ((b'""',) if "quote" in kw else ()) + ((b"\\\\",) if "escape" in kw else ()) + ((b'\\"',) if len(kw) == 2 else ()):
        assert {t for p, t in pairs if p == pair} == set(range(16)), (pair, sorted(pairs))   # … inside a selected field, across a granule edge too (t = 15)
    assert edges == {(w, t) for w in ("begin", "end") for t in range(16)}, sorted(edges)   # selected fields begin and end at every byte of a granule


def test_hand_cases():
    blob = blob_of(QPROG)
    prog = Program(blob)
    q = dict(quote=Q, sep_len=1)
    assert _check(prog, blob, b"", [0], P("2"), **q)[1] == [0]
    assert _check(prog, blob, b'x;"a";y\n', [0, 8], P("2"), **q)[0] == b'x;"""";y\n'                  # a → one quote, doubled and wrapped
    assert _check(prog, blob, b"x;a;y\n", [0, 6], P("2"), **q)[0] == b'x;"""";y\n'                    # … wrapped because of the quote
    assert _check(prog, blob, b"x;e;y\n", [0, 6], P("2"), **q)[0] == b"x;e;y\n"
    assert _check(prog, blob, b'x;"e";"";\n', [0, 10], P("2-"), **q)[0] == b'x;"e";"";\n'             # the empty output of a quoted field: ""
    assert _check(prog, blob, b'x;b;c;"d"\n', [0, 10], P("2-"), **q)[0] == b'x;";";"\n";"\\"\n'
    assert _check(prog, blob, b'x;b;c;d"a\n', [0, 10], P("2-"), quote=Q, escape=E, sep_len=1)[0] == b'x;";";"\n";\\\\\\"\n'
    assert _check(prog, blob, b"x;b;c;da\n", [0, 9], P("2-"), escape=E, sep_len=1)[0] == b'x;\\;;\\\n;\\\\"\n'
    assert _check(prog, blob, b"x;c;y|", [0, 6], P("2"), quote=Q, sep_len=1, special=b"|")[0] == b"x;\n;y|"   # the caller's special bytes decide
    # a rejected quoted field: nothing, and no ""; S counts in the value (the quote and the pair in front of the digit are 1 byte)
    want = _check(prog, blob, b'x;"""1";y\n' + b'x;"e";"f1"\n' + b'"e"\n', [0, 10, 21, 25], P("2-"), suffix=b"|", **q)
    assert want == (b"", [0, 0, 0, 0], [1, 1, 2], [_want(blob, b'"1')[0], _want(blob, b"f1")[0], 1], [0, 0, 0], [2, 3, 2])
    assert want[3][0] == 0 and want[3][1] == 1


def test_with_timing_the_new_kernels_count_in_the_field_groups():
    """kx_config::collect_timing: decoding adds into gather_ms (nothing is gathered on this path), spelling into splice_ms; a batch
    without a document (every record too short) and the list path behind it run with the same program."""
    blob = blob_of(QPROG)
    prog = Program(blob, collect_timing=True)
    data, offs = single._pack([b'x;"a";y;"b"', b"e", b'x;"1";y;z'] * 50, 1)
    for _ in range(2):
        before = prog.fields_kernel_stats()
        _check(prog, blob, data, offs, P("2,4"), lead=3, quote=Q, sep_len=1)
        after = prog.fields_kernel_stats()
        assert after["calls"] == before["calls"] + 1                                    # (the size query ends before the splice and is not counted)
        assert all(after[k] > before[k] for k in ("locate_ms", "gather_ms", "scan_ms", "splice_ms")), (before, after)
    _check(prog, blob, data, offs, P("9"), lead=3, quote=Q, sep_len=1)                  # no document at all
    flist._check(prog, blob, data, offs, P("2,4"), lead=3, quote=Q, sep_len=1)          # the list path, timed, with the same program
    d = b"".join(b'x;"a";y;"b"\n' for _ in range(300))
    with open("/dev/null", "wb") as sink:
        r, w = os.pipe()
        os.write(w, d)
        os.close(w)
        st = prog.run_records_fd(r, sink.fileno(), quote=Q, fields=[2, 4], fs=FS, unquote=True)
        os.close(r)
    assert (st["records"], st["rejected"], st["out_bytes"]) == (300, False, 300 * len(b'x;"""";y;";"\n'))


# ---------------------------------------------------------------------------------------------------------- 2. scan and wave edges
@pytest.mark.parametrize("nrec,text", [(1, "2,4"), (63, "2,4"), (64, "2,4"), (65, "2,4"), (341, "1-3"), (512, "2-3"), (205, "1-5")])
def test_scan_and_wave_edges(nrec, text):
    blob = blob_of(QPROG)
    prog = Program(blob)
    r = random.Random(nrec)
    bodies = [FS.join([b'"a e"', b"bc", b'"d""e"', b"", b'"g\nh"']) for _ in range(nrec)]
    for i in range(0, nrec, 7):
        bodies[i] = FS.join(bytes(r.choice(b"abcdefg") for _ in range(r.randrange(0, 6))) for _ in range(5))
    data, offs = single._pack(bodies, 1)
    ranges = P(text)
    _check(prog, blob, data, offs, ranges, lead=nrec % 16, quote=Q, sep_len=1, suffix=b"|")
    ndocs = sum(len(m[1]) for m in host.field_list_records_model(data, offs, 1, False, ranges, FS, Q))
    assert ndocs == {1: 2, 63: 126, 64: 128, 65: 130, 341: 1023, 512: 1024, 205: 1025}[nrec]


def test_more_documents_than_one_grid_stride():
    """The four new kernels launch at most 4 workgroups of 512 lanes per CU, one document a lane, and stride over the rest.  A batch
    beyond that: records picked from a small pool, the expectation put together from the picks."""
    import numpy as np
    import torch
    blob = blob_of(QPROG)
    prog = Program(blob)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = ncu * 4 * 512 * 6 // 10                                                         # two documents a record, but for a few without field 4
    r = random.Random(23)
    ranges = P("2,4")
    pool = [FS.join(_raw_fields(r, "quoted") for _ in range(5)) + b"\n" for _ in range(90)]
    pool += [b"e;f\n", b"\n", b'e;"1";f;g\n', b'e;"a";f;"b\nc"\n']
    want = [_expected(blob, p, [0, len(p)], ranges, quote=Q, sep_len=1, suffix=b"|") for p in pool]
    picks = np.array([r.randrange(len(pool)) for _ in range(n)], dtype=np.int64)
    picks[0], picks[-1] = len(pool) - 4, len(pool) - 2
    data = b"".join(pool[i] for i in picks.tolist())
    plen, olen = np.array([len(p) for p in pool], dtype=np.int64), np.array([len(w[0]) for w in want], dtype=np.int64)
    ndocs = int(np.array([0 if w[2][0] == 2 else 2 for w in want])[picks].sum())
    assert ndocs > ncu * 4 * 512
    offs = np.concatenate(([0], np.cumsum(plen[picks])))
    ooff = np.concatenate(([0], np.cumsum(olen[picks])))
    lead = 5
    v = torch.frombuffer(bytearray(single.LEAD[:lead] + data + single.TRAIL), dtype=torch.uint8).cuda()
    o = torch.from_numpy(offs + lead).cuda()
    out, goff, status, fpos, fstage, ffield = prog.run_batch_field_values_tensor(v, o, ranges, fs=FS, quote=Q, sep_len=1, suffix=b"|")
    torch.cuda.synchronize()
    col = lambda k: np.array([w[k][0] for w in want])[picks]   # noqa: E731
    assert np.array_equal(goff.cpu().numpy(), ooff)
    assert np.array_equal(status.cpu().numpy(), col(2)) and np.array_equal(fpos.cpu().numpy(), col(3)) and np.array_equal(ffield.cpu().numpy(), col(5))
    assert set(col(2).tolist()) == {0, 1, 2}
    got, exp = out.cpu().numpy().tobytes(), b"".join(want[i][0] for i in picks.tolist())
    assert got == exp, next(i for i in range(n) if got[ooff[i]:ooff[i + 1]] != exp[ooff[i]:ooff[i + 1]])


# ---------------------------------------------------------------------------------------------------------- 3. long fields, long outputs
def test_one_long_quoted_field_takes_the_route():
    blob = blob_of(COPY)
    prog = Program(blob)
    long_field = b'"' + b'""' * 70000 + b'"'                                             # a value of 70 000 quotes: above batch_doc_max (64 KiB)
    bodies = [b'x;"e,f";y', b'x;"e\nf";y', b"k"] * 20 + [b"pre;" + long_field + b";post"] + [b'x;"";y'] * 20
    data, offs = single._pack(bodies, 1)
    want = _check(prog, blob, data, offs, P("2"), lead=7, quote=Q, sep_len=1, suffix=b"|")
    assert prog.last_batch_stats.docs_routed == 1 and set(want[2]) == {0, 1, 2}          # (COPY rejects the value with a newline)
    assert want[0][want[1][60]:want[1][61]] == b"pre;" + long_field + b";post\n|"


def test_an_output_of_a_thousand_quotes():
    blob = blob_of(QPROG)
    prog = Program(blob)
    data = b"x;" + b"a" * 1000 + b";y\n"
    for kw, spelled in ((dict(quote=Q), b'"' + b'""' * 1000 + b'"'), (dict(quote=Q, escape=E), b'\\"' * 1000), (dict(escape=E), b'"' * 1000)):
        for lead in (0, 9):
            assert _check(prog, blob, data, [0, len(data)], P("2"), lead=lead, sep_len=1, **kw)[0] == b"x;" + spelled + b";y\n"
    assert len(b'"' + b'""' * 1000 + b'"') == 2002


# ---------------------------------------------------------------------------------------------------------- 4. capacity
def _raw(prog, v, o, spec, codec, cap, guard=0):
    """kx_run_batch_field_values through the C ABI: (rc, out_len, out bytes with the guard, out_off, docs words, fail_field, stats)."""
    import torch
    n = o.numel() - 1
    out = torch.full((max(cap + guard, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    ooff = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    docs = torch.full((max(n, 1), 2), -1, dtype=torch.int64, device="cuda")
    ff = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    ol, st = ctypes.c_size_t(), host.KxBatchStats()
    rc = prog._lib.kx_run_batch_field_values(prog._h, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(o.data_ptr()), n, spec, codec,
                                             ctypes.c_void_p(out.data_ptr() if cap else None), cap, ctypes.c_void_p(ooff.data_ptr()),
                                             ctypes.c_void_p(docs.data_ptr()), ctypes.c_void_p(ff.data_ptr()), ctypes.byref(ol), ctypes.byref(st), None)
    torch.cuda.synchronize()
    return rc, ol.value, out.cpu().numpy().tobytes(), ooff.tolist(), docs.tolist(), ff.tolist(), st


def test_size_query_and_capacity():
    blob = blob_of(QPROG)
    prog = Program(blob)
    bodies = [b'q;"a,b";r;s', b";;;", b'q;"e";f;"g1"', b"efg", b'z;"9";;', b"", b'x;"c";z;"";d'] * 9
    data, offs = single._pack(bodies, 2)
    v, o = single._device(data, offs, 5)
    f = flist._spec("2,4-", sep_len=2, keep_sep=1, suffix=b"\r\n!")
    f.quote = 34
    codec = host.KxFieldCodec(size=ctypes.sizeof(host.KxFieldCodec), n_special=1)
    codec.special[0] = 10
    want = _expected(blob, data, offs, P("2,4-"), quote=Q, sep_len=2, suffix=b"\r\n!")
    need = len(want[0])
    assert set(want[2]) == {0, 1, 2} and need > 100
    rc, ol, _, ooff, docs, ff, st = _raw(prog, v, o, ctypes.byref(f), ctypes.byref(codec), 0)
    assert (rc, ol) == (-3, need) and ooff == want[1] and st.out_bytes == need          # the size query fills offsets and records
    assert [d[1] & 0xFFFFFFFF for d in docs] == want[2] and [d[0] for d in docs] == want[3] and ff == want[5]
    rc, ol, out, ooff, docs, ff, _ = _raw(prog, v, o, ctypes.byref(f), ctypes.byref(codec), need - 1)
    assert (rc, ol) == (-3, need) and out == b"\xee" * (need - 1)                       # one byte short: nothing written, d_out_off filled
    assert ooff == want[1] and [d[1] & 0xFFFFFFFF for d in docs] == want[2] and ff == want[5]
    rc, ol, out, ooff, _, _, st = _raw(prog, v, o, ctypes.byref(f), ctypes.byref(codec), need, guard=48)
    assert (rc, ol, out, ooff) == (1, need, want[0] + b"\xee" * 48, want[1])            # nothing behind out_len
    assert st.docs_rejected == sum(1 for s in want[2] if s) and st.docs == len(bodies)
    import torch
    buf = torch.full((3 + need + 64,), 0xEE, dtype=torch.uint8, device="cuda")          # the size query, then the real call, through the binding
    res = prog.run_batch_field_values_tensor(v, o, P("2,4-"), fs=FS, quote=Q, sep_len=2, suffix=b"\r\n!", out=buf[3:3 + need])
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == b"\xee" * 3 + want[0] + b"\xee" * 64 and res[1].tolist() == want[1]
    res = prog.run_batch_field_values_tensor(v, o, P("2,4-"), fs=FS, quote=Q, sep_len=2, suffix=b"\r\n!")
    assert res[0].cpu().numpy().tobytes() == want[0]


# ---------------------------------------------------------------------------------------------------------- 5. the binary, run_records
def _stream(r, alphabet, bad):
    """About 40 KiB of QUOTE_ALL records of 1 to 5 fields over `alphabet` (the record separator among it), a field of 14 KiB, records
    with a field that holds `bad`, a tail without a separator."""
    recs = []
    for i in range(1400):
        fields = ["".join(r.choice(alphabet) for _ in range(r.randrange(0, 9))) for _ in range(r.choice((1, 3, 4, 4, 5, 5)))]
        if r.randrange(25) == 0:
            fields[r.randrange(len(fields))] += bad
        recs.append(fields)
    recs[3] = recs[4] = ["", "", "", ""]
    recs[700] = ["head", alphabet[0] * 7000 + "\n" + alphabet[0] * 7000, "mid", "tail"]
    buf = io.StringIO(newline="")
    csv.writer(buf, quoting=csv.QUOTE_ALL, delimiter=";", lineterminator="\n").writerows(recs)
    return buf.getvalue().encode() + b";".join([b'"%s"' % alphabet[:2].encode()] * 4)


def _want_stream(blob, data, ranges, chomp, ors, kw, sep=b"\n", fs=FS, special=None):
    """What record mode with --unquote must write and report; the spelling's special byte is the record separator (`special`: another)."""
    offs = host.split_escaped_records_model(data, sep, kw.get("quote"), kw["escape"])[0] if "escape" in kw else host.split_records_model(data, sep, Q)
    tail = bool(data) and not data.endswith(sep)
    out, _, status, fpos, fstage, ffield = _expected(blob, data, offs, ranges, fs=fs, special=sep if special is None else special, sep_len=1, last_whole=tail, keep_sep=not chomp,
                                                     suffix=ors, **kw)
    err, res = [], []
    for i, s in enumerate(status):
        if s == 2:
            err.append("Record %d has no field %d!\n" % (i + 1, ffield[i]))
        elif s:
            err.append("Match error at input symbol %d in field %d of record %d!\n" % (fpos[i], ffield[i], i + 1))
    return out, "".join(err).encode(), (status, fpos, fstage, ffield)


@pytest.mark.parametrize("name,src,alphabet,bad", [("flip", "flip_ab", "ab\n", "x"), ("qprog", QPROG, "abcdefg ", "1")])
def test_binary_whole_and_in_small_windows(tmp_path_factory, name, src, alphabet, bad):
    from kleenexlang_amd import program_path
    text = open(program_path(src)).read() if src == "flip_ab" else src
    blob, exe = blob_of(text), single._bin(tmp_path_factory, text)
    data = _stream(random.Random(len(name)), alphabet + ("\n" if "\n" not in alphabet else ""), bad)
    assert len(data) > 8 * 4096 and b'\n"' in data.replace(b'"\n"', b"")               # separators inside quoted fields
    # (every run is a process that loads the engine: the list as it is written, and one plain number with the framing)
    for field, ranges, framing, chomp, ors in (("2,4", P("2,4"), [], False, b""), ("2", P("2-2"), ["--chomp", "--ors=\\r\\n"], True, b"\r\n")):
        out, err, (status, _, _, _) = _want_stream(blob, data, ranges, chomp, ors, dict(quote=Q))
        assert set(status) == {0, 1, 2} and status[-1] == 0 and b" in field " in err
        for window in (1 << 30, 4096):
            r = single._run_bin(exe, ["--records", "--quote", "--field=" + field, "--fs=;", "--unquote"] + framing, data, window)
            assert r.returncode == 1, (r.returncode, r.stderr[-500:])
            assert r.stderr == err, (window, r.stderr[:300], err[:300])
            assert r.stdout == out, (window, len(r.stdout), len(out), next(i for i in range(min(len(out), len(r.stdout)) + 1) if r.stdout[i:i + 1] != out[i:i + 1]))
    # the README's example: flip_ab turns abba into baab inside the quotes it came in; QPROG's `";;"` holds a quote, which is doubled
    r = single._run_bin(exe, ["--records", "--quote", "--field=2", "--fs=,", "--unquote"], b'"id1","abba","x"\n' * 2, 4096)
    assert (r.returncode, r.stderr) == (0, b"")
    assert r.stdout == {"flip": b'"id1","baab","x"\n', "qprog": b'"id1",""";;""","x"\n'}[name] * 2


def _csv_file(dialect, seed):
    r = random.Random(seed)
    esc = dialect == "escape"
    alphabet = 'ab,"\n\r x' + ("\\" if esc else "z")
    kw = dict(lineterminator="\n")
    if dialect == "all":
        kw["quoting"] = csv.QUOTE_ALL
    if esc:
        kw.update(escapechar="\\", doublequote=False)
    rows = [["".join(r.choice(alphabet) for _ in range(r.randrange(0, 7))) for _ in range(r.randrange(2, 5))] for _ in range(1500)]
    buf = io.StringIO(newline="")
    csv.writer(buf, **kw).writerows(rows)
    return buf.getvalue().encode(), (dict(quote=Q, escape=E) if esc else dict(quote=Q)), (["--quote", "--escape"] if esc else ["--quote"])


@pytest.mark.parametrize("dialect", ["default", "all", "escape"])
def test_identity_reproduces_csv_writer_files(tmp_path_factory, dialect):
    """The identity program on every field of a csv.writer file: decoding and spelling again give the file back, byte for byte —
    through the binary in 4 KiB windows and through Program.run_records."""
    data, kw, args = _csv_file(dialect, 77)
    exe = single._bin(tmp_path_factory, IDENT)
    r = single._run_bin(exe, ["--records"] + args + ["--field=1-", "--fs=,", "--unquote"], data, 4096)
    assert (r.returncode, r.stderr) == (0, b"")
    assert r.stdout == data, next(i for i in range(len(data)) if r.stdout[i:i + 1] != data[i:i + 1])
    prog = Program(blob_of(IDENT))
    assert b"".join(prog.run_records(data, fields=[(1, None)], fs=b",", unquote=True, **kw)) == data


@pytest.mark.parametrize("sep", [b"\n", 10, b";"], ids=["lf", "int-lf", "semicolon"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_run_records_unquote(mode, sep):
    """`sep` as bytes and as an int (both are documented forms); with ";" the records end at the byte QPROG writes for a `b` and the
    fields at ",": the special byte of the spelling is then the record separator and not the model's default, so an output
    holding ";" is wrapped or escaped and one holding a newline goes out bare."""
    kw = MODES[mode]
    blob = blob_of(QPROG)
    prog = Program(blob)
    r = random.Random(60 + len(mode))
    bodies = [b.replace(b"\n", b"") for b in _bodies(r, mode, 600)] + [b"e;f;g;h"]
    sepb = bytes([sep]) if isinstance(sep, int) else sep
    fs = FS
    if sepb == b";":
        bodies, fs = [b.replace(b";", b",") for b in bodies], b","
    data = sepb.join(bodies)
    for fields, field, chomp, ors in ((P("2,4"), None, False, b""), (None, 2, True, b"\n"), ([(2, None)], None, True, b"12345678")):
        ranges = host._check_field_ranges(fields if fields is not None else [field])
        out, _, (status, fpos, fstage, ffield) = _want_stream(blob, data, ranges, chomp, ors, kw, sepb, fs)
        got = prog.run_records(data, sep=sep, chomp=chomp, ors=ors, fields=fields, field=field, fs=fs, unquote=True, **kw)
        assert len(got) == len(status) and set(status) == {0, 1, 2}
        for i, g in enumerate(got):
            if status[i] == 2:
                assert isinstance(g, NoFieldError) and g.fields == fpos[i], (i, g)
            elif status[i]:
                assert isinstance(g, MatchError) and (g.pos, g.stage, g.field) == (fpos[i], fstage[i], ffield[i]), (i, g)
        assert b"".join(g for g in got if isinstance(g, bytes)) == out
        if sepb == b";":                                                                # the int form of the same byte: the same results
            again = prog.run_records(data, sep=sepb[0], chomp=chomp, ors=ors, fields=fields, field=field, fs=fs[0], unquote=True, **kw)
            assert [g if isinstance(g, bytes) else (type(g), g.args) for g in again] == [g if isinstance(g, bytes) else (type(g), g.args) for g in got]
            # … and the special byte decides here: spelled with the model's default one, these outputs would read otherwise
            assert _want_stream(blob, data, ranges, chomp, ors, kw, sepb, fs, special=b"\n")[0] != out
    assert prog.run_records(b"", sep=sep, fields=[2, 4], fs=fs, unquote=True, **kw) == []
