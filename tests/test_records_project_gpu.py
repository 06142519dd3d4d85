"""GPU: field mode, projected — kx_run_batch_field_project (Program.run_batch_field_project_tensor), Program.run_records(only=, ofs=)
and `BIN --records … --field=LIST --only [--ofs=STR]`.  Every record's expected result is built in Python: host.project_records_model
cuts the record and orders the fields, the CPU oracle runs on each selected field alone (test_records_field_gpu's cache of oracle
results), and the outputs are joined here.  The programs, the packers and the bodies are the other field tests', by import."""
import csv
import ctypes
import io
import random

import pytest
from conftest import blob_of

import test_records_field_gpu as single
import test_records_field_list_gpu as lst
import test_records_project as cpu
from kleenexlang_amd import host
from kleenexlang_amd.host import MatchError, NoFieldError, Program

pytestmark = pytest.mark.gpu

COPY, FIELDS, WHOLE = single.COPY, single.FIELDS, single.WHOLE
FS, LEAD, TRAIL = single.FS, single.LEAD, single.TRAIL
_want = single._want
O = host.parse_field_order
SIXTEEN = "2,1,4,3,2-3,1,5,2,4-5,1,3,2,1-2,4,3,5-"                                      # 16 items; their union is 1-
ITEMS = ["4,2", "2,1,2", "3-,1-2", "1-", "6-,3-4,1", SIXTEEN]
OFS = [b"", b"|", b", ", b"<-ofs->!"]


def _union(items):
    return host._check_field_items(items)[1]


def _expected(blob, data, offs, items, ofs, fs=FS, quote=None, escape=None, sep_len=0, last_whole=False, keep_sep=True, suffix=b"", blanks=False,
              unquote=False, special=b"\n"):
    """(output bytes, output offsets, status, fail_pos, fail_stage, fail_field) from the model, the oracle and a join in Python.  With
    `unquote` the oracle runs on the value and its output is spelled with fs = OFS."""
    ranges = _union(items)
    out, ooff, status, fpos, fstage, ffield = [], [0], [], [], [], []
    for m in host.project_records_model(data, offs, sep_len, last_whole, items, None if blanks else fs, quote, escape, blanks=blanks):
        if isinstance(m, int):
            s = (m, 2, 0, host.field_list_missing(ranges, m))
        else:
            fields, sep = m
            res = [_want(blob, host.unquote_field_model(f, quote, escape) if unquote else f) for _, f in fields]
            bad = min(((K, j) for j, ((K, _), w) in enumerate(zip(fields, res)) if isinstance(w, tuple)), default=None)   # the lowest rejected NUMBER
            s = (res[bad[1]][0], 1, res[bad[1]][1], bad[0]) if bad is not None else None
        if s is not None:
            fpos.append(s[0]); status.append(s[1]); fstage.append(s[2]); ffield.append(s[3])
            ooff.append(ooff[-1])
        else:
            if unquote:
                sp = special + (b"\t" if blanks else b"")
                res = [host.requote_field_model(w, quote is not None and f[:1] == quote, ofs, quote, escape, sp) for (_, f), w in zip(fields, res)]
            status.append(0); fpos.append(0); fstage.append(0); ffield.append(0)
            out.append(ofs.join(res) + (sep if keep_sep else b"") + suffix)
            ooff.append(ooff[-1] + len(out[-1]))
    return b"".join(out), ooff, status, fpos, fstage, ffield


def _check(prog, blob, data, offs, items, ofs, lead=0, **kw):
    import torch
    want = _expected(blob, data, offs, items, ofs, **kw)
    v, o = single._device(data, offs, lead)
    if not kw.get("blanks"):
        kw.setdefault("fs", FS)
    res = prog.run_batch_field_project_tensor(v, o, items, ofs, **kw)
    torch.cuda.synchronize()
    got = (res[0].cpu().numpy().tobytes(),) + tuple(t.tolist() for t in res[1:])
    ctx = (items, ofs, lead, kw)
    rec = lambda i: data[offs[min(i, len(offs) - 2)]:offs[min(i, len(offs) - 2) + 1]][:80]   # noqa: E731
    for name, k in (("status", 2), ("fail_pos", 3), ("fail_stage", 4), ("fail_field", 5), ("out_off", 1)):
        if got[k] != want[k]:
            i = next(j for j in range(len(want[k])) if got[k][j] != want[k][j])
            raise AssertionError("%s[%d]: got %r, want %r (record %r, %r)" % (name, i, got[k][i], want[k][i], rec(i), ctx))
    assert got[0] == want[0], (ctx, next((i, rec(i), got[0][want[1][i]:want[1][i + 1]][:80], want[0][want[1][i]:want[1][i + 1]][:80])
                                         for i in range(len(offs) - 1) if got[0][want[1][i]:want[1][i + 1]] != want[0][want[1][i]:want[1][i + 1]]))
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.out_bytes) == (len(offs) - 1, sum(1 for s in want[2] if s), len(want[0]))   # the projected bytes
    return want


# ---------------------------------------------------------------------------------------------------------- 1. model + oracle
@pytest.mark.parametrize("name", sorted(single.PROGRAMS))
def test_batch_field_project_against_model_and_oracle(name):
    src, cfg = single.PROGRAMS[name]
    blob = blob_of(src)
    prog = Program(blob, config=host.config_from_env({}, **cfg))
    r = random.Random(300 + len(name))
    big, small = lst._bodies(r, name, 1000), lst._bodies(r, name, 100)
    seen = set()
    for lead in range(16):                                                              # every start alignment, every option's every value
        text, ofs = ITEMS[lead % 6], OFS[(lead + lead // 6) % 4]
        sep_len, suffix = (0, 1, 2, 8)[(lead + lead // 4) % 4], (b"", b"|", b"12345678")[lead % 3]
        last_whole, keep_sep = bool(lead & 1) ^ bool(lead & 4), bool(lead & 2) ^ bool(lead & 8)
        data, offs = single._pack(big, sep_len)
        want = _check(prog, blob, data, offs, O(text), ofs, lead=lead, sep_len=sep_len, last_whole=last_whole, keep_sep=keep_sep, suffix=suffix)
        seen |= {("items", text), ("ofs", ofs), ("sep", sep_len), ("sfx", len(suffix)), ("lw", last_whole), ("keep", keep_sep)}
        seen |= {("status", s) for s in set(want[2])} | {("oalign", o % 16) for o in want[1][:-1]}
        assert want[2][0] != 0 and want[2][-1] != 0                                     # a rejected record first and last
    assert len(seen) == 6 + 4 + 4 + 3 + 2 + 2 + 3 + 16, sorted(seen)
    n = 0
    for text in ITEMS:                                                                  # the small batch: every list with every separator
        for ofs in OFS:
            for sep_len in (0, 1, 2, 8):
                data, offs = single._pack(small, sep_len)
                _check(prog, blob, data, offs, O(text), ofs, lead=(5 * n + 3) % 16, sep_len=sep_len, last_whole=bool(n & 1), keep_sep=bool(n & 2),
                       suffix=(b"", b"\n", b"<<eor>>\n")[n % 3])
                n += 1


def test_statuses_are_the_list_paths():
    import torch
    blob = blob_of(FIELDS)
    prog = Program(blob)
    r = random.Random(41)
    data, offs = single._pack(lst._bodies(r, "fields", 1500), 1)
    v, o = single._device(data, offs, 6)
    seen = set()
    for text in ITEMS + ["9,4,2", "5-,3"]:
        items = O(text)
        a = prog.run_batch_field_project_tensor(v, o, items, b"|", fs=FS, sep_len=1)
        b = prog.run_batch_field_list_tensor(v, o, _union(items), fs=FS, sep_len=1)
        torch.cuda.synchronize()
        for k in (2, 3, 4, 5):                                                          # status, fail_pos, fail_stage, fail_field
            assert torch.equal(a[k], b[k]), (text, k)
        seen |= set(a[2].tolist())
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("quote,escape", [(None, None), (b'"', None), (b'"', b"\\")])
def test_the_identity_projection_is_the_list_path(quote, escape):
    import torch
    blob = blob_of(FIELDS)
    prog = Program(blob)
    r = random.Random(5)
    bodies = single._bodies(r, "fields", 1200) + (lst._liveness_bodies() if quote or escape else [])
    seen = set()
    for sep_len, last_whole, keep_sep, suffix, lead in ((1, False, True, b"", 0), (2, True, False, b"|", 7), (0, False, True, b"12345678", 13)):
        data, offs = single._pack(bodies, sep_len)
        v, o = single._device(data, offs, lead)
        kw = dict(fs=FS, quote=quote, escape=escape, sep_len=sep_len, last_whole=last_whole, keep_sep=keep_sep, suffix=suffix)
        a = prog.run_batch_field_project_tensor(v, o, O("1-"), FS, **kw)
        b = prog.run_batch_field_list_tensor(v, o, host.parse_field_list("1-"), **kw)
        torch.cuda.synchronize()
        for k in range(6):
            assert torch.equal(a[k], b[k]), (k, kw)
        seen |= set(a[2].tolist())
    assert seen == {0, 1}                                                               # (1- has no record too short)


# ---------------------------------------------------------------------------------------------------------- 2. hand cases
def test_hand_cases():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    assert _check(prog, blob, b"ab;c,d;e;f\r\n", [0, 12], O("4,2"), b"\t", sep_len=2, keep_sep=False, suffix=b"$")[0] == b"<f>\t<c> | <d>$"
    assert _check(prog, blob, b"ab;c,d;e;f\r\n", [0, 12], O("2,1,2"), b"", sep_len=2)[0] == b"<c> | <d><ab><c> | <d>\r\n"
    assert _check(prog, blob, b";;;", [0, 3], O("1-"), b"")[0] == b"<><><><>"
    assert _check(prog, blob, b";;;", [0, 3], O("3-,1-2"), b", ")[0] == b"<>, <>, <>, <>"
    want = _check(prog, blob, b"ab;c;e1;f1\n", [0, 11], O("4,3,2"), b"|", sep_len=1)      # written in descending order: the lowest NUMBER reports
    assert want[2:] == ([1], [_want(blob, b"e1")[0]], [0], [3])
    assert _check(prog, blob, b"ab;c\n", [0, 5], O("6-,3-4,1"), b"|", sep_len=1)[2:] == ([2], [2], [0], [3])       # K: the first field it lacks
    assert _check(prog, blob, b"", [0], O("4,2"), b"|")[1] == [0]                                                     # n_docs = 0
    assert _check(prog, blob, b"\n", [0, 1], O("1"), b"|", sep_len=1) == (b"<>\n", [0, 3], [0], [0], [0], [0])      # the lone separator
    assert _check(prog, blob, b"", [0, 0], O("2,1"), b"|", suffix=b"\n") == (b"", [0, 0], [2], [1], [0], [2])
    # an item inside the open range whose fields the record does not have writes nothing, no OFS either
    assert _check(prog, blob, b"a;b;c;d;e", [0, 9], O("9-10,3-,4"), b"|")[0] == b"<c>|<d>|<e>|<d>"
    assert _check(prog, blob, b"a;b;c", [0, 5], O("3-,9-10,7-"), b"|")[0] == b"<c>"


def test_an_accepted_record_without_a_byte_is_stepped_over():
    blob = blob_of(COPY)
    prog = Program(blob)
    data, offs = single._pack([b"a;b", b";", b";", b"c;d", b";", b"e;f"], 1)
    want = _check(prog, blob, data, offs, O("1,2"), b"", lead=3, sep_len=1, keep_sep=False)
    assert want == (b"abcdef", [0, 2, 2, 2, 4, 4, 6], [0] * 6, [0] * 6, [0] * 6, [0] * 6)
    want = _check(prog, blob, data, offs[:-1] + [offs[-1] - 1], O("2,1"), b"", lead=14, sep_len=1, keep_sep=False, last_whole=True)
    assert want[0] == b"badcfe"


# ---------------------------------------------------------------------------------------------------------- 3. the search, the route
@pytest.mark.parametrize("text", ["3,1-", "1-,1-"])
def test_five_thousand_fields_in_one_item(text):
    blob = blob_of(FIELDS)
    prog = Program(blob)
    bodies = [b"a;b;c", FS * 4999, b"a;b", b"x;y;z;1", b"", b"", b"a", b";", b"", FS * 4999, b"q"]   # (several records in one output granule)
    data, offs = single._pack(bodies, 1)
    for ofs in (b";", b""):
        want = _check(prog, blob, data, offs, O(text), ofs, lead=9, sep_len=1, keep_sep=False)
        assert want[2] == [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0] and want[5][3] == 4
        n = 5001 if text == "3,1-" else 10000
        assert want[0][want[1][1]:want[1][2]] == ofs.join([b"<>"] * n)
        assert want[1][6] - want[1][4] <= 10                                               # records 4, 5 and the start of 6 in one granule or two


def test_one_long_selected_field_takes_the_route():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    r = random.Random(3)
    long_field = bytes(r.choice(b"abc,") for _ in range(70 << 10))                   # above batch_doc_max (64 KiB)
    bodies = [b"ab;c,d;e;f", b"x;y;z;w1", b"k;l"] * 20 + [b"pre;" + long_field + b";mid;post"] + [b"ab;c,d;e;", b"", b"x;;z;;;"] * 20
    data, offs = single._pack(bodies, 1)
    want = _check(prog, blob, data, offs, O("4,2,3"), b"|", lead=7, sep_len=1, suffix=b"|")
    assert prog.last_batch_stats.docs_routed == 1 and set(want[2]) == {0, 1, 2}
    rec = want[0][want[1][60]:want[1][61]]
    assert rec.startswith(b"<post>|<") and rec.endswith(b">|<mid>\n|") and len(rec) > 70 << 10      # in the middle of the projected record


def test_more_than_one_grid_stride_in_both_kernels():
    """k_fpsplen launches at most 4 workgroups of 512 lanes per CU and strides over the rest, k_fpsplice at most 16 workgroups of 256
    lanes per CU, 16 bytes a lane.  A batch beyond both, built as test_records_field_list_gpu builds its own."""
    import numpy as np
    import torch
    blob = blob_of(FIELDS)
    prog = Program(blob)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = ncu * 4 * 512 + 75000
    r = random.Random(23)
    items, ofs = O("4,2,4"), b", "
    word = lambda k: bytes(r.choice(b"abc,") for _ in range(k))   # noqa: E731
    pool = [word(r.randrange(0, 5)) + FS + word(r.randrange(18, 34)) + FS + word(r.randrange(0, 5)) + FS + word(r.randrange(18, 34)) + FS + word(2) + b"\n"
            for _ in range(80)]
    pool += [word(3) + FS + word(20) + FS + FS + word(9) + b"7" + word(9) + FS + b"x\n" for _ in range(6)]   # rejected inside the second selected field
    pool += [word(12) + b"\n", b"\n", word(3) + FS + b"a" + FS + b"\n", FS * 3 + b"\n"]          # one field; one empty; three; four empty ones
    want = [_expected(blob, p, [0, len(p)], items, ofs, sep_len=1, suffix=b"|") for p in pool]
    picks = np.array([r.randrange(len(pool)) for _ in range(n)], dtype=np.int64)
    picks[0], picks[-1], picks[n // 2] = len(pool) - 4, 83, len(pool) - 3                          # a short record first, a rejected one last
    data = b"".join(pool[i] for i in picks.tolist())
    plen, olen = np.array([len(p) for p in pool], dtype=np.int64), np.array([len(w[0]) for w in want], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(plen[picks])))
    ooff = np.concatenate(([0], np.cumsum(olen[picks])))
    assert n > ncu * 4 * 512 and int(ooff[-1]) > ncu * 16 * 256 * 16                               # a second pass in both
    lead = 5
    v = torch.frombuffer(bytearray(LEAD[:lead] + data + TRAIL), dtype=torch.uint8).cuda()
    o = torch.from_numpy(offs + lead).cuda()
    out, goff, status, fpos, fstage, ffield = prog.run_batch_field_project_tensor(v, o, items, ofs, fs=FS, sep_len=1, suffix=b"|")
    torch.cuda.synchronize()
    col = lambda k: np.array([w[k][0] for w in want])[picks]   # noqa: E731
    assert np.array_equal(goff.cpu().numpy(), ooff)
    assert np.array_equal(status.cpu().numpy(), col(2)) and np.array_equal(fpos.cpu().numpy(), col(3)) and np.array_equal(ffield.cpu().numpy(), col(5))
    assert int(fstage.sum()) == 0 and set(col(5).tolist()) == {0, 2, 4}
    got, exp = out.cpu().numpy().tobytes(), b"".join(want[i][0] for i in picks.tolist())
    assert got == exp, next(i for i in range(n) if got[ooff[i]:ooff[i + 1]] != exp[ooff[i]:ooff[i + 1]])
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.docs_routed) == (n, int(np.count_nonzero(col(2))), 0)


# ---------------------------------------------------------------------------------------------------------- 4. capacity, the rules
def _raw(prog, v, o, spec, codec, proj, cap, guard=0, null_ff=False):
    """kx_run_batch_field_project through the C ABI: (rc, out_len, out bytes with the guard, out_off, docs words, fail_field, stats)."""
    import torch
    n = o.numel() - 1
    out = torch.full((max(cap + guard, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    ooff = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    docs = torch.full((max(n, 1), 2), -1, dtype=torch.int64, device="cuda")
    ff = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    ol, st = ctypes.c_size_t(), host.KxBatchStats()
    rc = prog._lib.kx_run_batch_field_project(prog._h, ctypes.c_void_p(v.data_ptr() if v.numel() else None), ctypes.c_void_p(o.data_ptr()), n,
                                              ctypes.byref(spec), ctypes.byref(codec) if codec is not None else None, ctypes.byref(proj),
                                              ctypes.c_void_p(out.data_ptr() if cap else None), cap, ctypes.c_void_p(ooff.data_ptr()),
                                              ctypes.c_void_p(docs.data_ptr()), ctypes.c_void_p(None if null_ff else ff.data_ptr()), ctypes.byref(ol),
                                              ctypes.byref(st), None)
    torch.cuda.synchronize()
    return rc, ol.value, out.cpu().numpy().tobytes(), ooff.tolist(), docs.tolist(), ff.tolist(), st


def test_size_query_and_capacity():
    import torch
    blob = blob_of(FIELDS)
    prog = Program(blob)
    bodies = [b"q;ab,c;r;s", b";;;", b"q;a;b;c1", b"abc", b"z;9;;", b"", b"x;y;z;w;v"] * 9
    data, offs = single._pack(bodies, 2)
    v, o = single._device(data, offs, 5)
    items = O("4-,2")
    f = cpu.spec_list([(lo, hi or 0) for lo, hi in _union(items)], sep_len=2, suffix_len=3)
    f.suffix[:3] = b"\r\n!"
    p = cpu.spec_proj([(lo, hi or 0) for lo, hi in items], ofs=b", ")
    want = _expected(blob, data, offs, items, b", ", sep_len=2, suffix=b"\r\n!")
    need = len(want[0])
    assert set(want[2]) == {0, 1, 2} and need > 100
    rc, ol, _, ooff, docs, ff, st = _raw(prog, v, o, f, None, p, 0)
    assert (rc, ol) == (-3, need) and ooff == want[1] and st.out_bytes == need      # the size query fills offsets and records
    assert [d[1] & 0xFFFFFFFF for d in docs] == want[2] and [d[0] for d in docs] == want[3] and ff == want[5]
    rc, ol, out, ooff, docs, ff, _ = _raw(prog, v, o, f, None, p, need - 1)
    assert (rc, ol) == (-3, need) and out == b"\xee" * (need - 1)                   # one byte short: nothing written
    assert ooff == want[1] and [d[1] & 0xFFFFFFFF for d in docs] == want[2] and ff == want[5]
    for at in (0, 3):                                                               # the exact capacity, at two alignments of the output
        buf = torch.full((at + need + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        res = prog.run_batch_field_project_tensor(v, o, items, b", ", fs=FS, sep_len=2, suffix=b"\r\n!", out=buf[at:at + need])
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == b"\xee" * at + want[0] + b"\xee" * 64 and res[1].tolist() == want[1]
    rc, ol, out, ooff, _, _, st = _raw(prog, v, o, f, None, p, need, guard=48)
    assert (rc, ol, out, ooff) == (1, need, want[0] + b"\xee" * 48, want[1])        # nothing behind out_len
    assert st.docs_rejected == sum(1 for s in want[2] if s) and st.docs == len(bodies)
    rc, ol, out, _, _, ff, _ = _raw(prog, v, o, f, None, p, need, null_ff=True)     # a null fail_field array is allowed
    assert (rc, ol, out) == (1, need, want[0]) and set(ff) == {-1}


def test_the_rules_are_found_before_any_device_work():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    data, offs = single._pack([b"a;b;c;d", b"e;f;g;h"], 1)
    v, o = single._device(data, offs, 2)
    cap = 64
    for spec, codec, proj, what in cpu.abi_refusals():
        rc, _, out, ooff, docs, ff, _ = _raw(prog, v, o, spec, codec, proj, cap)
        assert rc == -4 and what.decode() in prog._err() and "kx_run_batch_field_project" in prog._err(), (what, prog._err())
        assert out == b"\xee" * cap and set(ooff) == {-1} and set(ff) == {-1} and docs == [[-1, -1]] * 2, what     # nothing was touched
    ok = _raw(prog, v, o, cpu.spec_list([(2, 2), (4, 4)]), None, cpu.spec_proj([(4, 4), (2, 2)]), cap)
    assert ok[0] == 0 and ok[2][:ok[1]] == b"<d>;<b>\n<h>;<f>\n"


# ---------------------------------------------------------------------------------------------------------- 5. values, words
def test_unquote_protects_the_output_delimiter():
    """QUOTED rows from csv.writer whose values hold the tab, the comma and the quote; OFS is the tab: what comes out is read back
    by csv.reader(delimiter="\\t") as the projected values"""
    blob = blob_of(COPY)
    prog = Program(blob)
    rnd = random.Random(8)
    alphabet = ["a", "b", ",", '"', "\t", " "]
    rows = [["".join(rnd.choice(alphabet) for _ in range(rnd.randrange(0, 7))) for _ in range(rnd.randrange(4, 8))] for _ in range(400)]
    buf = io.StringIO()
    csv.writer(buf, lineterminator="\n").writerows(rows)
    data = buf.getvalue().encode()
    offs = list(host.split_records_model(data, b"\n", b'"'))
    assert len(offs) - 1 == len(rows)
    items = O("4,2-3,2")
    want = _check(prog, blob, data, offs, items, b"\t", lead=11, fs=b",", quote=b'"', unquote=True, sep_len=1)
    assert set(want[2]) == {0}
    back = list(csv.reader(io.StringIO(want[0].decode(), newline=""), delimiter="\t"))
    assert back == [[row[k - 1] for k in (4, 2, 3, 2)] for row in rows]
    assert any("\t" in row[k - 1] for row in rows for k in (2, 3, 4)) and any("," in row[3] for row in rows)
    plain = _check(prog, blob, data, offs, items, b"\t", lead=11, fs=b",", quote=b'"', sep_len=1)        # without unquote: the raw spellings
    assert plain[0] != want[0]
    _check(prog, blob, data, offs, O("3-,1"), b"|", lead=4, fs=b",", quote=b'"', escape=b"\\", unquote=True, sep_len=1, keep_sep=False, suffix=b"\n")


@pytest.mark.parametrize("unquote", [False, True])
def test_blanks_at_every_granule_offset_of_the_first_word(unquote):
    blob = blob_of(COPY)
    prog = Program(blob)
    tails = [b"w  xy\t z ", b'"a b"\t"c"  d', b"one", b"p \t q  r   s \t", b'x"y z"  "" k']
    bodies, pos = [], 0
    for t in range(16):
        for tail in tails:
            bodies.append(b" " * ((t - pos) % 16) + tail)
            pos += len(bodies[-1]) + 1
    bodies += [b"", b"  \t ", b"solo"]
    data, offs = single._pack(bodies, 1)
    assert {(offs[i] + len(bodies[i]) - len(bodies[i].lstrip(b" "))) % 16 for i in range(0, 80, 5)} == set(range(16))   # the first word's offset
    kw = dict(blanks=True, quote=b'"', sep_len=1)
    if unquote:
        kw["unquote"] = True
    seen = set()
    for text, ofs in (("2,1", b" "), ("3-,1", b"|"), ("1-", b","), ("2,1,2", b" ")):
        want = _check(prog, blob, data, offs, O(text), ofs, lead=0, **kw)
        seen |= set(want[2])
    assert seen == {0, 2}
    if unquote:                                                                         # a value with a blank is wrapped: OFS is the space
        one = _check(prog, blob, b'k "a b"\n', [0, 8], O("2,1"), b" ", **kw)
        assert one[0] == b'"a b" k\n'


# ---------------------------------------------------------------------------------------------------------- 6. the binary
LIST = "4-,2"


def _want_stream(blob, data, mode, items, ofs, chomp, ors):
    _, kw, model_offsets, sep, _ = single.MODES[mode]
    ranges = _union(items)
    out, err, res = [], [], []
    model = host.project_records_model(data, model_offsets(data), len(sep), single._tail(model_offsets, data), items, FS, kw.get("quote"),
                                       kw.get("escape"))
    for i, m in enumerate(model):
        if isinstance(m, int):
            err.append("Record %d has no field %d!\n" % (i + 1, host.field_list_missing(ranges, m)))
            res.append(("nofield", m))
            continue
        w = [_want(blob, f) for _, f in m[0]]
        bad = min(((K, j) for j, ((K, _), x) in enumerate(zip(m[0], w)) if isinstance(x, tuple)), default=None)
        if bad is not None:
            err.append("Match error at input symbol %d in field %d of record %d!\n" % (w[bad[1]][0], bad[0], i + 1))
            res.append((w[bad[1]][0], w[bad[1]][1], bad[0]))
        else:
            out.append(ofs.join(w) + (b"" if chomp else m[1]) + ors)
            res.append(out[-1])
    return b"".join(out), "".join(err).encode(), res


@pytest.mark.parametrize("mode", sorted(single.MODES))
def test_binary_only_whole_and_in_small_windows(tmp_path_factory, mode):
    blob, exe = blob_of(WHOLE), single._bin(tmp_path_factory, WHOLE)
    data = lst._stream(mode)
    _, kw, _, _, _ = single.MODES[mode]
    prog = Program(blob)
    for framing, ofs, chomp, ors in (([], FS, False, b""), (["--ofs=, ", "--chomp", "--ors=\\n"], b", ", True, b"\n")):
        out, err, res = _want_stream(blob, data, mode, O(LIST), ofs, chomp, ors)
        kinds = {("nofield" if r[0] == "nofield" else "rejected") if isinstance(r, tuple) else "ok" for r in res}
        assert kinds == {"ok", "rejected", "nofield"} and not isinstance(res[-1], tuple)
        for window in (1 << 30, 4096):
            r = single._run_bin(exe, single.MODES[mode][0] + ["--field=" + LIST, "--fs=;", "--only"] + framing, data, window)
            assert r.returncode == 1, (r.returncode, r.stderr[-500:])
            assert r.stderr == err, (window, r.stderr[:300], err[:300])
            assert r.stdout == out, (window, len(r.stdout), len(out), next(i for i in range(min(len(out), len(r.stdout)) + 1) if r.stdout[i:i + 1] != out[i:i + 1]))
        got = prog.run_records(data, chomp=chomp, ors=ors, fields=list(O(LIST)), fs=FS, only=True, ofs=ofs if framing else None, **kw)
        got = [("nofield", g.fields) if isinstance(g, NoFieldError) else (g.pos, g.stage, g.field) if isinstance(g, MatchError) else g for g in got]
        assert got == res, (mode, next((i, g, w) for i, (g, w) in enumerate(zip(got, res)) if g != w))
    # every record accepted: status 0, nothing on stderr
    r = single._run_bin(exe, single.MODES[mode][0] + ["--field=4,2", "--fs=;", "--only", "--ofs=\\t"], b"ab;c;d;e", 4096)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", b"[e]\t[c]")


def test_the_readme_example_and_run_records_fd(tmp_path_factory):
    import os
    import subprocess
    from kleenexlang_amd import build, program_path
    exe = str(tmp_path_factory.mktemp("recproject") / "flip")
    assert subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("flip_ab"), "--out", exe], timeout=300).returncode == 0
    r = single._run_bin(exe, ["--records", "--field=4,2", "--fs=,", "--only", "--ofs=\\t"], b"a,abba,b,bab\n", 1 << 30)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", b"aba\tbaab\n")
    prog = Program.from_file(program_path("flip_ab"))
    rd, wr = os.pipe()
    os.write(wr, b"a,abba,b,bab\nb,a\n")
    os.close(wr)
    ord_, owr = os.pipe()
    st = prog.run_records_fd(rd, owr, fields=[4, 2], fs=b",", only=True, ofs=b"\t")
    os.close(owr); os.close(rd)
    assert os.read(ord_, 100) == b"aba\tbaab\n" and st["rejected"] and st["records_rejected"] == 1
    os.close(ord_)
