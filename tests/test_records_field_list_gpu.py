"""GPU: field mode with a list of fields — kx_run_batch_field_list (Program.run_batch_field_list_tensor),
Program.run_records(fields=) and `BIN --records … --field=LIST --fs=F`.  Every record's expected result is built in Python, as
test_records_field_gpu builds it: host.field_list_records_model cuts the record, the CPU oracle runs on each selected field alone
(one cache of oracle results for both files), and gaps + oracle outputs + separator + suffix are spliced here."""
import ctypes
import os
import random

import pytest
from conftest import blob_of

import test_records_field_gpu as single
from kleenexlang_amd import host
from kleenexlang_amd.host import MatchError, NoFieldError, Program

pytestmark = pytest.mark.gpu

COPY, FIELDS, TWO, SWAP, WHOLE = single.COPY, single.FIELDS, single.TWO, single.SWAP, single.WHOLE
FS, LEAD, TRAIL, JUNK = single.FS, single.LEAD, single.TRAIL, single.JUNK
_want = single._want
LISTS = ["2,4", "1-3", "2-", "1,3-4,6-", "1,3,5,7,9,11,13,15-", "1-"]                   # (the fifth: 8 ranges, the cap)
P = host.parse_field_list


def _expected(blob, data, offs, ranges, fs=FS, quote=None, escape=None, sep_len=0, last_whole=False, keep_sep=True, suffix=b""):
    """(output bytes, output offsets, status, fail_pos, fail_stage, fail_field) from the model, the oracle and a splice in Python."""
    out, ooff, status, fpos, fstage, ffield = [], [0], [], [], [], []
    for m in host.field_list_records_model(data, offs, sep_len, last_whole, ranges, fs, quote, escape):
        if isinstance(m, int):
            s = (m, 2, 0, host.field_list_missing(ranges, m))
        else:
            gaps, fields, sep = m
            res = [_want(blob, f) for _, f in fields]
            bad = next((j for j, w in enumerate(res) if isinstance(w, tuple)), None)         # the lowest rejected field
            s = (res[bad][0], 1, res[bad][1], fields[bad][0]) if bad is not None else None
        if s is not None:
            fpos.append(s[0]); status.append(s[1]); fstage.append(s[2]); ffield.append(s[3])
            ooff.append(ooff[-1])
        else:
            status.append(0); fpos.append(0); fstage.append(0); ffield.append(0)
            out.append(b"".join(g + w for g, w in zip(gaps, res + [b""])) + (sep if keep_sep else b"") + suffix)
            ooff.append(ooff[-1] + len(out[-1]))
    return b"".join(out), ooff, status, fpos, fstage, ffield


def _check(prog, blob, data, offs, ranges, lead=0, **kw):
    import torch
    want = _expected(blob, data, offs, ranges, **kw)
    v, o = single._device(data, offs, lead)
    kw.setdefault("fs", FS)
    res = prog.run_batch_field_list_tensor(v, o, ranges, **kw)
    torch.cuda.synchronize()
    got = (res[0].cpu().numpy().tobytes(),) + tuple(t.tolist() for t in res[1:])
    ctx = (ranges, lead, kw)
    rec = lambda i: data[offs[min(i, len(offs) - 2)]:offs[min(i, len(offs) - 2) + 1]][:80]   # noqa: E731
    for name, k in (("status", 2), ("fail_pos", 3), ("fail_stage", 4), ("fail_field", 5), ("out_off", 1)):
        if got[k] != want[k]:
            i = next(j for j in range(len(want[k])) if got[k][j] != want[k][j])
            raise AssertionError("%s[%d]: got %r, want %r (record %r, %r)" % (name, i, got[k][i], want[k][i], rec(i), ctx))
    assert got[0] == want[0], (ctx, next((i, rec(i), got[0][want[1][i]:want[1][i + 1]][:80]) for i in range(len(offs) - 1)
                                         if got[0][want[1][i]:want[1][i + 1]] != want[0][want[1][i]:want[1][i + 1]]))
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.out_bytes) == (len(offs) - 1, sum(1 for s in want[2] if s), len(want[0]))
    return want


# ---------------------------------------------------------------------------------------------------------- 1. model + oracle
def _bodies(r, name, n):
    """n bodies of 1 to 9 fields out of a pool (so that the oracle runs once per pool entry): most fields a few bytes, one in four
    at LENGTHS or one below, so that gaps, fields and outputs lie at the granule, checkpoint and piece borders; one field in 16 is
    one the program rejects.  Some bodies have 15 to 17 fields (the list of 8 ranges needs 15).  Rejected records stand first, last
    and in a run in the middle; empty bodies and bodies of only separators side by side."""
    sizes = sorted(set(single.LENGTHS) | {L - 1 for L in single.LENGTHS if L})
    pool = {L: [single._part(r, name, L, False), single._part(r, name, L, False), single._part(r, name, L, True)] for L in sizes + [2, 3, 5]}

    def part():
        L = r.choice(sizes) if r.randrange(4) == 0 else r.choice((0, 1, 2, 3, 5))
        return pool[L][2 if r.randrange(16) == 0 else r.randrange(2)]

    bodies = [FS.join(part() for _ in range(r.choice((15, 16, 17)) if r.randrange(8) == 0 else r.randrange(1, 10))) for _ in range(n)]
    allbad = FS.join([pool[17][2]] * 16)                                                 # every field rejected: no list accepts it
    bodies[0] = bodies[-1] = allbad
    bodies[n // 2:n // 2 + 5] = [allbad, pool[0][0], allbad, FS.join([pool[3][0]] * 5 + [pool[64][2]] * 11), allbad]
    bodies[n // 3:n // 3 + 5] = [b"", b"", FS * 3, FS * 16, b""]                           # empty bodies side by side, bodies of only separators
    good = pool[5][0]
    bodies[n // 4:n // 4 + 2] = [FS.join([good, good, good, pool[5][2], good, good]),       # the first selected field accepted, a later one
                                 FS.join([good, good, pool[5][2]] + [good] * 3)]           #   rejected: field 4 of 2,4, field 3 of 2-, …
    return bodies


PROGRAMS = single.PROGRAMS


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_batch_field_list_against_model_and_oracle(name):
    src, cfg = PROGRAMS[name]
    blob = blob_of(src)
    prog = Program(blob, config=host.config_from_env({}, **cfg))
    r = random.Random(100 + len(name))
    big, small = _bodies(r, name, 3000), _bodies(r, name, 120)
    seen, second = set(), 0
    for lead in range(16):                                                              # every start alignment, every option's every value
        text = LISTS[lead % 6]
        sep_len, suffix = (0, 1, 2, 8)[(lead + lead // 4) % 4], (b"", b"|", b"12345678")[lead % 3]
        last_whole, keep_sep = bool(lead & 1) ^ bool(lead & 4), bool(lead & 2) ^ bool(lead & 8)
        data, offs = single._pack(big, sep_len)
        ranges = P(text)
        want = _check(prog, blob, data, offs, ranges, lead=lead, sep_len=sep_len, last_whole=last_whole, keep_sep=keep_sep, suffix=suffix)
        seen |= {("list", text), ("sep", sep_len), ("sfx", len(suffix)), ("lw", last_whole), ("keep", keep_sep)}
        seen |= {("status", s) for s in set(want[2])} | {("align", (o + lead) % 16) for o in offs[:-1]} | {("oalign", o % 16) for o in want[1][:-1]}
        assert want[2][0] != 0 and want[2][-1] != 0                                     # a rejected record first and last
        second += sum(1 for s, k in zip(want[2], want[5]) if s == 1 and k != ranges[0][0])
        if name != "swap":
            assert prog.last_batch_stats.docs_routed == 0
    assert len(seen) == 6 + 4 + 3 + 2 + 2 + 3 + 16 + 16, sorted(seen)
    assert second > 16                                                                  # records whose first selected field was accepted, a later one not
    n = 0
    for text in LISTS:                                                                  # the small batch: every list with every framing
        for sep_len in (0, 1, 2, 8):
            for keep_sep in (False, True):
                data, offs = single._pack(small, sep_len)
                _check(prog, blob, data, offs, P(text), lead=(5 * n + 3) % 16, sep_len=sep_len, last_whole=bool(n & 1), keep_sep=keep_sep,
                       suffix=(b"", b"\n", b"<<eor>>\n")[n % 3])
                n += 1


def test_no_records_and_single_records():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    assert _check(prog, blob, b"", [0], P("2,4"))[1] == [0]
    assert _check(prog, blob, b"", [0, 0], P("1-"), suffix=b"\n") == (b"<>\n", [0, 3], [0], [0], [0], [0])      # the empty body: one empty field, run
    assert _check(prog, blob, b"", [0, 0], P("1-2"), suffix=b"\n") == (b"", [0, 0], [2], [1], [0], [2])         # … and no second one: nothing runs
    assert _check(prog, blob, b"\n", [0, 1], P("1"), sep_len=1) == (b"<>\n", [0, 3], [0], [0], [0], [0])        # the lone separator
    assert _check(prog, blob, b"ab;c,d;e;f\r\n", [0, 12], P("2,4"), sep_len=2, keep_sep=False, suffix=b"$")[0] == b"ab;<c> | <d>;e;<f>$"
    assert _check(prog, blob, b"ab;c;e;f\r\n", [0, 10], P("2-3"), sep_len=2, last_whole=True)[0] == b"ab;<c>;<e>;f\r\n"   # (rest, not separator)
    assert _check(prog, blob, b";;;", [0, 3], P("1-"))[0] == b"<>;<>;<>;<>"
    assert _check(prog, blob, b";;;", [0, 3], P("2,4"))[0] == b";<>;;<>"
    want = _check(prog, blob, b"ab;c;e1;f1\n", [0, 11], P("2-"), sep_len=1)
    assert want[2:] == ([1], [_want(blob, b"e1")[0]], [0], [3]) and want[3][0] < 3                              # the lowest rejected field; S counts inside it
    assert _check(prog, blob, b"ab;c\n", [0, 5], P("1,3-4,6-"), sep_len=1)[2:] == ([2], [2], [0], [3])            # K: the first field it lacks
    assert _check(prog, blob, b"a;b;c;d;e\n", [0, 10], P("1,3-4,6-"), sep_len=1)[2:] == ([2], [5], [0], [6])


def test_more_than_one_grid_stride_in_every_kernel():
    """The per-record kernels (k_flcount, k_fllocate, k_flsplen) launch at most 4 workgroups of 512 lanes per CU and stride over
    the rest; the per-granule kernels (k_fgather, k_flsplice) at most 16 workgroups of 256 lanes per CU, 16 bytes a lane.  A batch
    beyond both: short records picked from a small pool, so that the model and the oracle run once per pool entry and the
    expectation is put together from the picks."""
    import numpy as np
    import torch
    blob = blob_of(FIELDS)
    prog = Program(blob)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = ncu * 4 * 512 + 75000
    r = random.Random(22)
    ranges = P("2,4")
    word = lambda k: bytes(r.choice(b"abc,") for _ in range(k))   # noqa: E731
    pool = [word(r.randrange(0, 5)) + FS + word(r.randrange(18, 34)) + FS + word(r.randrange(0, 5)) + FS + word(r.randrange(18, 34)) + FS + word(2) + b"\n"
            for _ in range(80)]
    pool += [word(3) + FS + word(20) + FS + FS + word(9) + b"7" + word(9) + FS + b"x\n" for _ in range(6)]   # rejected inside the second selected field
    pool += [word(12) + b"\n", b"\n", word(3) + FS + b"a" + FS + b"\n", FS * 3 + b"\n"]          # one field; one empty; three; four empty ones
    want = [_expected(blob, p, [0, len(p)], ranges, sep_len=1, suffix=b"|") for p in pool]
    flen = np.array([sum(len(f) for _, f in m[1]) if isinstance(m, tuple) else 0 for p in pool
                     for m in host.field_list_records_model(p, [0, len(p)], 1, False, ranges, FS)], dtype=np.int64)
    picks = np.array([r.randrange(len(pool)) for _ in range(n)], dtype=np.int64)
    picks[0], picks[-1], picks[n // 2] = len(pool) - 4, 83, len(pool) - 3                          # a short record first, a rejected one last
    data = b"".join(pool[i] for i in picks.tolist())
    plen, olen = np.array([len(p) for p in pool], dtype=np.int64), np.array([len(w[0]) for w in want], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(plen[picks])))
    ooff = np.concatenate(([0], np.cumsum(olen[picks])))
    stride_bytes = ncu * 16 * 256 * 16
    assert n > ncu * 4 * 512 and int(flen[picks].sum()) > stride_bytes and int(ooff[-1]) > stride_bytes   # a second pass in all five
    lead = 5
    v = torch.frombuffer(bytearray(LEAD[:lead] + data + TRAIL), dtype=torch.uint8).cuda()
    o = torch.from_numpy(offs + lead).cuda()
    out, goff, status, fpos, fstage, ffield = prog.run_batch_field_list_tensor(v, o, ranges, fs=FS, sep_len=1, suffix=b"|")
    torch.cuda.synchronize()
    col = lambda k: np.array([w[k][0] for w in want])[picks]   # noqa: E731
    assert np.array_equal(goff.cpu().numpy(), ooff)
    assert np.array_equal(status.cpu().numpy(), col(2)) and np.array_equal(fpos.cpu().numpy(), col(3)) and np.array_equal(ffield.cpu().numpy(), col(5))
    assert int(fstage.sum()) == 0 and set(col(5).tolist()) == {0, 2, 4}
    got, exp = out.cpu().numpy().tobytes(), b"".join(want[i][0] for i in picks.tolist())
    assert got == exp, next(i for i in range(n) if got[ooff[i]:ooff[i + 1]] != exp[ooff[i]:ooff[i + 1]])
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.docs_routed) == (n, int(np.count_nonzero(col(2))), 0)


# ---------------------------------------------------------------------------------------------------------- 2. liveness
def _liveness_bodies():
    """test_records_field_gpu's cases, each with its first special byte at every offset of a granule, and three fields behind it."""
    cases = [b'"x;y";B;C', b'"x"";y";B', b'x\\;y;B;C', b'x\\";y";B', b'x\\\\;B;C', b'"x\\";y;B', b';";";;"";', b'\\', b'"', b'a;b\\']
    bodies, pos = [], 0
    for t in range(16):
        for c in cases:
            k = min(i for i in range(len(c)) if c[i] in b';"\\')
            bodies.append(b"a" * ((t - pos - k) % 16) + c + b";p;;q")
            pos += len(bodies[-1]) + 1
    return bodies


@pytest.mark.parametrize("quote,escape", [(b'"', None), (None, b"\\"), (b'"', b"\\")])
def test_quote_and_escape_liveness_at_every_granule_offset(quote, escape):
    blob = blob_of(COPY)
    prog = Program(blob)
    data, offs = host.pack_batch([b + b"\n" for b in _liveness_bodies()])
    plain = host.field_list_records_model(data, offs, 1, False, P("2-3"), FS)
    model = host.field_list_records_model(data, offs, 1, False, P("2-3"), FS, quote, escape)
    assert sum(1 for a, b in zip(plain, model) if a != b) >= 16                      # the quote and the escape decide
    for text in ("1,3", "2-3", "2-", "1,3-4,6-", "1-"):
        want = _check(prog, blob, data, offs, P(text), lead=3, quote=quote, escape=escape, sep_len=1)
        assert 0 in want[2] and (text != "1,3-4,6-" or 2 in want[2])                  # (every body has three fields or more; few have six)


@pytest.mark.parametrize("quote,escape", [(None, None), (b'"', None), (b'"', b"\\")])
def test_a_one_field_list_is_the_single_field_path_bit_for_bit(quote, escape):
    import torch
    blob = blob_of(FIELDS)
    prog = Program(blob)
    r = random.Random(5)
    bodies = single._bodies(r, "fields", 1500) + (_liveness_bodies() if quote or escape else [])
    seen = set()
    for K, sep_len, last_whole, keep_sep, suffix, lead in ((1, 1, False, True, b"", 0), (2, 2, True, False, b"|", 7), (3, 0, False, True, b"12345678", 13),
                                                           (4, 8, True, True, b"\n", 2)):
        data, offs = single._pack(bodies, sep_len)
        v, o = single._device(data, offs, lead)
        kw = dict(fs=FS, quote=quote, escape=escape, sep_len=sep_len, last_whole=last_whole, keep_sep=keep_sep, suffix=suffix)
        one = prog.run_batch_fields_tensor(v, o, K, **kw)
        for ranges in ([K], P("%d-%d" % (K, K))):
            lst = prog.run_batch_field_list_tensor(v, o, ranges, **kw)
            torch.cuda.synchronize()
            for a, b in zip(one, lst[:5]):
                assert torch.equal(a, b), (K, kw)
            assert torch.equal(lst[5], torch.where(lst[2] != 0, K, 0))
            seen |= set(lst[2].tolist())
    assert seen == {0, 1, 2}                                                          # (over the four K: the bodies have one to three fields, some more)


# ---------------------------------------------------------------------------------------------------------- 3. the route, an open range
def test_one_long_selected_field_takes_the_route():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    r = random.Random(3)
    long_field = bytes(r.choice(b"abc,") for _ in range(70 << 10))                   # above batch_doc_max (64 KiB)
    bodies = [b"ab;c,d;e;f", b"x;y;z;w1", b"k;l"] * 20 + [b"pre;" + long_field + b";mid;post"] + [b"ab;c,d;e;", b"", b"x;;z;;;"] * 20
    data, offs = single._pack(bodies, 1)
    want = _check(prog, blob, data, offs, P("2,4-"), lead=7, sep_len=1, suffix=b"|")
    assert prog.last_batch_stats.docs_routed == 1 and set(want[2]) == {0, 1, 2}
    short = [b for b in bodies if len(b) < 100]
    d2, o2 = single._pack(short, 1)
    w2 = _check(prog, blob, d2, o2, P("2,4-"), lead=7, sep_len=1, suffix=b"|")        # the neighbours alone: the same outputs
    assert prog.last_batch_stats.docs_routed == 0
    i = 60
    assert want[0][:want[1][i]] + want[0][want[1][i + 1]:] == w2[0] and want[2][:i] + want[2][i + 1:] == w2[2]


def test_five_thousand_empty_fields_under_an_open_range():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    bodies = [b"a;b;c", FS * 4999, b"a;b", b"x;y;z;1"]
    data, offs = single._pack(bodies, 1)
    want = _check(prog, blob, data, offs, P("3-"), lead=9, sep_len=1)
    assert want[2] == [0, 0, 2, 1] and want[5] == [0, 0, 3, 4]
    assert want[0][want[1][1]:want[1][2]] == b";;" + b";".join([b"<>"] * 4998) + b"\n"


# ---------------------------------------------------------------------------------------------------------- 4. capacity, offsets
def _raw(prog, v, o, spec, cap, guard=0, null_ff=False):
    """kx_run_batch_field_list through the C ABI: (rc, out_len, out bytes with the guard, out_off, docs words, fail_field, stats)."""
    import torch
    n = o.numel() - 1
    out = torch.full((max(cap + guard, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    ooff = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    docs = torch.full((max(n, 1), 2), -1, dtype=torch.int64, device="cuda")
    ff = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    ol, st = ctypes.c_size_t(), host.KxBatchStats()
    rc = prog._lib.kx_run_batch_field_list(prog._h, ctypes.c_void_p(v.data_ptr() if v.numel() else None), ctypes.c_void_p(o.data_ptr()), n, spec,
                                           ctypes.c_void_p(out.data_ptr() if cap else None), cap, ctypes.c_void_p(ooff.data_ptr()),
                                           ctypes.c_void_p(docs.data_ptr()), ctypes.c_void_p(None if null_ff else ff.data_ptr()), ctypes.byref(ol), ctypes.byref(st),
                                           None)
    torch.cuda.synchronize()
    return rc, ol.value, out.cpu().numpy().tobytes(), ooff.tolist(), docs.tolist(), ff.tolist(), st


def _spec(text, **kw):
    suffix = kw.pop("suffix", b"")
    arr, nr = host._field_range_array(P(text))
    f = host.KxBatchFieldList(size=ctypes.sizeof(host.KxBatchFieldList), n_ranges=nr, ranges=arr, fs=FS[0], quote=-1, escape=-1, suffix_len=len(suffix), **kw)
    f.suffix[:len(suffix)] = suffix
    return f


def test_size_query_and_capacity():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    bodies = [b"q;ab,c;r;s", b";;;", b"q;a;b;c1", b"abc", b"z;9;;", b"", b"x;y;z;w;v"] * 9
    data, offs = single._pack(bodies, 2)
    v, o = single._device(data, offs, 5)
    f = _spec("2,4-", sep_len=2, keep_sep=1, suffix=b"\r\n!")
    want = _expected(blob, data, offs, P("2,4-"), sep_len=2, suffix=b"\r\n!")
    need = len(want[0])
    assert set(want[2]) == {0, 1, 2} and need > 100
    rc, ol, _, ooff, docs, ff, st = _raw(prog, v, o, ctypes.byref(f), 0)
    assert (rc, ol) == (-3, need) and ooff == want[1] and st.out_bytes == need      # the size query fills offsets and records
    assert [d[1] & 0xFFFFFFFF for d in docs] == want[2] and [d[0] for d in docs] == want[3] and ff == want[5]
    rc, ol, out, ooff, docs, ff, _ = _raw(prog, v, o, ctypes.byref(f), need - 1)
    assert (rc, ol) == (-3, need) and out == b"\xee" * (need - 1)                   # one byte short: nothing written
    assert ooff == want[1] and [d[1] & 0xFFFFFFFF for d in docs] == want[2] and ff == want[5]
    for at in (0, 3):                                                               # the exact capacity, at two alignments of the output
        import torch
        buf = torch.full((at + need + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        res = prog.run_batch_field_list_tensor(v, o, P("2,4-"), fs=FS, sep_len=2, suffix=b"\r\n!", out=buf[at:at + need])
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == b"\xee" * at + want[0] + b"\xee" * 64 and res[1].tolist() == want[1]
    rc, ol, out, ooff, _, _, st = _raw(prog, v, o, ctypes.byref(f), need, guard=48)
    assert (rc, ol, out, ooff) == (1, need, want[0] + b"\xee" * 48, want[1])        # nothing behind out_len
    assert st.docs_rejected == sum(1 for s in want[2] if s) and st.docs == len(bodies)
    rc, ol, out, _, _, ff, _ = _raw(prog, v, o, ctypes.byref(f), need, null_ff=True)   # a null fail_field array is allowed
    assert (rc, ol, out) == (1, need, want[0]) and set(ff) == {-1}


def test_bad_ranges_are_refused_on_the_device():
    blob = blob_of(COPY)
    prog = Program(blob)
    data, offs = host.pack_batch([b"a;b\r\n", b"\n", b"d;e\r\n", b"\r"])
    v, o = single._device(data, offs, 2)
    cap = 64
    for f in (_spec("1-", sep_len=2), _spec("1,3", sep_len=2, last_whole=1), _spec("2", sep_len=8)):   # a range shorter than its separator
        rc, _, out, ooff, _, ff, _ = _raw(prog, v, o, ctypes.byref(f), cap)
        assert rc == -4 and out == b"\xee" * cap and "shorter" in prog._err() and set(ooff) == {-1} and set(ff) == {-1}, prog._err()
    data2, offs2 = host.pack_batch([b"a;b\r\n", b"\r\n", b"d;e\r\n", b"\r"])
    v2, o2 = single._device(data2, offs2, 2)
    rc, ol, out, ooff, _, ff, _ = _raw(prog, v2, o2, ctypes.byref(_spec("1-", sep_len=2, last_whole=1)), cap)   # (the short LAST range is whole)
    assert (rc, out[:ol], ooff, ff) == (0, b"a;bd;e\r", [0, 3, 3, 6, 7], [0, 0, 0, 0])
    dec = o2.clone()
    dec[2] = 1
    rc, _, out, ooff, _, _, _ = _raw(prog, v2, dec, ctypes.byref(_spec("1-", sep_len=2)), cap)
    assert rc == -4 and out == b"\xee" * cap and "decrease" in prog._err() and set(ooff) == {-1}


# ---------------------------------------------------------------------------------------------------------- 5. 6. the binary
LIST = "2,4-"


def _stream(mode, seed=11):
    """test_records_field_gpu's stream (records of 0 to 13 pieces, a 14 KiB record, a rejected one), with a tail of five fields."""
    return single._stream(mode, seed) + b";x;y"


def _want_stream(blob, data, mode, ranges, chomp, ors):
    _, kw, model_offsets, sep, _ = single.MODES[mode]
    out, err, res = [], [], []
    model = host.field_list_records_model(data, model_offsets(data), len(sep), single._tail(model_offsets, data), ranges, FS, kw.get("quote"),
                                          kw.get("escape"))
    for i, m in enumerate(model):
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


@pytest.mark.parametrize("mode", sorted(single.MODES))
def test_binary_field_list_whole_and_in_small_windows(tmp_path_factory, mode):
    blob, exe = blob_of(WHOLE), single._bin(tmp_path_factory, WHOLE)
    data = _stream(mode)
    assert len(data) > 8 * 4096
    for framing, chomp, ors in (([], False, b""), (["--chomp", "--ors=\\n"], True, b"\n")):
        out, err, res = _want_stream(blob, data, mode, P(LIST), chomp, ors)
        kinds = {("nofield" if r[0] == "nofield" else "rejected") if isinstance(r, tuple) else "ok" for r in res}
        assert kinds == {"ok", "rejected", "nofield"} and not isinstance(res[-1], tuple)
        assert {r[2] for r in res if isinstance(r, tuple) and r[0] != "nofield"} >= {2, 4}        # the line names the rejected field
        for window in (1 << 30, 4096):
            r = single._run_bin(exe, single.MODES[mode][0] + ["--field=" + LIST, "--fs=;"] + framing, data, window)
            assert r.returncode == 1, (r.returncode, r.stderr[-500:])
            assert r.stderr == err, (window, r.stderr[:300], err[:300])
            assert r.stdout == out, (window, len(r.stdout), len(out), next(i for i in range(min(len(out), len(r.stdout)) + 1) if r.stdout[i:i + 1] != out[i:i + 1]))
    # every record accepted: status 0, nothing on stderr
    r = single._run_bin(exe, single.MODES[mode][0] + ["--field=1,3-", "--fs=;"], b"ab;c;d;e", 4096)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", b"[ab];c;[d];[e]")


@pytest.mark.parametrize("mode", sorted(single.MODES))
def test_run_records_with_a_field_list(mode):
    _, kw, _, _, _ = single.MODES[mode]
    blob = blob_of(WHOLE)
    prog = Program(blob)
    data = _stream(mode, seed=12)
    for fields, chomp, ors in ((P(LIST), False, b""), ([1, (3, 4)], True, b"\n"), ([(2, None)], True, b"12345678")):
        _, _, want = _want_stream(blob, data, mode, host._check_field_ranges(fields), chomp, ors)
        got = prog.run_records(data, chomp=chomp, ors=ors, fields=fields, fs=FS, **kw)
        got = [("nofield", g.fields) if isinstance(g, NoFieldError) else (g.pos, g.stage, g.field) if isinstance(g, MatchError) else g for g in got]
        assert got == want, (mode, fields, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w))
    assert prog.run_records(b"", fields=[2, 4], fs=FS, **kw) == []
