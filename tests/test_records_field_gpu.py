"""GPU: field mode — kx_run_batch_fields (Program.run_batch_fields_tensor), Program.run_records(field=, fs=) and
`BIN --records … --field=K --fs=F`.  Every record's expected result is built in Python: host.field_records_model cuts the record,
the CPU oracle runs on the model's field alone, and prefix + oracle output + rest + separator + suffix is spliced here."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest
from conftest import blob_of

from kleenexlang_amd import build, host
from kleenexlang_amd.host import MatchError, NoFieldError, Program
from oracle import oracle

pytestmark = pytest.mark.gpu

KEXC = os.path.join(build.OUT, "kexc")
COPY = 'main := /[^\\n]*/\n'                                                       # copy-through; a newline is rejected
FIELDS = 'main := f (~/,/ " | " f)*\nf := "<" /[a-z]*/ ">"\n'                      # constants around every part; digits are rejected
TWO = 'start: low >> up\nlow := (~/A/ "a" | /[a-z]/)*\nup := (~/a/ "A" | /[b-y]/)*\n'   # stage 0 rejects what is no letter, stage 1 a z
SWAP = 'main := a@/[a-z]*/ ~/,/ b@/[0-9]*/ !b "," !a\n'                            # register actions: the two parts swapped
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)                # granule, checkpoint and piece borders
FS = b";"                                                                          # no grammar here takes it
JUNK = b"\n1\n9\n\n1\n"                                                           # separator bytes: nothing any of the grammars accepts
LEAD, TRAIL = b";\n1;;\n9;\n;1\n;;9\n;", b";;\n1;"                                 # in front of off[0] and behind off[n]: field separators too


def _want(blob, doc, cache={}):
    k = (blob, doc)
    if k not in cache:
        try:
            cache[k] = oracle.run(blob, doc)
        except oracle.OracleMatchError as e:
            cache[k] = (e.pos, e.stage)
    return cache[k]


def _expected(blob, data, offs, field, fs=FS, quote=None, escape=None, sep_len=0, last_whole=False, keep_sep=True, suffix=b""):
    """(output bytes, output offsets, status, fail_pos, fail_stage) from the model, the oracle and a splice in Python."""
    out, ooff, status, fpos, fstage = [], [0], [], [], []
    for m in host.field_records_model(data, offs, sep_len, last_whole, field, fs, quote, escape):
        w = _want(blob, m[1]) if isinstance(m, tuple) else None
        if w is None or isinstance(w, tuple):
            s = (m, 2, 0) if w is None else (w[0], 1, w[1])
            fpos.append(s[0]); status.append(s[1]); fstage.append(s[2])
            ooff.append(ooff[-1])
        else:
            status.append(0); fpos.append(0); fstage.append(0)
            out.append(m[0] + w + m[2] + (m[3] if keep_sep else b"") + suffix)
            ooff.append(ooff[-1] + len(out[-1]))
    return b"".join(out), ooff, status, fpos, fstage


def _device(data, offs, lead):
    """data at `lead` bytes into a buffer of junk (so that off[0] = lead), junk behind it."""
    import torch
    v = torch.frombuffer(bytearray(LEAD[:lead] + data + TRAIL), dtype=torch.uint8).cuda()
    assert v.data_ptr() % 16 == 0
    o = torch.tensor([x + lead for x in offs], dtype=torch.int64).cuda()
    return v, o


def _check(prog, blob, data, offs, field, lead=0, **kw):
    import torch
    want = _expected(blob, data, offs, field, **kw)
    v, o = _device(data, offs, lead)
    kw.setdefault("fs", FS)
    out, ooff, status, fpos, fstage = prog.run_batch_fields_tensor(v, o, field, **kw)
    torch.cuda.synchronize()
    got = (out.cpu().numpy().tobytes(), ooff.tolist(), status.tolist(), fpos.tolist(), fstage.tolist())
    ctx = (field, lead, kw)
    for name, g, w in zip(("status", "fail_pos", "fail_stage", "out_off"), (got[2], got[3], got[4], got[1]), (want[2], want[3], want[4], want[1])):
        if g != w:
            i = next(k for k in range(len(w)) if g[k] != w[k])
            raise AssertionError("%s[%d]: got %r, want %r (record %r, %r)" % (name, i, g[i], w[i], data[offs[min(i, len(offs) - 2)]:offs[min(i, len(offs) - 2) + 1]][:80], ctx))
    assert got[0] == want[0], (ctx, next((i, data[offs[i]:offs[i + 1]][:80], got[0][want[1][i]:want[1][i + 1]][:80]) for i in range(len(offs) - 1)
                                         if got[0][want[1][i]:want[1][i + 1]] != want[0][want[1][i]:want[1][i + 1]]))
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.out_bytes) == (len(offs) - 1, sum(1 for s in want[2] if s), len(want[0]))
    return want


# ---------------------------------------------------------------------------------------------------------- 1. model + oracle
def _part(r, name, L, bad):
    """A field of L bytes for the program `name`; `bad`: one the program rejects (where L allows it)."""
    if name == "swap":
        if L == 0:
            return b""                                                              # (no comma: rejected)
        w, n = L // 2, L - L // 2 - 1
        b = bytearray(bytes(r.choice(b"abcdefgh") for _ in range(w)) + b"," + bytes(r.choice(b"0123456789") for _ in range(n)))
        if bad:
            b[-1] = 0x78                                                            # an x among the digits, or no comma
        return bytes(b)
    alphabet, reject = {"copy": (b"abcxyz ,", b"\n"), "fields": (b"abc,", b"19"), "two": (b"Aabcxy", b"z1")}[name]
    b = bytearray(r.choice(alphabet) for _ in range(L))
    if bad and L:
        b[r.randrange(L)] = r.choice(reject)
    return bytes(b)


def _bodies(r, name, n):
    """n bodies of one to three fields out of a pool (so that the oracle runs once per pool entry), the fields' lengths at
    LENGTHS and one below — prefix, field and rest then lie at the borders.  Records that the program rejects (K = 1) or that have
    a single field (K > 1) stand first, last and in a run in the middle."""
    sizes = sorted(set(LENGTHS) | {L - 1 for L in LENGTHS if L})
    pool = {L: [_part(r, name, L, False), _part(r, name, L, False), _part(r, name, L, True)] for L in sizes}
    part = lambda: r.choice(pool[r.choice(sizes)])   # noqa: E731
    bodies = [FS.join(part() for _ in range(r.choice((1, 2, 2, 3, 3, 3)))) for _ in range(n)]
    bad1 = pool[17][2]
    bodies[0] = bodies[-1] = bad1
    bodies[n // 2:n // 2 + 5] = [bad1, pool[0][0], bad1, pool[64][2], bad1]
    bodies[n // 3:n // 3 + 3] = [b"", b"", FS + FS]                                   # empty bodies side by side, three empty fields
    return bodies


def _pack(bodies, sep_len):
    return host.pack_batch([b + (JUNK * 2)[:sep_len] for b in bodies])


PROGRAMS = {"copy": (COPY, {}), "fields": (FIELDS, {}), "two": (TWO, {}), "swap": (SWAP, {"batch_actions": 2})}


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_batch_fields_against_model_and_oracle(name):
    src, cfg = PROGRAMS[name]
    blob = blob_of(src)
    prog = Program(blob, config=host.config_from_env({}, **cfg))
    r = random.Random(len(name))
    big, small = _bodies(r, name, 3000), _bodies(r, name, 160)
    # the large batch (more than a wave and a workgroup; more than one grid stride is test_more_than_one_grid_stride_in_every_kernel's):
    # every start alignment, and every value of every option at least once
    seen = set()
    for lead in range(16):
        sep_len, K, suffix = (0, 1, 2, 8)[lead % 4], (1, 2, 3, 4)[(lead // 4 + lead) % 4], (b"", b"|", b"12345678")[lead % 3]
        last_whole, keep_sep = bool(lead & 1) ^ bool(lead & 4), bool(lead & 2) ^ bool(lead & 8)
        data, offs = _pack(big, sep_len)
        want = _check(prog, blob, data, offs, K, lead=lead, sep_len=sep_len, last_whole=last_whole, keep_sep=keep_sep, suffix=suffix)
        seen |= {("sep", sep_len), ("K", K), ("sfx", len(suffix)), ("lw", last_whole), ("keep", keep_sep)}
        seen |= {("status", s) for s in set(want[2])} | {("align", (o + lead) % 16) for o in offs[:-1]} | {("oalign", o % 16) for o in want[1][:-1]}
        assert want[2][0] != 0 and (last_whole and sep_len or want[2][-1] != 0)      # a rejected or a no-field record first and last
        if name != "swap":
            assert prog.last_batch_stats.docs_routed == 0
    assert len(seen) == 4 + 4 + 3 + 2 + 2 + 3 + 16 + 16, sorted(seen)
    # the small batch: the options' whole cross product
    for n, (sep_len, last_whole, keep_sep, suffix, K) in enumerate(itertools.product((0, 1, 2, 8), (False, True), (False, True),
                                                                                     (b"", b"\n", b"<<eor>>\n"), (1, 2, 3, 4))):
        data, offs = _pack(small, sep_len)
        _check(prog, blob, data, offs, K, lead=(5 * n + 3) % 16, sep_len=sep_len, last_whole=last_whole, keep_sep=keep_sep, suffix=suffix)


def test_no_records_and_single_records():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    assert _check(prog, blob, b"", [0], 1)[1] == [0]
    assert _check(prog, blob, b"", [0, 0], 1, suffix=b"\n") == (b"<>\n", [0, 3], [0], [0], [0])       # the empty body: one empty field, run
    assert _check(prog, blob, b"", [0, 0], 2, suffix=b"\n") == (b"", [0, 0], [2], [1], [0])           # … and no second one: not run
    assert _check(prog, blob, b"\n", [0, 1], 1, sep_len=1) == (b"<>\n", [0, 3], [0], [0], [0])        # the lone separator
    assert _check(prog, blob, b"ab;c,d;e\r\n", [0, 10], 2, sep_len=2, keep_sep=False, suffix=b"$")[0] == b"ab;<c> | <d>;e$"
    assert _check(prog, blob, b"ab;c,d;e\r\n", [0, 10], 2, sep_len=2, last_whole=True)[0] == b"ab;<c> | <d>;e\r\n"   # (rest, not separator)
    want = _check(prog, blob, b"ab;c1;e\n", [0, 8], 2, sep_len=1)
    assert want[2] == [1] and want[3] == [_want(blob, b"c1")[0]] and want[3][0] < 3                   # S counts inside the field


def test_more_than_one_grid_stride_in_every_kernel():
    """The per-record kernels (k_flocate, k_fsplen) launch at most 4 workgroups of 512 lanes per CU and stride over the rest; the
    per-granule kernels (k_fgather, k_fsplice) at most 16 workgroups of 256 lanes per CU, 16 bytes a lane.  A batch beyond both:
    records picked from a small pool, so that the model and the oracle run once per pool entry and the expectation is put together
    from the picks."""
    import numpy as np
    import torch
    blob = blob_of(FIELDS)
    prog = Program(blob)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = ncu * 4 * 512 + 75000
    r = random.Random(21)
    word = lambda k: bytes(r.choice(b"abc,") for _ in range(k))   # noqa: E731
    pool = [word(r.randrange(0, 9)) + FS + word(r.randrange(40, 72)) + FS + word(r.randrange(0, 9)) + b"\n" for _ in range(80)]
    pool += [word(5) + FS + word(20) + b"7" + word(20) + FS + b"x\n" for _ in range(6)]       # rejected inside the field
    pool += [word(12) + b"\n", b"\n", word(3) + FS + b"\n", FS + FS + b"\n"]                  # one field; one empty; an empty second field
    want = [_expected(blob, p, [0, len(p)], 2, sep_len=1, suffix=b"|") for p in pool]
    flen = np.array([len(m[1]) if isinstance(m, tuple) else 0 for p in pool
                     for m in host.field_records_model(p, [0, len(p)], 1, False, 2, FS)], dtype=np.int64)
    picks = np.array([r.randrange(len(pool)) for _ in range(n)], dtype=np.int64)
    picks[0], picks[-1], picks[n // 2] = len(pool) - 4, 83, len(pool) - 3                          # a no-field record first, a rejected one last
    data = b"".join(pool[i] for i in picks.tolist())
    plen, olen = np.array([len(p) for p in pool], dtype=np.int64), np.array([len(w[0]) for w in want], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(plen[picks])))
    ooff = np.concatenate(([0], np.cumsum(olen[picks])))
    stride_bytes = ncu * 16 * 256 * 16
    assert n > ncu * 4 * 512 and int(flen[picks].sum()) > stride_bytes and int(ooff[-1]) > stride_bytes   # a second pass in all four
    lead = 5
    v = torch.frombuffer(bytearray(LEAD[:lead] + data + TRAIL), dtype=torch.uint8).cuda()
    o = torch.from_numpy(offs + lead).cuda()
    out, goff, status, fpos, fstage = prog.run_batch_fields_tensor(v, o, 2, fs=FS, sep_len=1, suffix=b"|")
    torch.cuda.synchronize()
    assert np.array_equal(goff.cpu().numpy(), ooff)
    assert np.array_equal(status.cpu().numpy(), np.array([w[2][0] for w in want])[picks])
    assert np.array_equal(fpos.cpu().numpy(), np.array([w[3][0] for w in want])[picks])
    assert int(fstage.sum()) == 0
    got, exp = out.cpu().numpy().tobytes(), b"".join(want[i][0] for i in picks.tolist())
    assert got == exp, next(i for i in range(n) if got[ooff[i]:ooff[i + 1]] != exp[ooff[i]:ooff[i + 1]])
    st = prog.last_batch_stats
    assert (st.docs, st.docs_rejected, st.docs_routed) == (n, int(np.count_nonzero(np.array([w[2][0] for w in want])[picks])), 0)


# ---------------------------------------------------------------------------------------------------------- 2. liveness
@pytest.mark.parametrize("quote,escape", [(b'"', None), (None, b"\\"), (b'"', b"\\")])
def test_quote_and_escape_liveness_at_every_granule_offset(quote, escape):
    blob = blob_of(COPY)
    prog = Program(blob)
    cases = [b'"x;y";B;C', b'"x"";y";B', b'x\\;y;B;C', b'x\\";y";B', b'x\\\\;B;C', b'"x\\";y;B', b';";";;"";', b'\\', b'"', b'a;b\\']
    bodies, pos, decisive = [], 0, set()
    for t in range(16):                                                              # every case with its first special byte at every offset of a granule
        for ci, c in enumerate(cases):
            k = min(i for i in range(len(c)) if c[i] in b';"\\')
            shift = (t - pos - k) % 16
            bodies.append(b"a" * shift + c)
            decisive.add((ci, (pos + shift + k) % 16))
            pos += len(bodies[-1]) + 1
    assert decisive == {(ci, t) for ci in range(len(cases)) for t in range(16)}
    data, offs = host.pack_batch([b + b"\n" for b in bodies])
    plain = host.field_records_model(data, offs, 1, False, 2, FS)
    model = host.field_records_model(data, offs, 1, False, 2, FS, quote, escape)
    assert sum(1 for a, b in zip(plain, model) if a != b) >= 16                      # the quote and the escape decide
    for K in (1, 2, 3, 4):
        want = _check(prog, blob, data, offs, K, lead=0, quote=quote, escape=escape, sep_len=1)
        assert K not in (2, 3) or {0, 2} <= set(want[2])
    q, e = quote is not None, escape is not None
    first = lambda body: host.field_records_model(body, [0, len(body)], 0, False, 1, FS, quote, escape)[0][1]   # noqa: E731
    assert first(b'"x;y";B') == (b'"x;y"' if q else b'"x')
    assert first(b'x\\;y;B') == (b"x\\;y" if e else b"x\\")
    assert first(b'x\\\\;B') == b"x\\\\"
    assert first(b'x\\";y";B') == (b'x\\"' if e or not q else b'x\\";y"')


# ---------------------------------------------------------------------------------------------------------- 3. a long field
def test_one_long_field_takes_the_route():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    r = random.Random(3)
    long_field = bytes(r.choice(b"abc,") for _ in range(70 << 10))                   # above batch_doc_max (64 KiB)
    bodies = [b"ab;c,d;e", b"x;y1;z", b"k"] * 20 + [b"pre;" + long_field + b";post"] + [b"ab;c,d;e", b"", b"x;;z"] * 20
    data, offs = _pack(bodies, 1)
    want = _check(prog, blob, data, offs, 2, lead=7, sep_len=1, suffix=b"|")
    assert prog.last_batch_stats.docs_routed == 1 and set(want[2]) == {0, 1, 2}
    short = [b for b in bodies if len(b) < 100]
    d2, o2 = _pack(short, 1)
    w2 = _check(prog, blob, d2, o2, 2, lead=7, sep_len=1, suffix=b"|")               # the neighbours alone: the same outputs
    assert prog.last_batch_stats.docs_routed == 0
    i = 60
    assert want[0][:want[1][i]] + want[0][want[1][i + 1]:] == w2[0] and want[2][:i] + want[2][i + 1:] == w2[2]


# ---------------------------------------------------------------------------------------------------------- 4. capacity
def _raw(prog, v, o, spec, cap):
    """kx_run_batch_fields through the C ABI: (rc, out_len, out bytes, out_off, docs words, stats)."""
    import torch
    n = o.numel() - 1
    out = torch.full((max(cap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    ooff = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    docs = torch.full((max(n, 1), 2), -1, dtype=torch.int64, device="cuda")
    ol, st = ctypes.c_size_t(), host.KxBatchStats()
    rc = prog._lib.kx_run_batch_fields(prog._h, ctypes.c_void_p(v.data_ptr() if v.numel() else None), ctypes.c_void_p(o.data_ptr()), n, spec,
                                       ctypes.c_void_p(out.data_ptr() if cap else None), cap, ctypes.c_void_p(ooff.data_ptr()),
                                       ctypes.c_void_p(docs.data_ptr()), ctypes.byref(ol), ctypes.byref(st), None)
    torch.cuda.synchronize()
    return rc, ol.value, out.cpu().numpy().tobytes(), ooff.tolist(), docs.tolist(), st


def _spec(**kw):
    suffix = kw.pop("suffix", b"")
    f = host.KxBatchFields(size=ctypes.sizeof(host.KxBatchFields), fs=FS[0], quote=-1, escape=-1, suffix_len=len(suffix), **kw)
    f.suffix[:len(suffix)] = suffix
    return f


def test_size_query_and_capacity():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    bodies = [b"q;ab,c;r", b";;", b"q;a1", b"abc", b"z;9", b"", b"x;y;z"] * 9
    data, offs = _pack(bodies, 2)
    v, o = _device(data, offs, 5)
    f = _spec(field=2, sep_len=2, keep_sep=1, suffix=b"\r\n!")
    want = _expected(blob, data, offs, 2, sep_len=2, suffix=b"\r\n!")
    need = len(want[0])
    assert set(want[2]) == {0, 1, 2} and need > 100
    rc, ol, _, ooff, docs, st = _raw(prog, v, o, ctypes.byref(f), 0)
    assert (rc, ol) == (-3, need) and ooff == want[1] and st.out_bytes == need      # the size query fills offsets and records
    assert [d[1] & 0xFFFFFFFF for d in docs] == want[2] and [d[0] for d in docs] == want[3]
    rc, ol, out, _, _, _ = _raw(prog, v, o, ctypes.byref(f), need - 1)
    assert (rc, ol) == (-3, need) and out == b"\xee" * (need - 1)                   # one byte short: nothing written
    rc, ol, out, ooff, _, _ = _raw(prog, v, o, ctypes.byref(f), need)
    assert (rc, ol, out, ooff) == (1, need, want[0], want[1])
    rc, ol, out, _, _, st = _raw(prog, v, o, ctypes.byref(f), need + 16)
    assert (rc, ol) == (1, need) and out == want[0] + b"\xee" * 16                  # nothing behind the last byte
    assert st.docs_rejected == sum(1 for s in want[2] if s)


def test_bad_ranges_are_refused_on_the_device():
    blob = blob_of(COPY)
    prog = Program(blob)
    data, offs = host.pack_batch([b"a;b\r\n", b"\n", b"d;e\r\n", b"\r"])
    v, o = _device(data, offs, 2)
    cap = 64
    for f in (_spec(field=1, sep_len=2), _spec(field=1, sep_len=2, last_whole=1), _spec(field=2, sep_len=8)):   # a range shorter than its separator
        rc, _, out, _, _, _ = _raw(prog, v, o, ctypes.byref(f), cap)
        assert rc == -4 and out == b"\xee" * cap and "shorter" in prog._err(), prog._err()
    data2, offs2 = host.pack_batch([b"a;b\r\n", b"\r\n", b"d;e\r\n", b"\r"])
    v2, o2 = _device(data2, offs2, 2)
    rc, ol, out, ooff, _, _ = _raw(prog, v2, o2, ctypes.byref(_spec(field=1, sep_len=2, last_whole=1)), cap)   # (the short LAST range is whole)
    assert (rc, out[:ol], ooff) == (0, b"a;bd;e\r", [0, 3, 3, 6, 7])
    dec = o2.clone()
    dec[2] = 1
    rc, _, out, _, _, _ = _raw(prog, v2, dec, ctypes.byref(_spec(field=1, sep_len=2)), cap)
    assert rc == -4 and out == b"\xee" * cap and "decrease" in prog._err()


# ---------------------------------------------------------------------------------------------------------- 5. 6. the binary
# takes every byte the records below hold but a digit: quotes, escapes and quoted or escaped separators stay in a field
WHOLE = 'main := ("[" /[a-z,;"]+/ "]" | /\\\\/ | ~/\\n/ "\\\\n" | ~/\\r/ "\\\\r")*\n'
# per mode: the binary's split arguments, run_records's keywords, the split model, the separator, and the pieces of a record
# (each leaves the quote parity even and no escape open, so that the records of the split are these records)
MODES = {
    "byte": (["--records=\\0"], dict(sep=b"\0"), lambda d: host.split_records_model(d, b"\0"), b"\0",
             [b"ab", b";", b";", b"c", b"1", b"\n"]),
    "quoted": (["--records", "--quote"], dict(quote=b'"'), lambda d: host.split_records_model(d, b"\n", b'"'), b"\n",
               [b"ab", b";", b";", b'"a\nb"', b'";"', b'"a;\n;b"', b"c", b"1"]),
    "escaped": (["--records", "--quote", "--escape"], dict(quote=b'"', escape=b"\\"), lambda d: host.split_escaped_records_model(d, b"\n", b'"', b"\\")[0], b"\n",
                [b"ab", b";", b";", b'"a\nb"', b"\\;", b"\\\\", b"\\\n", b'\\"', b'";"', b"c", b"1"]),
    "rs": (["--records", "--rs=\\r\\n"], dict(rs=b"\r\n"), lambda d: host.split_rs_records_model(d, b"\r\n")[0], b"\r\n",
           [b"ab", b";", b";", b"\n", b"\r", b"c", b"1"]),
}
_BINS = {}


def _bin(tmp_path_factory, src):
    if src not in _BINS:
        d = tmp_path_factory.mktemp("recfieldbin")
        (d / "prog.kex").write_text(src)
        r = subprocess.run([KEXC, "compile", "--quiet", str(d / "prog.kex"), "--out", str(d / "bin")], stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr
        _BINS[src] = str(d / "bin")
    return _BINS[src]


def _run_bin(exe, args, data, window):
    env = dict(os.environ, KX_WINDOW_BYTES=str(window))
    return subprocess.run(["timeout", "-k", "10", "120", exe, *args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=150)


def _tail(model_offsets, data):
    """The last record has no valid separator: appending a byte does not leave a boundary at len(data)."""
    return bool(data) and len(data) not in model_offsets(data + b"x")[:-1]


def _stream(mode, seed=11):
    """About 40 KiB of records of the mode: fields of a few bytes, a field of 14 KiB (more than three 4 KiB windows), records
    without a second field, a tail."""
    _, _, _, sep, pieces = MODES[mode]
    r = random.Random(seed)
    recs = []
    for i in range(1500):
        b = b"".join(r.choice(pieces) for _ in range(r.randrange(0, 14)))
        if mode == "rs":
            b = b.replace(b"\r\n", b"\n")                                            # (a separator inside a body would be a record's end)
            b = b[:-1] + b"c" if b.endswith(b"\r") else b
        recs.append(b)
    recs[3] = recs[4] = b""
    recs[700] = b"head;" + b"longfield," * 1400 + b";tail"
    recs[701] = b"head;" + b"longfield," * 900 + b"7;tail"                           # rejected deep inside its field
    return sep.join(recs) + sep + b"ab;c,d;last"


def _want_stream(blob, data, mode, field, chomp, ors):
    _, kw, model_offsets, sep, _ = MODES[mode]
    out, err, res = [], [], []
    model = host.field_records_model(data, model_offsets(data), len(sep), _tail(model_offsets, data), field, FS, kw.get("quote"), kw.get("escape"))
    for i, m in enumerate(model):
        w = _want(blob, m[1]) if isinstance(m, tuple) else None
        if w is None:
            err.append("Record %d has no field %d!\n" % (i + 1, field))
            res.append(("nofield", m))
        elif isinstance(w, tuple):
            err.append("Match error at input symbol %d in record %d!\n" % (w[0], i + 1))
            res.append(w)
        else:
            out.append(m[0] + w + m[2] + (b"" if chomp else m[3]) + ors)
            res.append(out[-1])
    return b"".join(out), "".join(err).encode(), res


@pytest.mark.parametrize("mode", sorted(MODES))
def test_binary_field_mode_whole_and_in_small_windows(tmp_path_factory, mode):
    blob, exe = blob_of(WHOLE), _bin(tmp_path_factory, WHOLE)
    data = _stream(mode)
    assert len(data) > 8 * 4096
    for framing, chomp, ors in (([], False, b""), (["--chomp", "--ors=\\n"], True, b"\n")):
        out, err, res = _want_stream(blob, data, mode, 2, chomp, ors)
        kinds = {("nofield" if r[0] == "nofield" else "rejected") if isinstance(r, tuple) else "ok" for r in res}
        assert kinds == {"ok", "rejected", "nofield"} and not isinstance(res[-1], tuple)
        for window in (1 << 30, 4096):
            r = _run_bin(exe, MODES[mode][0] + ["--field=2", "--fs=;"] + framing, data, window)
            assert r.returncode == 1, (r.returncode, r.stderr[-500:])
            assert r.stderr == err, (window, r.stderr[:300], err[:300])
            assert r.stdout == out, (window, len(r.stdout), len(out), next(i for i in range(min(len(out), len(r.stdout)) + 1) if r.stdout[i:i + 1] != out[i:i + 1]))
    # every record accepted: status 0, nothing on stderr; K = 1 of a stream without separators is the stream
    r = _run_bin(exe, MODES[mode][0] + ["--field=1", "--fs=;"], b"ab;c", 4096)
    assert (r.returncode, r.stderr, r.stdout) == (0, b"", b"[ab];c")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_run_records_with_a_field(mode):
    _, kw, _, _, _ = MODES[mode]
    blob = blob_of(WHOLE)
    prog = Program(blob)
    data = _stream(mode, seed=12)
    for field, chomp, ors in ((2, False, b""), (1, True, b"\n"), (3, True, b"12345678")):
        _, _, want = _want_stream(blob, data, mode, field, chomp, ors)
        got = prog.run_records(data, chomp=chomp, ors=ors, field=field, fs=FS, **kw)
        got = [("nofield", g.fields) if isinstance(g, NoFieldError) else (g.pos, g.stage) if isinstance(g, MatchError) else g for g in got]
        assert got == want, (mode, field, next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w))
    assert prog.run_records(b"", field=1, fs=FS, **kw) == []


@pytest.mark.parametrize("mode", sorted(MODES))
def test_without_a_field_nothing_changes(tmp_path_factory, mode):
    """`--records` without `--field` on the same input: the bytes of Program.run_records, whose path this option does not touch."""
    args, kw, _, _, _ = MODES[mode]
    blob, exe = blob_of(WHOLE), _bin(tmp_path_factory, WHOLE)
    prog = Program(blob)
    data = _stream(mode)
    for framing, chomp, ors in (([], False, b""), (["--chomp", "--ors=\\n"], True, b"\n")):
        res = prog.run_records(data, chomp=chomp, ors=ors, **kw)
        out = b"".join(x for x in res if not isinstance(x, MatchError))
        err = "".join("Match error at input symbol %d in record %d!\n" % (x.pos, i + 1) for i, x in enumerate(res) if isinstance(x, MatchError)).encode()
        assert err and out
        r = _run_bin(exe, args + framing, data, 4096)
        assert (r.returncode, r.stderr) == (1, err) and r.stdout == out
