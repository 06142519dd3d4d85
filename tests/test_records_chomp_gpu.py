"""GPU: record mode's framing — kx_run_batch_framed (trim, last_whole, suffix), Program.run_records(chomp=, ors=) and
`BIN --records … --chomp --ors=STR`.  Every document's expected result is the CPU oracle run on the chomped record alone
(host.chomp_records_model), its output followed by the suffix, or the oracle's failure position and stage."""
import ctypes
import os
import random
import subprocess

import pytest
from conftest import blob_of

from kleenexlang_amd import build, host
from kleenexlang_amd.host import MatchError, Program
from oracle import oracle

pytestmark = pytest.mark.gpu

KEXC = os.path.join(build.OUT, "kexc")
# no grammar here names a separator: the framing is the caller's
COPY = 'main := /[^\\n]*/\n'                                                       # copy-through; an empty record gives an empty output
FIELDS = 'main := f (~/,/ " | " f)*\nf := "<" /[a-z]*/ ">"\n'                      # constants around every field; digits are rejected
TWO = 'start: low >> up\nlow := (~/A/ "a" | /[a-z]/)*\nup := (~/a/ "A" | /[b-y]/)*\n'   # stage 0 rejects what is no letter, stage 1 a z
SWAP = 'main := a@/[a-z]*/ ~/,/ b@/[0-9]*/ !b "," !a\n'                            # register actions: the two fields swapped
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)                # granule, checkpoint and piece borders
JUNK = b"\n1\n9\n\n1\n"                                                           # trimmed bytes: nothing any of the grammars accepts


def _want(blob, doc, cache={}):
    k = (blob, doc)
    if k not in cache:
        try:
            cache[k] = oracle.run(blob, doc)
        except oracle.OracleMatchError as e:
            cache[k] = (e.pos, e.stage)
    return cache[k]


def _expected(blob, docs, suffix):
    """(output bytes, output offsets, status, fail_pos, fail_stage) for the model's documents."""
    out, ooff, status, fpos, fstage = [], [0], [], [], []
    for d in docs:
        w = _want(blob, d)
        if isinstance(w, tuple):
            status.append(1); fpos.append(w[0]); fstage.append(w[1])
            ooff.append(ooff[-1])
        else:
            status.append(0); fpos.append(0); fstage.append(0)
            out.append(w + suffix)
            ooff.append(ooff[-1] + len(w) + len(suffix))
    return b"".join(out), ooff, status, fpos, fstage


def _device(data, offs, lead):
    """data at `lead` bytes into a buffer of junk (so that off[0] = lead), one junk byte behind it."""
    import torch
    v = torch.frombuffer(bytearray(b"\n" * lead + data + b"\n"), dtype=torch.uint8).cuda()[:lead + len(data)]
    o = torch.tensor([x + lead for x in offs], dtype=torch.int64).cuda()
    return v, o


def _run(prog, data, offs, lead=0, **frame):
    import torch
    v, o = _device(data, offs, lead)
    out, ooff, status, fpos, fstage = prog.run_batch_tensor(v, o, **frame)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), ooff.tolist(), status.tolist(), fpos.tolist(), fstage.tolist()


def _check(prog, blob, data, offs, lead=0, trim=0, last_whole=False, suffix=b""):
    docs = host.chomp_records_model(data, offs, trim, last_whole)
    want = _expected(blob, docs, suffix)
    got = _run(prog, data, offs, lead, trim=trim, last_whole=last_whole, suffix=suffix)
    for name, g, w in zip(("status", "fail_pos", "fail_stage", "out_off"), (got[2], got[3], got[4], got[1]), (want[2], want[3], want[4], want[1])):
        if g != w:
            i = next(k for k in range(len(w)) if g[k] != w[k])
            raise AssertionError("%s[%d]: got %r, want %r (document %r, trim %d, lead %d, last_whole %s)" % (name, i, g[i], w[i], docs[min(i, len(docs) - 1)][:70], trim, lead, last_whole))
    assert got[0] == want[0], next((i, docs[i][:70]) for i in range(len(docs)) if got[0][want[1][i]:want[1][i + 1]] != want[0][want[1][i]:want[1][i + 1]])
    return want


def _pack(bodies, trim):
    """Every body followed by `trim` bytes of junk: (data, offsets)."""
    parts = [b + (JUNK * 2)[:trim] for b in bodies]
    return host.pack_batch(parts)


def _border_bodies(r, alphabet, reject=b""):
    """Bodies of every length in LENGTHS, several of each so that starts fall on many alignments, empty ones side by side; with
    `reject`, some bodies hold a byte the grammar refuses."""
    bodies = []
    for rep in range(3):
        for L in LENGTHS:
            b = bytearray(r.choice(alphabet) for _ in range(L))
            if reject and L and r.randrange(3) == 0:
                b[r.randrange(L)] = r.choice(reject)
            bodies.append(bytes(b))
    bodies += [b"", b"", b"", bytes(r.choice(alphabet) for _ in range(65)), b"", b""]
    r.shuffle(bodies)
    return bodies + [b"", b"", bytes(r.choice(alphabet) for _ in range(64))]        # (with last_whole the last range keeps its junk)


# ---------------------------------------------------------------------------------------------------------- 1. the trim
@pytest.mark.parametrize("trim", [1, 2, 8])
@pytest.mark.parametrize("name", ["copy", "fields"])
def test_trim_at_every_border_and_alignment(name, trim):
    src, alphabet, reject = {"copy": (COPY, b"abcxyz ,", b""), "fields": (FIELDS, b"abc,", b"19")}[name]
    blob = blob_of(src)
    prog = Program(blob)
    bodies = _border_bodies(random.Random(trim * 3 + len(name)), alphabet, reject)
    data, offs = _pack(bodies, trim)
    starts = set()
    for lead in range(1, 17):                                                       # every start alignment, off[0] != 0
        for last_whole in (False, True):
            want = _check(prog, blob, data, offs, lead=lead, trim=trim, last_whole=last_whole)
            starts |= {(o + lead) % 16 for o in offs[:-1]}
    assert starts == set(range(16))
    assert 0 in want[2] and (name == "copy" or want[2].count(1) > 3)
    assert want[2][-1] == 1                                                         # (last_whole: the junk is part of the last document, and refused)
    st = prog.last_batch_stats
    assert (st.docs, st.docs_routed) == (len(bodies), 0)


def test_trimmed_document_drops_a_piece_slot():
    """64 + trim bytes at a piece-aligned start hold two piece slots, the trimmed document one; 128 + trim three and two."""
    blob = blob_of(COPY)
    prog = Program(blob)
    for trim in (1, 8):
        for L in (64, 128):
            body = bytes(97 + i % 26 for i in range(L))
            data, offs = _pack([body] * 5 + [b""] * 3 + [body] * 4, trim)
            for lead in (64, 128 - trim, 63, 1):
                _check(prog, blob, data, offs, lead=lead, trim=trim)
                _check(prog, blob, data, offs, lead=lead, trim=trim, last_whole=True, suffix=b"|")


# ---------------------------------------------------------------------------------------------------------- 2. the suffix
@pytest.mark.parametrize("suffix", [b"", b"\n", b"\r\n;", b"12345678"])
def test_suffix_after_every_accepted_document(suffix):
    r = random.Random(len(suffix))
    aligns = set()
    for src, alphabet, reject in ((COPY, b"abcxyz", b"\n"), (FIELDS, b"abc,", b"19")):
        blob = blob_of(src)
        prog = Program(blob)
        bodies = _border_bodies(r, alphabet, reject)
        data, offs = _pack(bodies, 0)
        want = _check(prog, blob, data, offs, lead=3, suffix=suffix)
        assert want[2].count(1) > 3 and want[2].count(0) > 20                       # rejected documents between accepted ones
        aligns |= {o % 16 for o in want[1]}
        if src == COPY:                                                             # accepted documents whose own output is empty
            assert sum(1 for i, b in enumerate(bodies) if not b and want[1][i + 1] - want[1][i] == len(suffix)) >= 5
        assert prog.last_batch_stats.out_bytes == len(want[0])
        _check(prog, blob, data, offs, lead=9, trim=0, last_whole=True, suffix=suffix)   # (last_whole without a trim changes nothing)
    assert aligns == set(range(16))                                                 # output offsets of every alignment


def _raw(prog, v, o, frame, cap, framed=True):
    """kx_run_batch_framed (or kx_run_batch) through the C ABI: (rc, out_len, out bytes, out_off, docs words)."""
    import torch
    n = o.numel() - 1
    out = torch.full((max(cap, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    ooff = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    docs = torch.full((max(n, 1), 2), -1, dtype=torch.int64, device="cuda")
    ol, st = ctypes.c_size_t(), host.KxBatchStats()
    lib = prog._lib
    args = [ctypes.c_void_p(out.data_ptr() if cap else None), cap, ctypes.c_void_p(ooff.data_ptr()), ctypes.c_void_p(docs.data_ptr()),
            ctypes.byref(ol), ctypes.byref(st), None]
    head = [prog._h, ctypes.c_void_p(v.data_ptr() if v.numel() else None), ctypes.c_void_p(o.data_ptr()), n]
    rc = lib.kx_run_batch_framed(*head, frame, *args) if framed else lib.kx_run_batch(*head, *args)
    torch.cuda.synchronize()
    return rc, ol.value, out.cpu().numpy().tobytes(), ooff.tolist(), docs.tolist(), st


def _frame(trim=0, last_whole=0, suffix=b"", suffix_len=None):
    f = host.KxBatchFrame(trim=trim, last_whole=last_whole, suffix_len=len(suffix) if suffix_len is None else suffix_len)
    f.suffix[:len(suffix)] = suffix
    return f


def test_size_query_and_capacity_count_the_suffixes():
    blob = blob_of(FIELDS)
    prog = Program(blob)
    bodies = [b"ab,c", b"", b"a1", b"abc", b"9", b"", b"x,y,z"] * 9
    data, offs = _pack(bodies, 2)
    v, o = _device(data, offs, 5)
    f = _frame(trim=2, suffix=b"\r\n!")
    want = _expected(blob, host.chomp_records_model(data, offs, 2, False), b"\r\n!")
    need = len(want[0])
    assert need == sum(len(_want(blob, b)) + 3 for b in bodies if not isinstance(_want(blob, b), tuple))
    rc, ol, _, ooff, docs, st = _raw(prog, v, o, ctypes.byref(f), 0)
    assert (rc, ol) == (-3, need) and ooff == want[1] and st.out_bytes == need      # the size query fills offsets and records
    assert [d[1] & 0xFFFFFFFF for d in docs] == want[2]
    rc, ol, out, _, _, _ = _raw(prog, v, o, ctypes.byref(f), need - 1)
    assert (rc, ol) == (-3, need) and out == b"\xee" * (need - 1)                   # one byte short: nothing written
    rc, ol, out, ooff, _, _ = _raw(prog, v, o, ctypes.byref(f), need)
    assert (rc, ol, out, ooff) == (1, need, want[0], want[1])
    rc, ol, out, _, _, _ = _raw(prog, v, o, ctypes.byref(f), need + 16)
    assert (rc, ol) == (1, need) and out == want[0] + b"\xee" * 16                  # nothing behind the last suffix


# ---------------------------------------------------------------------------------------------------------- 3. no frame
def test_null_and_all_zero_frames_are_kx_run_batch():
    r = random.Random(5)
    for src, cfg in ((FIELDS, {}), (TWO, {}), (SWAP, {"batch_actions": 2}), (COPY, {"batch_doc_max": 256})):
        blob = blob_of(src)
        prog = Program(blob, config=host.config_from_env({}, **cfg))
        bodies = [bytes(r.choice(b"abcz,12A\n") for _ in range(r.choice(LENGTHS))) for _ in range(120)] + [b"ab,12", b"", b"abc" * 200]
        data, offs = host.pack_batch(bodies)
        v, o = _device(data, offs, 7)
        base = _raw(prog, v, o, None, len(data) * 6 + 64, framed=False)
        assert base[0] == 1 and {d[1] & 0xFFFFFFFF for d in base[4]} == {0, 1}      # a mixed batch
        zero = _frame()
        for frame in (None, ctypes.byref(zero)):
            got = _raw(prog, v, o, frame, len(data) * 6 + 64)
            assert got[:5] == base[:5]
            assert (got[5].docs_rejected, got[5].docs_routed, got[5].docs_replayed, got[5].out_bytes) == \
                   (base[5].docs_rejected, base[5].docs_routed, base[5].docs_replayed, base[5].out_bytes)


# ---------------------------------------------------------------------------------------------------------- 4. KX_E_ARG
def test_bad_frames_are_refused():
    blob = blob_of(COPY)
    prog = Program(blob)
    data, offs = host.pack_batch([b"abc\r\n", b"\n", b"de\r\n", b"\r"])
    v, o = _device(data, offs, 2)
    cap = 64
    untouched = b"\xee" * cap
    for f in (_frame(trim=2), _frame(trim=2, last_whole=1), _frame(trim=8), _frame(trim=0xFFFFFFFF)):   # a range shorter than the trim
        rc, _, out, _, _, _ = _raw(prog, v, o, ctypes.byref(f), cap)
        assert rc == -4 and out == untouched and "shorter" in prog._err(), prog._err()
    data2, offs2 = host.pack_batch([b"abc\r\n", b"\r\n", b"de\r\n", b"\r"])
    v2, o2 = _device(data2, offs2, 2)
    rc, ol, out, ooff, _, _ = _raw(prog, v2, o2, ctypes.byref(_frame(trim=2, last_whole=1)), cap)       # (the short LAST range is whole)
    assert (rc, out[:ol], ooff) == (0, b"abcde\r", [0, 3, 3, 5, 6])
    bad = _frame(suffix=b"12345678", suffix_len=9)
    rc, _, out, _, _, _ = _raw(prog, v2, o2, ctypes.byref(bad), cap)
    assert rc == -4 and out == untouched and "suffix" in prog._err()
    for k in range(3):
        bad = _frame(trim=2, last_whole=1)
        bad.reserved[k] = 1
        rc, _, out, _, _, _ = _raw(prog, v2, o2, ctypes.byref(bad), cap)
        assert rc == -4 and out == untouched and "reserved" in prog._err()
    dec = o2.clone()
    dec[2] = 1                                                                      # decreasing offsets are still what they were
    assert _raw(prog, v2, dec, ctypes.byref(_frame(trim=2)), cap)[0] == -4 and "decrease" in prog._err()


# ---------------------------------------------------------------------------------------------------------- 5. register actions
@pytest.mark.parametrize("trim,suffix", [(1, b"\n"), (2, b""), (8, b"12345678"), (0, b"\r\n;")])
def test_action_program_replayed_with_trim_and_suffix(trim, suffix):
    blob = blob_of(SWAP)
    r = random.Random(trim + len(suffix))
    word = lambda n: bytes(r.choice(b"abcdefgh") for _ in range(n))   # noqa: E731
    num = lambda n: bytes(r.choice(b"0123456789") for _ in range(n))  # noqa: E731
    lane = [word(r.randrange(0, 40)) + b"," + num(r.randrange(0, 40)) for _ in range(150)] + [b",", b"", b"ab", b"ab,1x", b"a,1", b","]
    for L in LENGTHS:
        lane.append(word(L // 2) + b"," + num(L - L // 2 - 1) if L else b"")
    wave = [word(3000) + b"," + num(2500), word(5000) + b",7", b"a," + num(6000)]   # more than 4 KiB of tokens: one wave each
    long_doc = word(5000) + b"," + num(4000)                                        # above batch_doc_max: the single-document route
    bodies = lane[:80] + [wave[0]] + lane[80:] + [long_doc, wave[1]] + [b"", b","] + [wave[2]]
    data, offs = _pack(bodies, trim)
    prog = Program(blob, config=host.config_from_env({}, batch_actions=2, batch_doc_max=8192))
    for lead, last_whole in ((3, False), (16, True)):
        want = _check(prog, blob, data, offs, lead=lead, trim=trim, last_whole=last_whole and trim > 0, suffix=suffix)
        st = prog.last_batch_stats
        assert st.docs_routed == 1 and st.docs_replayed == want[2].count(0) - 1, (st.docs_routed, st.docs_replayed)
        assert st.out_bytes == len(want[0]) and want[2].count(1) >= 3
    assert _want(blob, b"abc,12") == b"12,abc"
    # the lanes only (no wave, no route), and everything by the route: the same arrays
    data, offs = _pack(lane, trim)
    got = _check(prog, blob, data, offs, lead=5, trim=trim, suffix=suffix)
    assert prog.last_batch_stats.docs_routed == 0
    route = Program(blob, config=host.config_from_env({}, batch_actions=1))
    assert _check(route, blob, data, offs, lead=5, trim=trim, suffix=suffix) == got
    assert route.last_batch_stats.docs_routed == len(lane) and route.last_batch_stats.docs_replayed == 0


# ---------------------------------------------------------------------------------------------------------- 6. a pipeline
def test_pipeline_trims_before_stage_0_and_appends_after_the_last():
    blob = blob_of(TWO)
    prog = Program(blob)
    assert prog.num_stages == 2
    r = random.Random(6)
    bodies = _border_bodies(r, b"AabcxyA", reject=b"z1")                            # z: rejected in stage 1; 1: in stage 0
    for trim, suffix in ((1, b"\n"), (2, b"<<>>"), (0, b"\n"), (8, b"")):
        data, offs = _pack(bodies, trim)
        want = _check(prog, blob, data, offs, lead=11, trim=trim, suffix=suffix)
        rejected_at = {want[4][i] for i in range(len(bodies)) if want[2][i]}
        assert rejected_at == {0, 1}
    assert _want(blob, b"AbcA") == b"AbcA" and _want(blob, b"ab1")[1] == 0 and _want(blob, b"abz")[1] == 1
    # the output of stage 0 is as long as its input: a stage-1 trim would cut a letter, a stage-0 suffix would reach stage 1
    assert _run(prog, b"abc\nAz\n\nq", [0, 4, 7, 8, 9], trim=1, last_whole=True, suffix=b";")[:3] == (b"Abc;;q;", [0, 4, 4, 5, 7], [0, 1, 0, 0])


# ---------------------------------------------------------------------------------------------------------- 7. Program.run_records
def _tail(model_offsets, data):
    """The last record has no valid separator: appending a byte does not leave a boundary at len(data)."""
    return bool(data) and len(data) not in model_offsets(data + b"x")[:-1]


def _want_records(blob, data, model_offsets, trim, ors):
    """(stdout, stderr, per-record results) from the split model, the chomp model and the oracle on every chomped record."""
    docs = host.chomp_records_model(data, model_offsets(data), trim, _tail(model_offsets, data))
    out, err, res = [], [], []
    for i, d in enumerate(docs):
        w = _want(blob, d)
        if isinstance(w, tuple):
            err.append("Match error at input symbol %d in record %d!\n" % (w[0], i + 1))
            res.append(w)
        else:
            out.append(w + ors)
            res.append(w + ors)
    return b"".join(out), "".join(err).encode(), res


def _as_res(got):
    return [(g.pos, g.stage) if isinstance(g, MatchError) else g for g in got]


MODES = {
    "byte": (dict(sep=b"\0"), lambda d: host.split_records_model(d, b"\0"), 1),
    "quoted": (dict(quote=b'"'), lambda d: host.split_records_model(d, b"\n", b'"'), 1),
    "escaped": (dict(quote=b'"', escape=b"\\"), lambda d: host.split_escaped_records_model(d, b"\n", b'"', b"\\")[0], 1),
    "rs": (dict(rs=b"\r\n"), lambda d: host.split_rs_records_model(d, b"\r\n")[0], 2),
}
# the program of each mode takes what its records may hold once the separator is gone (a quoted or escaped newline stays)
MODE_SRC = {"byte": FIELDS, "quoted": 'main := ("[" /[a-z"]+/ "]" | ~/\\n/ "\\\\n")*\n', "escaped": 'main := ("[" /[a-z"]+/ "]" | /\\\\/ | ~/\\n/ "\\\\n")*\n',
            "rs": 'main := ("[" /[a-z,]+/ "]" | ~/\\n/ "\\\\n")*\n'}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_run_records_with_chomp_and_ors(mode):
    kw, model_offsets, trim = MODES[mode]
    blob = blob_of(MODE_SRC[mode])
    prog = Program(blob)
    sep = {"byte": b"\0", "rs": b"\r\n"}.get(mode, b"\n")
    r = random.Random(len(mode))
    # (every piece leaves the quote parity even and no escape open: the records of the split are these records)
    alphabet = {"byte": [b"ab", b",", b"c", b"1"], "quoted": [b"ab", b'"a\nb"', b'"\n"', b"c", b"1"],
                "escaped": [b"ab", b'"a\nb"', b"\\\\", b"\\\n", b"c", b"1"], "rs": [b"ab", b",", b"\n", b"\r", b"c"]}[mode]
    recs = [b"".join(r.choice(alphabet) for _ in range(r.randrange(0, 8))) + sep for _ in range(400)]
    recs[5], recs[6], recs[7] = sep, sep, sep                                       # records that are only the separator, side by side
    tails = {"byte": [b"", b"ab,c"], "quoted": [b"", b'ab"c\n', b'"\n'], "escaped": [b"", b"ab\\\n", b'ab"c\\"\n', b'"\n'], "rs": [b"", b"ab\r", b"\n"]}[mode]
    for tail in tails:
        data = b"".join(recs) + tail
        for chomp, ors in ((True, b"\n"), (True, b""), (False, b"<eor>\n"), (True, b"12345678")):
            _, _, want = _want_records(blob, data, model_offsets, trim if chomp else 0, ors)
            got = prog.run_records(data, chomp=chomp, ors=ors, **kw)
            assert _as_res(got) == want, (mode, tail, chomp, ors, next((i, g, w) for i, (g, w) in enumerate(zip(_as_res(got), want)) if g != w))
        assert any(isinstance(w, tuple) for w in want) and sum(not isinstance(w, tuple) for w in want) > 100
    if mode in ("quoted", "escaped"):                                               # the tail kept its quoted / escaped newline: "\n" in its output
        assert want[-1].endswith(b"\\n12345678") and not isinstance(want[5], tuple) and want[5] == b"12345678"
    assert prog.run_records(b"", chomp=True, ors=b"\n", **kw) == []
    assert _as_res(prog.run_records(sep, chomp=True, ors=b"|", **kw)) == [_want(blob, b"") + b"|"]


# ---------------------------------------------------------------------------------------------------------- 8. 9. the binary
_BINS = {}


def _bin(tmp_path_factory, src):
    if src not in _BINS:
        d = tmp_path_factory.mktemp("recchompbin")
        (d / "prog.kex").write_text(src)
        r = subprocess.run([KEXC, "compile", "--quiet", str(d / "prog.kex"), "--out", str(d / "bin")], stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr
        _BINS[src] = str(d / "bin")
    return _BINS[src]


def _run_bin(exe, args, data, window):
    env = dict(os.environ, KX_WINDOW_BYTES=str(window))
    return subprocess.run(["timeout", "-k", "10", "120", exe, *args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=150)


def _check_bin(exe, blob, data, args, model_offsets, trim, ors, window=4096):
    out, err, _ = _want_records(blob, data, model_offsets, trim, ors)
    r = _run_bin(exe, args, data, window)
    assert r.returncode == (1 if err else 0), (r.returncode, r.stderr[-500:])
    assert r.stderr == err, (r.stderr[:300], err[:300])
    assert r.stdout == out, (len(r.stdout), len(out), next(i for i in range(min(len(out), len(r.stdout)) + 1) if r.stdout[i:i + 1] != out[i:i + 1]))


def test_binary_crlf_in_lf_out_with_small_windows(tmp_path_factory):
    """4 KiB windows (the smallest the driver takes): a separator straddling a window border at both splits, a record spanning
    more than three windows, rejected records in between, with and without a terminator at the end."""
    blob, exe = blob_of(FIELDS), _bin(tmp_path_factory, FIELDS)
    W = 4096
    r = random.Random(8)
    rec = lambda: b",".join(bytes(r.choice(b"abcdef") for _ in range(r.randrange(0, 9))) for _ in range(r.randrange(1, 6)))   # noqa: E731
    recs = [rec() + (b"7" if i % 13 == 4 else b"") + b"\r\n" for i in range(700)]
    recs[300] = b",".join([b"longfield"] * 1400) + b"\r\n"                          # ≈ 14 KiB: spans more than three windows
    recs[10], recs[11] = b"\r\n", b"\r\n"
    body = b"".join(recs)
    model_offsets = lambda d: host.split_rs_records_model(d, b"\r\n")[0]   # noqa: E731
    args = ["--records", "--rs=\\r\\n", "--chomp", "--ors=\\n"]
    for k in (W - 1, W, W + 1):                                                     # the \r at byte k - 1, the \n at byte k: around a window border
        pre = b"m" * (k - 1) + b"\r\n"
        _check_bin(exe, blob, pre + body, args, model_offsets, 2, b"\n", W)
    _check_bin(exe, blob, body[:-2], args, model_offsets, 2, b"\n", W)              # a tail: run whole, and it gets its \n
    _check_bin(exe, blob, body + b"ab\r", args, model_offsets, 2, b"\n", W)         # half a separator at the end is the tail's data: rejected
    _check_bin(exe, blob, b"", args, model_offsets, 2, b"\n", W)
    _check_bin(exe, blob, b"\r\n", args, model_offsets, 2, b"\n", W)
    _check_bin(exe, blob, body, ["--records", "--rs=\\r\\n", "--ors=\\n"], model_offsets, 0, b"\n", W)      # --ors alone: every record rejected at its \r
    _check_bin(exe, blob, body, ["--records", "--rs=\\r\\n", "--chomp"], model_offsets, 2, b"", W)
    nul = body.replace(b"\r\n", b"\0")
    _check_bin(exe, blob, nul, ["--records=\\0", "--chomp", "--ors=\\n"], lambda d: host.split_records_model(d, b"\0"), 1, b"\n", W)


def test_binary_swap_records_replayed(tmp_path_factory):
    blob, exe = blob_of(SWAP), _bin(tmp_path_factory, SWAP)
    r = random.Random(4)
    recs = [bytes(r.choice(b"abcdefgh") for _ in range(r.randrange(0, 9))) + b"," + b"%d" % r.randrange(10 ** 6) + (b"x" if i % 17 == 3 else b"") + b"|~|"
            for i in range(1500)]
    data = b"".join(recs) + b"tail,99"
    model_offsets = lambda d: host.split_rs_records_model(d, b"|~|")[0]   # noqa: E731
    _check_bin(exe, blob, data, ["--records", "--rs=|~|", "--chomp", "--ors=\\r\\n"], model_offsets, 3, b"\r\n", 4096)


@pytest.mark.parametrize("spelling,sep", [("\\n", b"\n"), ("\\r\\n", b"\r\n"), ("\\0", b"\0")])
def test_copy_through_reproduces_the_input(tmp_path_factory, spelling, sep):
    src = 'main := /[^\\n\\r\\x00]*/\n'
    exe = _bin(tmp_path_factory, src)
    r = random.Random(len(sep))
    data = b"".join(bytes(r.choice(b"abc ,;x") for _ in range(r.randrange(0, 70))) + sep for _ in range(2000))
    split = ["--records", "--rs=" + spelling] if len(sep) > 1 else ["--records=" + spelling]
    for window in (4096, 1 << 20):
        res = _run_bin(exe, split + ["--chomp", "--ors=" + spelling], data, window)
        assert (res.returncode, res.stderr) == (0, b"") and res.stdout == data      # ends in a separator: byte for byte
        res = _run_bin(exe, split + ["--chomp", "--ors=" + spelling], data + b"the tail", window)
        assert (res.returncode, res.stderr) == (0, b"") and res.stdout == data + b"the tail" + sep   # a tail: the input plus one separator


# ---------------------------------------------------------------------------------------------------------- 10. no framing
# takes every byte the records below hold but a digit, the separators included: without --chomp they reach the program
WHOLE = 'main := ("[" /[a-z,"]+/ "]" | /\\\\/ | ~/\\n/ "\\\\n" | ~/\\r/ "\\\\r")*\n'
# per mode: the keywords of MODES as the C arguments of the mode's own entry point and as kx_records_opts fields; the pieces of a
# record (each leaves the quote parity even and no escape open); (piece, k): a piece to lay with its byte k on a window border —
# a record, open quotes, an open escape, half a separator then cross it; and a tail
PLAIN = {
    "byte": ("kx_run_records_fd", (10,), dict(mode=host.KX_RECORDS_BYTE, sep=10, quote=-1, escape=-1),
             [b"ab", b",", b"c"], [(b"ab", 1)], b"ab,c"),
    "quoted": ("kx_run_records_fd_quoted", (10, 34), dict(mode=host.KX_RECORDS_QUOTED, sep=10, quote=34, escape=-1),
               [b"ab", b'"a\nb"', b'"\n"', b"c"], [(b'"a\nb"', 2)], b'ab"c\n'),
    "escaped": ("kx_run_records_fd_escaped", (10, 34, 92), dict(mode=host.KX_RECORDS_ESCAPED, sep=10, quote=34, escape=92),
                [b"ab", b'"a\nb"', b"\\\\", b"\\\n", b"c"], [(b"\\\n", 1), (b'"a\nb"', 2)], b'ab"c\\"\n'),
    "rs": ("kx_run_records_fd_rs", (b"\r\n", 2), dict(mode=host.KX_RECORDS_RS, rs_len=2, quote=-1, escape=-1),
           [b"ab", b",", b"\n", b"\r", b"c"], [(b"ab\r\n", 3)], b"ab\r"),
}


@pytest.mark.parametrize("mode", sorted(PLAIN))
def test_opts_without_framing_is_the_modes_own_entry_point(mode, tmp_path, monkeypatch):
    """include/kxhip.h: with chomp = 0 and ors_len = 0, kx_run_records_fd_opts is the entry point of its mode — the same output,
    report, return code and counts, over 4 KiB windows with a record, the quote parity, an escape and half a separator crossing
    their borders, rejected records in between and a tail."""
    W = 4096
    monkeypatch.setenv("KX_WINDOW_BYTES", str(W))
    name, own_args, fields, pieces, straddlers, tail = PLAIN[mode]
    sep = b"\r\n" if mode == "rs" else b"\n"
    r = random.Random(len(mode))
    data, border = bytearray(), W
    for i in range(1500):
        if len(data) >= border - 100:                                               # (a record is at most 78 bytes)
            piece, k = straddlers[(border // W - 1) % len(straddlers)]
            data += b"c" * (border - len(data) - k) + piece
            assert data[border - k:border - k + len(piece)] == piece
            data += b"" if piece.endswith(sep) else b"ab" + sep
            border += W
        data += b"".join(r.choice(pieces) for _ in range(r.randrange(0, 16))) + (b"1" if i % 9 == 4 else b"") + sep
    data = bytes(data) + tail
    assert border > 3 * W
    (tmp_path / "in.dat").write_bytes(data)
    prog = Program(blob_of(WHOLE))

    def call(name, args):
        st = host.KxRecordsStats()
        with open(tmp_path / "in.dat", "rb") as fi, open(tmp_path / "out.dat", "wb") as fo, open(tmp_path / "err.dat", "wb") as fe:
            rc = getattr(prog._lib, name)(prog._h, fi.fileno(), fo.fileno(), *args, fe.fileno(), ctypes.byref(st))
        counts = {k: getattr(st, k) for k in ("records", "records_rejected", "windows", "in_bytes", "out_bytes", "longest_record")}
        return rc, (tmp_path / "out.dat").read_bytes(), (tmp_path / "err.dat").read_bytes(), counts

    own = call(name, own_args)
    o = host.KxRecordsOpts(size=ctypes.sizeof(host.KxRecordsOpts), chomp=0, ors_len=0, **fields)
    o.rs[:2] = b"\r\n"                                                              # (read in KX_RECORDS_RS only)
    opts = call("kx_run_records_fd_opts", (ctypes.byref(o),))
    for what, a, b in zip(("return code", "output", "report", "counts"), own, opts):
        assert a == b, (mode, what, a[:200] if isinstance(a, bytes) else a, b[:200] if isinstance(b, bytes) else b)
    rc, out, err, counts = own
    model = MODES[mode][1] if mode != "byte" else (lambda d: host.split_records_model(d, b"\n"))
    assert rc == 1 and counts["records"] == len(model(data)) - 1 and counts["in_bytes"] == len(data) and counts["windows"] > 3
    assert 90 <= counts["records_rejected"] == err.count(b"\n") < counts["records"] // 2 and len(out) == counts["out_bytes"] > len(data) // 2
