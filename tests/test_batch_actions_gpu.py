"""GPU: the batch replay of register-action stages (kx_config::batch_actions = 2; k_bact_measure / k_bact_lanes / k_bact_waves).
Every document's expected result is the CPU oracle run on that document alone (output bytes, or OracleMatchError.pos / .stage);
every case also runs with batch_actions = 1 (the single-document route) and must give identical arrays."""
import ctypes
import json
import os
import random
import subprocess
import time

import pytest
from conftest import GOLDEN, blob_of

from kleenexlang_amd import build, host
from kleenexlang_amd.host import Program
from oracle import oracle

pytestmark = pytest.mark.gpu

KEXC = os.path.join(build.OUT, "kexc")
# (the sources of tests/test_register_actions.py)
SWAP = 'main := (a@/[a-z]*/ ~/,/ b@/[0-9]*/ !b "," !a /\\n/)*\n'
ACCUMULATE = 'main := [acc <- ""] (word)* "=" !acc\nword := w@/[a-z]+/ [acc += w "+"] ~/ /\n'
NESTED = 'main := o@(i@/a*/ "<" !i ">" /b*/) !o "|" !o "|" !i\n'
BYTE_FF = 'main := (r@/[^\\n]*/ "\\xff" !r ~/\\n/ "\\n")*\n'
TWO_STAGE = 'start: rev >> up\nrev := (a@/[a-z]/ b@/[a-z]/ !b !a)*\nup := (~/a/ "A" | /[b-z]/)*\n'
ACTIONBUG = next(t for t in json.load(open(os.path.join(GOLDEN, "action_vectors.json")))["line_tests"] if t["name"] == "actionbug")
COLS = 'main := (a@f ~/,/ b@f ~/,/ c@f ~/\\n/ !c "," !a "," !b "\\n")*\nf := /[^,\\n]*/\n'
KEEP = 'main := a@/[a-z]*/ ~/,/ /[0-9]*/ ~/\\n/\n'
TEN = "main := (" + " ~/,/ ".join("r%d@f" % i for i in range(10)) + " ~/\\n/ " + ' "," '.join("!r%d" % i for i in reversed(range(10))) + \
      ' "\\n")*\nf := /[^,\\n]*/\n'
LOW, REV, UP = 'low := (~/A/ "a" | /[a-z]/)*\n', 'rev := (a@/[a-z]/ b@/[a-z]/ !b !a)*\n', 'up := (~/a/ "A" | /[b-z]/)*\n'
THREE = "start: low >> rev >> up\n" + LOW + REV + UP
QUOTED = 'main := (a@f ~/,/ b@f ~/\\n/ !b "," !a "\\n")*\nf := /"([^"]|"")*"/ | /[^,"\\n]*/\n'
# The route's cost per document of an action stage on the parent commit: profiles/batch_actions_bench.py's route case
# (2 000 swap_fields lines) run on the parent commit, 390.7 ms per call: DESIGN.md §5n and the "parent commit" rows of
# profiles/batch_actions_bench.json (§5j had recorded 0.34-0.37 ms for the same path on another box).
PARENT_ROUTE_MS_PER_DOC = 0.195


def _want(blob, doc, cache={}):
    k = (blob, doc)
    if k not in cache:
        try:
            cache[k] = oracle.run(blob, doc)
        except oracle.OracleMatchError as e:
            cache[k] = (e.pos, e.stage)
    return cache[k]


def _arrays(prog, docs, lead=0):
    """run_batch_tensor on the packed documents, the values starting `lead` bytes into the buffer (off[0] = lead)."""
    import torch
    values, offs = host.pack_batch(docs)
    v = torch.frombuffer(bytearray(b"\x01" * lead + values + b"\0"), dtype=torch.uint8).cuda()[:lead + len(values)]
    o = torch.tensor([x + lead for x in offs], dtype=torch.int64).cuda()
    out, ooff, status, fpos, fstage = prog.run_batch_tensor(v, o)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes(), ooff.tolist(), status.tolist(), fpos.tolist(), fstage.tolist()


def _check_arrays(blob, docs, arrays):
    ob, ooff, status, fpos, fstage = arrays
    pos = accepted = 0
    for i, d in enumerate(docs):
        w = _want(blob, d)
        assert ooff[i] == pos, i
        if isinstance(w, tuple):
            assert (status[i], fpos[i], fstage[i]) == (1, w[0], w[1]), (i, d[:60], w, status[i], fpos[i], fstage[i])
        else:
            assert status[i] == 0 and ob[ooff[i]:ooff[i + 1]] == w, (i, d[:60], ob[ooff[i]:ooff[i + 1]][:80], w[:80])
            pos += len(w)
            accepted += 1
    assert ooff[len(docs)] == pos == len(ob)
    return accepted


def _both_ways(src_or_blob, docs, lead=0, replayed=None, routed=0, env=None, **fields):
    """The replay against the oracle, its counts, and the route with identical arrays."""
    blob = src_or_blob if isinstance(src_or_blob, bytes) else blob_of(src_or_blob)
    prog = Program(blob, config=host.config_from_env(env or {}, batch_actions=2, **fields))
    got = _arrays(prog, docs, lead)
    _check_arrays(blob, docs, got)
    st = prog.last_batch_stats
    assert st.docs_routed == routed, (st.docs_routed, routed)
    if replayed is not None:
        assert st.docs_replayed == replayed, (st.docs_replayed, replayed)
    route = Program(blob, config=host.config_from_env(env or {}, batch_actions=1, **fields))
    assert _arrays(route, docs, lead) == got
    assert route.last_batch_stats.docs_replayed == 0
    return prog


def _accepted_at(blob, docs, stage):
    """documents that reach the end of `stage` (are not rejected at or before it)"""
    n = 0
    for d in docs:
        w = _want(blob, d)
        n += not isinstance(w, tuple) or w[1] > stage
    return n


def _swap_line(r):
    return b"%s,%d\n" % (bytes(r.choice(b"abcdefgh") for _ in range(r.randrange(1, 9))), r.randrange(10 ** 6))


def _case_docs(name, r):
    if name == "swap_fields":
        docs = [b"".join(_swap_line(r) for _ in range(r.randrange(0, 4))) for _ in range(300)] + [b"", b"abc\n", b"ab,12\n", b"x,\n,99\n", b"q,1"]
    elif name == "accumulate":
        docs = [b"".join(bytes(r.choice(b"abc") for _ in range(r.randrange(1, 12))) + b" " for _ in range(r.randrange(0, 9))) for _ in range(300)]
        docs += [b"", b"ab", b"ab  ", b"ab cd efg "]
    elif name == "nested":
        docs = [b"a" * r.randrange(0, 20) + b"b" * r.randrange(0, 20) for _ in range(300)] + [b"", b"aab", b"bbb", b"aaaa", b"aba", b"c"]
    elif name == "byte_ff":
        docs = [b"".join(bytes(r.choice(b"ab\xff\xfe") for _ in range(r.randrange(0, 30))) + b"\n" for _ in range(r.randrange(0, 3))) for _ in range(300)]
        docs += [b"", b"\xff\n", b"\xff\xff\xff\xff\n", b"\xff" * 50 + b"\n", b"\xff", bytes(r.randrange(11, 256) for _ in range(300)) + b"\n"]
    elif name == "two_stage":
        docs = [bytes(r.choice(b"abcxyz") for _ in range(r.randrange(0, 40))) for _ in range(300)] + [b"", b"ab", b"abcd", b"abc", b"zaqa", b"a1"]
    else:
        docs = [(s + "\n").encode() for s in ACTIONBUG["in"]] * 300 + [b"", b"cc\n"]
    r.shuffle(docs)
    return docs


SOURCES = {"swap_fields": SWAP, "accumulate": ACCUMULATE, "nested": NESTED, "byte_ff": BYTE_FF, "two_stage": TWO_STAGE,
           "actionbug": ACTIONBUG["program"]}


@pytest.mark.parametrize("name", sorted(SOURCES))
def test_action_programs_replayed_in_the_batch(name):
    blob = blob_of(SOURCES[name])
    docs = _case_docs(name, random.Random(len(name)))
    info = [Program(blob).stage_has_actions(s) for s in range(Program(blob).num_stages)]
    want_replayed = sum(_accepted_at(blob, docs, s) for s, a in enumerate(info) if a)
    assert want_replayed > 100
    for lead in range(16):      # the values start at every alignment 0..15 (off[0] != 0)
        if lead in (0, 5):
            _both_ways(blob, docs, lead, replayed=want_replayed)
        else:
            prog = Program(blob, config=host.config_from_env({}, batch_actions=2))
            _check_arrays(blob, docs, _arrays(prog, docs, lead))
            assert (prog.last_batch_stats.docs_routed, prog.last_batch_stats.docs_replayed) == (0, want_replayed)


def test_the_issues_programs_compute_what_the_issue_states():
    for src, doc, want in ((COLS, b"x,\xff\xff,zz\n", b"zz,x,\xff\xff\n"), (KEEP, b"ab,1\n", b"1"), (TEN, b"0,1,2,3,4,5,6,7,8,9\n", b"9,8,7,6,5,4,3,2,1,0\n"),
                           (THREE, b"AbcA", b"bAAc"), (NESTED, b"aab", b"<aa>b||"), (TWO_STAGE, b"abcd", b"bAdc")):
        assert _want(blob_of(src), doc) == want, (src, doc)
    assert _want(blob_of(COLS), b"a,b\n") == (3, 0)
    assert _want(blob_of(THREE), b"ab1") == (2, 0) and _want(blob_of(THREE), b"abc") == (3, 1)
    assert _want(blob_of(TWO_STAGE), b"abc")[0] == 3
    keep = [b"ab,1\n", b",\n", b"zz,77\n", b"ab,1", b""] * 40
    _both_ways(KEEP, keep, replayed=_accepted_at(blob_of(KEEP), keep, 0))


@pytest.mark.parametrize("big", [False, True])
def test_lane_wave_and_route_in_one_batch(big):
    """cols: three registers → lanes; ten: ten registers → waves; one document above batch_doc_max → the route."""
    env = {"KX_FORCE_BIG": "1"} if big else {}
    r = random.Random(3)
    field = lambda: bytes(r.choice(b"abc\xff xyz") for _ in range(r.randrange(0, 12)))   # noqa: E731
    cols = [b",".join(field() for _ in range(3)) + b"\n" for _ in range(400)] + [b"a,b\n", b""]
    long_doc = b"".join(cols[:300])
    assert len(long_doc) > 2048
    prog = _both_ways(COLS, cols + [long_doc], replayed=len(cols) - 1, routed=1, env=env, batch_doc_max=2048)
    assert prog.last_batch_stats.docs_rejected == 1
    ten = [b",".join(field() for _ in range(10)) + b"\n" for _ in range(400)] + [b"1,2,3\n", b""]
    ten += [b",".join(bytes(r.choice(b"pq") for _ in range(r.randrange(100, 600))) for _ in range(10)) + b"\n" for _ in range(8)]   # fields beyond the LDS mirrors
    long_ten = b"".join(ten[:200])
    assert len(long_ten) > 8192
    _both_ways(TEN, ten + [long_ten], replayed=len(ten) - 1, routed=1, env=env, batch_doc_max=8192)
    # long fields in few registers: lanes whose frames and registers live in the arenas; and the same by waves (act_lanes = 1)
    wide = [b",".join(bytes(r.choice(b"mn\xff") for _ in range(r.randrange(0, 300))) for _ in range(3)) + b"\n" for _ in range(200)]
    _both_ways(COLS, wide, replayed=len(wide), env=env)
    _both_ways(COLS, wide, replayed=len(wide), env=env, act_lanes=1)
    _both_ways(COLS, wide, replayed=len(wide), env=env, act_lanes=2)


@pytest.mark.parametrize("order", ["low rev up", "rev low up", "low up rev"])
def test_action_stage_first_in_the_middle_and_last(order):
    """`three`, its stages permuted: the action stage (rev) in every position; rejections at each stage."""
    parts = {"low": LOW, "rev": REV, "up": UP}
    names = order.split()
    src = "start: " + " >> ".join(names) + "\n" + "".join(parts[n] for n in names)
    blob = blob_of(src)
    r = random.Random(9)
    docs = [bytes(r.choice(b"AabcxyzA") for _ in range(2 * r.randrange(0, 20))) for _ in range(300)]
    docs += [b"AbcA", b"ab1", b"abc", b"", b"1", b"abA", b"aaa", b"Aa"] * 3
    stages = {_want(blob, d)[1] for d in docs if isinstance(_want(blob, d), tuple)}
    act = names.index("rev")
    assert stages and (act in stages or order != "low rev up"), stages      # (only behind `low` can `rev` meet an odd length)
    # a document rejected before the action stage (or by its transducer) is not replayed
    _both_ways(blob, docs, lead=3, replayed=_accepted_at(blob, docs, act))


def test_size_query_exact_capacity_and_one_byte_short():
    import torch
    blob = blob_of(SWAP)
    r = random.Random(2)
    docs = [_swap_line(r) for _ in range(500)] + [b"abc\n"]
    values, offs = host.pack_batch(docs)
    prog = Program(blob, config=host.config_from_env({}, batch_actions=2))
    v = torch.frombuffer(bytearray(values), dtype=torch.uint8).cuda()
    o = torch.tensor(offs, dtype=torch.int64).cuda()
    ooff = torch.empty(len(docs) + 1, dtype=torch.int64, device="cuda")
    recs = torch.empty((len(docs), 2), dtype=torch.int64, device="cuda")
    want = b"".join(oracle.run(blob, d) for d in docs[:-1])

    def call(buf, cap):
        ol = ctypes.c_size_t()
        st = host.KxBatchStats()
        rc = prog._lib.kx_run_batch(prog._h, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(o.data_ptr()), len(docs),
                                    ctypes.c_void_p(buf), cap, ctypes.c_void_p(ooff.data_ptr()), ctypes.c_void_p(recs.data_ptr()),
                                    ctypes.byref(ol), ctypes.byref(st), None)
        return rc, ol.value
    assert call(None, 0) == (-3, len(want))          # the REPLAYED total, not the token streams'
    assert ooff[-1].item() == len(want)
    out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    assert call(out.data_ptr(), len(want) - 1) == (-3, len(want))
    assert call(out.data_ptr(), len(want)) == (1, len(want))     # (1: the rejected document)
    assert out.cpu().numpy().tobytes() == want


def _time_batch(prog, docs, repeats=5, warmup=2):
    """median milliseconds of run_batch_tensor (HIP events), and the arrays of the last call"""
    import torch
    values, offs = host.pack_batch(docs)
    v = torch.frombuffer(bytearray(values), dtype=torch.uint8).cuda()
    o = torch.tensor(offs, dtype=torch.int64).cuda()
    ms = []
    for k in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = prog.run_batch_tensor(v, o)
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], res


def test_a_million_lines_in_one_call_and_the_speed_up_over_the_route():
    """2^20 swap_fields lines, all bytes compared; on 2^16 of them the replay must be at least 100x cheaper per document than
    the route was on the parent commit (PARENT_ROUTE_MS_PER_DOC).  Figures of the development run (MI355X): see DESIGN.md §5n."""
    blob = blob_of(SWAP)
    r = random.Random(5)
    pool = [_swap_line(r) for _ in range(20000)]
    want = {d: oracle.run(blob, d) for d in set(pool)}
    docs = [pool[r.randrange(len(pool))] for _ in range(1 << 20)]
    prog = Program(blob, config=host.config_from_env({}, batch_actions=2))
    ms20, (out, ooff, status, _, _) = _time_batch(prog, docs, repeats=1, warmup=1)
    assert (prog.last_batch_stats.docs_routed, prog.last_batch_stats.docs_replayed) == (0, len(docs))
    assert int(status.sum().item()) == 0
    assert out.cpu().numpy().tobytes() == b"".join(want[d] for d in docs)
    assert ooff[-1].item() == sum(len(want[d]) for d in docs)
    small = docs[:1 << 16]
    ms16, _ = _time_batch(prog, small)
    replay_ms_per_doc = ms16 / len(small)
    route = Program(blob, config=host.config_from_env({}, batch_actions=1))
    t0 = time.perf_counter()
    got = route.run_batch(docs[:500])
    route_ms_per_doc = (time.perf_counter() - t0) * 1e3 / 500
    assert got == [want[d] for d in docs[:500]]
    print("\nbatch replay: 2^20 documents in %.2f ms; 2^16 documents in %.3f ms = %.3f us per document; parent route %.0f us per document "
          "(recorded); this process's route %.0f us per document (cross-check); ratio to the recorded figure %.0fx"
          % (ms20, ms16, replay_ms_per_doc * 1e3, PARENT_ROUTE_MS_PER_DOC * 1e3, route_ms_per_doc * 1e3, PARENT_ROUTE_MS_PER_DOC / replay_ms_per_doc))
    assert replay_ms_per_doc * 100 <= PARENT_ROUTE_MS_PER_DOC


# ------------------------------------------------------------------------------------------------------------ record mode
def _want_records(blob, data, offs):
    out, err = [], []
    for i in range(len(offs) - 1):
        w = _want(blob, data[offs[i]:offs[i + 1]])
        if isinstance(w, tuple):
            err.append("Match error at input symbol %d in record %d!\n" % (w[0], i + 1))
        else:
            out.append(w)
    return b"".join(out), "".join(err).encode()


def _bin(tmp_path, src):
    p = tmp_path / "p.kex"
    p.write_text(src)
    exe = tmp_path / "bin"
    r = subprocess.run([KEXC, "compile", "--quiet", str(p), "--out", str(exe)], stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run_bin(exe, data, args=("--records",), **env):
    return subprocess.run(["timeout", "-k", "10", "600", exe, *args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env), timeout=660)


def test_record_mode_replays_action_programs(tmp_path):
    blob = blob_of(SWAP)
    exe = _bin(tmp_path, SWAP)
    r = random.Random(8)
    lines = [_swap_line(r) for _ in range(200000)]
    for k in (7, 100003, 199999):
        lines[k] = b"abc\n"           # three rejected lines
    data = b"".join(lines)
    offs = host.split_records_model(data, b"\n")
    out, err = _want_records(blob, data, offs)
    assert err.count(b"\n") == 3
    for env in ({}, {"KX_WINDOW_BYTES": "4096"}):      # whole, and with records straddling 4 KiB windows
        res = _run_bin(exe, data, **env)
        assert res.returncode == 1 and res.stderr == err, (res.returncode, res.stderr[:300])
        assert res.stdout == out, (len(res.stdout), len(out))
    # the library call: nothing routed; with the route asked for, the same bytes and every record routed
    prog = Program(blob)
    f = tmp_path / "in.dat"
    f.write_bytes(data)
    with open(f, "rb") as fi, open(tmp_path / "out.dat", "wb") as fo:
        st = prog.run_records_fd(fi.fileno(), fo.fileno())
    assert (tmp_path / "out.dat").read_bytes() == out
    assert st["records"] == len(lines) and st["records_routed"] == 0 and st["records_rejected"] == 3 and st["rejected"]
    assert prog._cfg.batch_actions == 0                 # (set for the call, restored)
    small = b"".join(lines[:500])
    sout, serr = _want_records(blob, small, host.split_records_model(small, b"\n"))
    res = _run_bin(exe, small, KX_BATCH_ACTIONS="0")
    assert (res.returncode, res.stdout, res.stderr) == (1, sout, serr)
    f.write_bytes(small)
    with open(f, "rb") as fi, open(tmp_path / "out.dat", "wb") as fo:
        st = prog.run_records_fd(fi.fileno(), fo.fileno(), batch_actions=False)
    assert (tmp_path / "out.dat").read_bytes() == sout and st["records_routed"] == 500
    norm = lambda res: [x if isinstance(x, bytes) else (x.pos, x.stage) for x in res]   # noqa: E731
    assert norm(prog.run_records(small)) == norm(prog.run_records(small, batch_actions=False))
    # --records --quote with an action program: the splits compose with the replay
    qblob = blob_of(QUOTED)
    qexe = _bin(tmp_path, QUOTED)
    qdata = b'"a,\nb",c\n' + b'x,"y""z"\n' * 50 + b'"a,\nb",c\n' + b'bad"\n' + b"p,q\n"
    assert _want(qblob, b'"a,\nb",c\n') == b'c,"a,\nb"\n'
    res = _run_bin(qexe, qdata, args=("--records", "--quote"))
    got = Program(qblob).run_records(qdata, quote=b'"')
    exp = [_want(qblob, rec) for rec in _quoted_records(qdata)]
    assert len(got) == len(exp) == 53 and sum(isinstance(e, tuple) for e in exp) == 1
    assert [g if isinstance(g, bytes) else (g.pos, g.stage) for g in got] == exp
    assert res.stdout == b"".join(e for e in exp if isinstance(e, bytes))
    assert res.returncode == (1 if any(isinstance(e, tuple) for e in exp) else 0)


def _quoted_records(data, sep=0x0A, quote=0x22):
    """records of `data` where a separator inside quotes ends no record (the parity rule of kx_split_records_quoted)"""
    recs, start, inq = [], 0, False
    for i, b in enumerate(data):
        if b == quote:
            inq = not inq
        elif b == sep and not inq:
            recs.append(data[start:i + 1])
            start = i + 1
    if start < len(data):
        recs.append(data[start:])
    return recs


def test_a_replayed_batch_leaves_the_delayed_form_as_it_found_it():
    blob = blob_of(THREE)
    prog = Program(blob, config=host.config_from_env({}, batch_actions=2))
    form = [prog.stage_delayed_form(s) for s in range(prog.num_stages)]
    docs = [b"AbcA", b"ab1", b"abc", b"xyzw"] * 200
    _check_arrays(blob, docs, _arrays(prog, docs))
    assert prog.last_batch_stats.docs_replayed == _accepted_at(blob, docs, 1)
    assert [prog.stage_delayed_form(s) for s in range(prog.num_stages)] == form
