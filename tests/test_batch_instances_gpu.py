"""GPU: every instance of the batch kernels (k_bforward, k_bback, k_bemit, k_bemit_fr: WIDE or not, framed or not) on every table layout
chooseLayout can give a stage, against the CPU oracle run on each document alone — output bytes and output offsets, or (status,
fail_pos, fail_stage).  Nothing is compared with another run of the engine, except where that IS the claim (part b).

The batch kernels print no line of their own.  Which instance ran follows from kx_stage_describe_cfg under the configuration the
Program was loaded with and from runBatch's two conditions (test_batch_instances.batch_instances); the layout flags of every case and
the populations of its documents are asserted in test_batch_instances.py, which needs no GPU.

  a. the matrix: every case under four frames at three leads, and once more with batch_doc_max = 100 (the route)   test_matrix
  b. framed and unframed runs of the same accepted bodies agree: k_bemit_fr against k_bemit, <…, BFrame> against <…>     test_framed_and_unframed_agree
  c. randprog.program_wide as batches, unframed and framed                                                            test_generated_wide_*
  d. the second trip of the grid-stride loops on a wide framed and a wide unframed run; the scan's group edges       test_second_trip, test_scan_group_edges
  e. the last document's last granule is the buffer's last                                                          test_buffer_ends

Counts, as the tests print them on an MI355X (256 CUs); every figure but `routed` is the oracle's, and the engine's own
kx_batch_stats (docs_rejected, docs_routed, out_bytes) are asserted equal to them in every run.  Per matrix case, over its 14 runs:
  plain_direct, plain_nodirect, inline_pinned, big_plain_direct   1 946 documents, 1 005 accepted, 941 rejected, 86 routed
  job_stride                                                      1 666, 879, 787, 76
  leaves_js1, leaves_js2                                          910, 501, 409, 72 (batch_doc_max = 48)
  inline, wide_entries, classes, big_wide_entries, big_classes    1 372, 837, 535, 76
  xlat, tblmode, big_xlat                                         1 540, 879, 661, 76
  two_stage_wide_last / two_stage_wide_first                      1 372, 837, 255 rejected at stage 0 and 280 at stage 1, 132 / 186 routed
  c. generated programs: 31 programs (9 of them once more with KX_FORCE_BIG), none refused; 17 866 documents, 14 380 accepted, 3 486
     rejected at stage 0, none at stage 1 (`tidy` takes every byte), none routed; 10 runs with a general first stage, 9 with a general second
  d. 525 313 documents: classes framed 393 903 accepted, 131 410 rejected, 6.0 MB of output; wide_entries 359 841, 165 472, 22.7 MB
The table of instances and the cases that cover each is in DESIGN.md §3b.  No mismatch was found."""
import pytest
import test_batch_instances as tb
import test_random_inputs as tr
from conftest import blob_of
from test_random_inputs_gpu import batch_docs, load
from test_records_chomp_gpu import _check, _expected, _run

from kleenexlang_amd import host
from kleenexlang_amd.host import Program

pytestmark = pytest.mark.gpu


def _tally(want, nstages):
    """(documents, accepted, rejected per stage) of an expectation of test_records_chomp_gpu._expected"""
    status, fstage = want[2], want[4]
    return len(status), status.count(0), [sum(1 for s, f in zip(status, fstage) if s and f == st) for st in range(nstages)]


def _instances(name, trim):
    """what runBatch launches for the case's stages in a call with this trim"""
    out = set()
    for st in range(len(tb.CASE[name].wide)):
        out |= set(tb.batch_instances(tb.describe(name, st), st, trim))
    return out


# --------------------------------------------------------------------------------------------------------------- a. the matrix
@pytest.mark.parametrize("name", tb.NAMES)
def test_matrix(name):
    """Bodies of every length in LENGTHS the language has (three of each, empty ones side by side), rejected variants of every
    fourth (a refused byte at 0, 31 / 32, 63 / 64 and the last byte; a cut before the end), under no frame, trim = 1, trim = 8 with the
    last range whole and an 8-byte suffix, and a 3-byte suffix alone — at leads 1, 7 and 16.  No document takes the route.  Then
    batch_doc_max = 100 under the first two frames: exactly the documents above 100 bytes that no earlier stage rejected take
    batchRouteOne, through the unaligned copy and with the trimmed length (LEAVES_PROGRAM's documents end at 65 bytes: 48 there)."""
    c, bl = tb.CASE[name], tb.blob(name)
    ns = len(c.wide)
    docs = list(tb.bodies_of(name))
    prog = Program(bl, config=tb.config(name))
    assert prog.num_stages == ns
    starts, seen, runs = set(), set(), 0
    tot = {"docs": 0, "accepted": 0, "rejected": [0] * ns, "routed": 0}
    try:
        for trim, last_whole, suffix in tb.FRAMES:
            data, offs = tb.pack(name, docs, trim)
            seen |= _instances(name, trim)
            for lead in tb.LEADS:
                want = _check(prog, bl, data, offs, lead=lead, trim=trim, last_whole=last_whole, suffix=suffix)
                n, acc, rej = _tally(want, ns)
                st = prog.last_batch_stats
                assert (st.docs, st.docs_routed, st.docs_rejected, st.out_bytes) == (len(docs), 0, sum(rej), len(want[0])), (name, trim, lead)
                starts |= {(o + lead) % 16 for o in offs[:-1]}
                tot["docs"] += n
                tot["accepted"] += acc
                tot["rejected"] = [a + b for a, b in zip(tot["rejected"], rej)]
                runs += 1
                assert 2 * acc >= n and sum(rej) >= 10, (name, acc, n)
    finally:
        prog.close()
    assert starts == set(range(16)) and runs == 12
    expected = {k for st, wide in enumerate(c.wide) for t in (0, 1) for k in tb.instance_names(wide, st == 0 and t)}
    assert seen == expected, (name, sorted(seen))
    # the route
    route = Program(bl, config=tb.config(name, batch_doc_max=tb.route_max(name)))
    try:
        expect_routed = tb.routed_expected(name, docs, tb.route_max(name))
        assert expect_routed >= 6, (name, expect_routed)
        for trim, last_whole, suffix in tb.FRAMES[:2]:
            data, offs = tb.pack(name, docs, trim)
            want = _check(route, bl, data, offs, lead=7, trim=trim, last_whole=last_whole, suffix=suffix)
            n, acc, rej = _tally(want, ns)
            st = route.last_batch_stats
            assert (st.docs_routed, st.docs_rejected) == (expect_routed, sum(rej)), (name, trim, st.docs_routed, expect_routed)
            tot["docs"] += n
            tot["accepted"] += acc
            tot["rejected"] = [a + b for a, b in zip(tot["rejected"], rej)]
            tot["routed"] += st.docs_routed
    finally:
        route.close()
    print("batch matrix", name, tot, "instances", sorted(seen))


# ------------------------------------------------------------------------------------------- b. framed and unframed agree
@pytest.mark.parametrize("name", tb.NAMES)
def test_framed_and_unframed_agree(name):
    """The case's accepted bodies packed as they are, and followed by two bytes the grammar refuses with trim = 2: the same output,
    offsets and records (and the oracle's).  Stage 0 runs k_bforward / k_bback / k_bemit in the first call and their <…, BFrame>
    twins (k_bemit_fr, the hand-kept copy of k_bemit) in the second."""
    bl = tb.blob(name)
    acc = list(tb.accepted_bodies(name))
    prog = Program(bl, config=tb.config(name))
    try:
        data, offs = tb.pack(name, acc, 0)
        want = _check(prog, bl, data, offs, lead=5)
        plain = _run(prog, data, offs, 5)
        data2, offs2 = tb.pack(name, acc, 2)
        framed = _run(prog, data2, offs2, 5, trim=2)
    finally:
        prog.close()
    assert want[2].count(0) == len(acc) and len(want[0]) > 0
    for what, a, b in zip(("output", "output offsets", "status", "fail_pos", "fail_stage"), plain, framed):
        assert a == b, (name, what)
    assert plain[0] == want[0] and plain[1] == want[1]
    assert _instances(name, 2) != _instances(name, 0)


# --------------------------------------------------------------------------------------- c. generated wide programs as batches
_WIDE = {}


def wide_part(part):
    """-> {"programs", "refused", "no_source", "docs", "accepted", "rejected": per stage, "general_first", "general_second", "forced_big"}"""
    if part in _WIDE:
        return _WIDE[part]
    c = {"programs": 0, "refused": 0, "no_source": 0, "docs": 0, "accepted": 0, "rejected": [0, 0], "general_first": 0, "general_second": 0,
         "forced_big": 0}
    for seed in tb.WIDE_SEEDS[part::tb.WIDE_PARTS]:
        src = tr.source("wide", seed)
        if src is None:
            c["no_source"] += 1
            continue
        bl = blob_of(src, 3)
        docs = batch_docs("wide", seed)
        two = src.startswith("start:")
        for fields in ({},) + (({"force": host.KX_FORCE_BIG},) if two else ()):      # (test_batch_instances.py: why KX_FORCE_BIG)
            p = load(src, **fields)
            if p is None:
                c["refused"] += 1
                break
            try:
                for trim, suffix in ((0, b""), (2, b"|")):
                    data, offs = host.pack_batch([d + b"\xfe\n"[:trim] for d in docs])
                    want = _check(p, bl, data, offs, lead=3, trim=trim, suffix=suffix)
                    n, acc, rej = _tally(want, 2)
                    assert 2 * acc > n, (seed, src, acc, n)
                    assert (p.last_batch_stats.docs_routed, p.last_batch_stats.docs_rejected) == (0, sum(rej))
                    c["docs"] += n
                    c["accepted"] += acc
                    c["rejected"] = [a + b for a, b in zip(c["rejected"], rej)]
                general = tb.wide_generals(seed, **fields)
                assert len(general) == p.num_stages
                c["general_first"] += general[0]
                c["general_second"] += two and general[1]
                c["forced_big"] += bool(fields)
                c["programs"] += not fields
            finally:
                p.close()
    _WIDE[part] = c
    return c


@pytest.mark.parametrize("part", range(tb.WIDE_PARTS))
def test_generated_wide_programs_as_batches(part):
    """randprog.program_wide (two-stage pipelines, more than 31 byte classes, bytes from 0x80 on, constants of up to 40 bytes) on the
    documents of test_random_inputs_gpu.batch_docs — accepted samples of 0 to 700 bytes and their rejected variants — unframed and
    with trim = 2 (two junk bytes behind every document) and the suffix `|`.  A later stage reads its offsets from the workspace and
    skips the documents the stage before it rejected.  The two-stage programs run once more with KX_FORCE_BIG: both stages general."""
    c = wide_part(part)
    assert c["programs"] >= 5, c


def test_generated_wide_populations():
    tot = None
    for part in range(tb.WIDE_PARTS):
        c = wide_part(part)
        tot = dict(c) if tot is None else {k: ([a + b for a, b in zip(tot[k], v)] if isinstance(v, list) else tot[k] + v) for k, v in c.items()}
    print("batch wide programs", tot)
    allowed = (tr.NPROG - tr.MEASURED["wide"]["usable"]) * len(tb.WIDE_SEEDS) // tr.NPROG
    assert tot["refused"] + tot["no_source"] <= allowed, tot
    assert tot["general_first"] >= 1 and tot["general_second"] >= 1, tot
    assert tot["rejected"][0] > 0, tot


# ------------------------------------------------------------------------------------- d. the grid-stride loops' second trip
def _pool_run(name, ndocs, trim, suffix):
    import numpy as np
    import torch
    bl = tb.blob(name)
    data, off, out, ooff, status, fpos = tb.pool_arrays(name, ndocs, trim, tb.CASE[name].junk, suffix)
    prog = Program(bl, config=tb.config(name))
    try:
        v = torch.frombuffer(bytearray(data + b"\n"), dtype=torch.uint8).cuda()[:len(data)]
        got = prog.run_batch_tensor(v, torch.from_numpy(off).cuda(), trim=trim, suffix=suffix)
        torch.cuda.synchronize()
        st = prog.last_batch_stats
        g_out, g_ooff, g_status, g_fpos, g_fstage = (t.cpu().numpy() for t in got)
    finally:
        prog.close()
    assert np.array_equal(g_ooff, ooff), (name, ndocs, int(np.argmax(g_ooff != ooff)))
    assert np.array_equal(g_status, status), (name, ndocs, int(np.argmax(g_status != status)))
    assert np.array_equal(g_fpos, fpos) and not g_fstage.any(), (name, ndocs)
    want_out = np.frombuffer(out, dtype=np.uint8)
    assert g_out.size == want_out.size and np.array_equal(g_out, want_out), (name, ndocs, int(np.argmax(g_out != want_out)))
    assert (st.docs, st.docs_routed, st.docs_rejected, st.out_bytes) == (ndocs, 0, int(status.sum()), len(out))
    return {"docs": ndocs, "accepted": int((status == 0).sum()), "rejected": int(status.sum()), "routed": 0, "out_bytes": len(out)}


@pytest.mark.parametrize("name,trim,suffix", [("classes", 1, b"\n"), ("wide_entries", 0, b"")])
def test_second_trip(name, trim, suffix):
    """ndocs = CUs * 4 * 512 + 1025: document i >= CUs * 4 * 512 is a lane's second trip in k_bforward, k_bback and k_binit, and
    the piece slots beyond that are k_bemit's / k_bemit_fr's — on <true, BFrame> instances (more than 64 byte classes, trim = 1 and a
    suffix) and on the unframed wide ones (constants of 300 and 130 bytes).  Documents of 0 to 5 bytes from a pool of 40."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    ndocs = tb.second_trip_docs(ncu)
    c = _pool_run(name, ndocs, trim, suffix)
    assert ndocs > ncu * 4 * 512 + 1024 and c["out_bytes"] < 64 << 20
    print("batch second trip", name, "CUs", ncu, c)


def test_scan_group_edges():
    """k_bscan_reduce / k_bscan_down work in groups of 1 024 documents (ooff[ndocs] is one entry more): 1 023, 1 024, 1 025 and 2 049
    documents on a wide case, framed"""
    for ndocs in tb.SCAN_EDGES:
        c = _pool_run("classes", ndocs, 1, b"\n")
        print("batch scan edge", c)


# ----------------------------------------------------------------------------------------------------------- e. buffer ends
@pytest.mark.parametrize("name", sorted(tb.END_CASES))
def test_buffer_ends(name):
    """The values tensor has exactly lead + len(data) bytes: the last document's last 16-byte granule is the tensor's last, and
    bload_piece loads no granule beyond the one that holds a document's last byte.  Last bodies of 1, 16, 17 and 64 bytes starting
    at residue 15, unframed and with trim = 1."""
    import torch
    bl = tb.blob(name)
    prog = Program(bl, config=tb.config(name))
    try:
        for last in tb.END_CASES[name]:
            for trim, suffix in ((0, b""), (1, b"\n")):
                data, offs = tb.end_batch(name, last, trim)
                v = torch.empty(tb.END_LEAD + len(data), dtype=torch.uint8, device="cuda")
                v.copy_(torch.frombuffer(bytearray(b"\n" * tb.END_LEAD + data), dtype=torch.uint8))
                o = torch.tensor([x + tb.END_LEAD for x in offs], dtype=torch.int64).cuda()
                assert (v.data_ptr() + int(o[-2])) % 16 == 15 and int(o[-1]) == v.numel()
                want = _expected(bl, host.chomp_records_model(data, offs, trim, False), suffix)
                out, ooff, status, fpos, fstage = prog.run_batch_tensor(v, o, trim=trim, suffix=suffix)
                torch.cuda.synchronize()
                got = (out.cpu().numpy().tobytes(), ooff.tolist(), status.tolist(), fpos.tolist(), fstage.tolist())
                assert got == tuple(want), (name, last, trim)
                assert want[2] == [0] * (len(offs) - 1)
    finally:
        prog.close()
