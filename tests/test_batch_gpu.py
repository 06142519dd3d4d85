"""GPU: batched runs (kx_run_batch / Program.run_batch_tensor / Program.run_batch).  Every document's result is checked
against the CPU oracle run on that document alone: output bytes, or OracleMatchError.pos / .stage for a rejection."""
import os
import random

import pytest
from conftest import blob_of, dictionary_program

from kleenexlang_amd import host, workloads
from kleenexlang_amd.host import MatchError, Program
from oracle import oracle

pytestmark = pytest.mark.gpu

PROGRAMS = sorted(f[:-4] for f in os.listdir(host.PROGRAM_DIR) if f.endswith(".kex"))
LINE_SHAPE = dict(workloads.PROGRAM_INPUT, add_commas="numbers")


def _want(blob, doc):
    try:
        return oracle.run(blob, doc)
    except oracle.OracleMatchError as e:
        return (e.pos, e.stage)


def _check(blob, docs, got):
    assert len(got) == len(docs)
    for i, (d, g) in enumerate(zip(docs, got)):
        w = _want(blob, d)
        if isinstance(w, tuple):
            assert isinstance(g, MatchError) and (g.pos, g.stage) == w, (i, d[:80], w, g)
        else:
            assert g == w, (i, d[:80], g[:120] if isinstance(g, bytes) else g, w[:120])


def _tensor_check(prog, blob, docs):
    """run_batch_tensor on the packed list: out_offsets exact, ranges of rejected documents empty."""
    import torch
    values, offs = host.pack_batch(docs)
    v = torch.frombuffer(bytearray(values + b"\0"), dtype=torch.uint8).cuda()[:len(values)]
    out, ooff, status, fpos, fstage = prog.run_batch_tensor(v, torch.tensor(offs, dtype=torch.int64).cuda())
    torch.cuda.synchronize()
    ob, ooff, status, fpos, fstage = out.cpu().numpy().tobytes(), ooff.tolist(), status.tolist(), fpos.tolist(), fstage.tolist()
    pos = 0
    for i, d in enumerate(docs):
        w = _want(blob, d)
        assert ooff[i] == pos
        if isinstance(w, tuple):
            assert (status[i], fpos[i], fstage[i]) == (1, w[0], w[1]), i
        else:
            assert status[i] == 0 and ob[ooff[i]:ooff[i + 1]] == w, i
            pos += len(w)
    assert ooff[len(docs)] == pos == len(ob)


def _lines(name, count, seed=3):
    data = workloads.generate(LINE_SHAPE[name], count * 1000, seed=seed)
    docs = [l + b"\n" for l in data.split(b"\n")[:-1]][:count]
    assert len(docs) == count
    return docs


@pytest.mark.parametrize("name", PROGRAMS)
def test_every_program_on_ten_thousand_lines(name):
    blob = blob_of(name)
    if name in LINE_SHAPE:
        docs = _lines(name, 10000)
    else:
        r = random.Random(11)
        docs = [bytes(r.choice(b"ab\nc") for _ in range(r.randint(0, 40))) for _ in range(10000)]
    assert len(docs) >= 10000
    prog = Program(blob)
    _check(blob, docs, prog.run_batch(docs))
    _tensor_check(prog, blob, docs)


def test_lengths_alignments_views_and_sliced_offsets():
    import torch
    blob = blob_of("csv2json")
    base = workloads.generate("csv", 1 << 16, seed=5)
    lens = [0, 1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097]
    docs = []
    for k, n in enumerate(lens):
        docs.append(base[k * 97:k * 97 + n])   # (mostly rejected: a row cut anywhere; prefixes that are whole rows pass)
        cut = base[:n + 200]
        docs.append(cut[:cut.rfind(b"\n") + 1] if b"\n" in cut else b"")
    prog = Program(blob)
    _check(blob, docs, prog.run_batch(docs))
    for align in range(16):   # every start alignment, a view at an odd address, off[0] != 0
        values, offs = host.pack_batch(docs)
        buf = torch.zeros(len(values) + 64, dtype=torch.uint8)
        buf[align + 1:align + 1 + len(values)] = torch.frombuffer(bytearray(values), dtype=torch.uint8)
        dev = buf.cuda()
        view = dev[1:]                                      # odd start address
        o = torch.tensor([x + align for x in offs], dtype=torch.int64).cuda()
        out, ooff, status, fpos, fstage = prog.run_batch_tensor(view, o)
        torch.cuda.synchronize()
        ob, ooff, status, fpos = out.cpu().numpy().tobytes(), ooff.tolist(), status.tolist(), fpos.tolist()
        for i, d in enumerate(docs):
            w = _want(blob, d)
            if isinstance(w, tuple):
                assert status[i] == 1 and fpos[i] == w[0] and ooff[i] == ooff[i + 1]
            else:
                assert ob[ooff[i]:ooff[i + 1]] == w, (align, i)


def test_rejections_leave_their_neighbours_alone():
    blob = blob_of("iso_datetime_to_json")
    good = _lines("iso_datetime_to_json", 300)
    docs = []
    for i, g in enumerate(good):
        docs.append(g)
        if i % 3 == 0:
            docs.append(b"#" + g)                 # first byte
        elif i % 3 == 1:
            docs.append(g[:10] + b"#" + g[10:])   # mid-document
        else:
            docs.append(g[:-3])                   # a non-final end
    got = Program(blob).run_batch(docs)
    _check(blob, docs, got)
    assert sum(isinstance(g, MatchError) for g in got) == 300


def test_random_programs():
    import randprog
    done = 0
    for seed in range(200):
        try:
            blob = blob_of(randprog.program(seed), 0)
        except host.CompileError:      # (beyond the engine's table limits: test_random_programs.py skips those too)
            continue
        if oracle.info(blob)["nstates"] > 2000:
            continue
        docs = randprog.inputs(seed, 60, 150)
        _check(blob, docs, Program(blob).run_batch(docs))
        done += 1
    assert done >= 100, done


def test_pipeline_rejections_at_both_stages():
    blob = host.compile_source('start: a >> b\na := (~/x/ "Q" | /[a-wyz]/)*\nb := /[a-z]*/\n')
    docs = [b"abc", b"axb", b"a1", b"", b"x", b"zzz", b"1x", b"ab" * 100 + b"x"]
    prog = Program(blob)
    got = prog.run_batch(docs)
    _check(blob, docs, got)
    assert [g.stage for g in got if isinstance(g, MatchError)] == [1, 0, 1, 0, 1]
    _tensor_check(prog, blob, docs)


def test_register_actions_and_long_documents_take_the_route():
    import json
    from conftest import GOLDEN
    t = next(t for t in json.load(open(os.path.join(GOLDEN, "action_vectors.json")))["line_tests"] if t["name"] == "actionbug")
    blob = blob_of(t["program"])
    docs = [(s + "\n").encode() for s in t["in"]] * 20 + [b"", b"cc\n"]
    prog = Program(blob)
    _check(blob, docs, prog.run_batch(docs))
    assert prog.last_batch_stats.docs_routed == len(docs)
    blob = blob_of("apache_log")
    lines = _lines("apache_log", 4000)
    docs = lines[:50] + [b"".join(lines[:k]) for k in (2, 3, 5, 9)] + [b"".join(lines)]   # the last > 1 MiB? (grown below)
    while len(docs[-1]) <= (1 << 20):
        docs[-1] += docs[-1]
    docs.append(lines[7][:-1])   # rejected, short
    docs.append(b"".join(lines[:6])[:-2])   # rejected, routed
    prog = Program(blob, config=host.config_from_env({}, batch_doc_max=256))
    got = prog.run_batch(docs)
    _check(blob, docs, got)
    assert prog.last_batch_stats.docs_routed == sum(len(d) > 256 for d in docs)


def test_big_tables_lookahead_and_regex_coders():
    src, words = dictionary_program()
    blob = host.compile_source(src)
    r = random.Random(4)
    docs = [" ".join(r.choice(words) if r.random() < 0.5 else "q%d" % r.randint(0, 99) for _ in range(r.randint(0, 30))).encode() for _ in range(500)]
    docs += [b"A", b"x-y"]
    _check(blob, docs, Program(blob, config=host.config_from_env({}, force=host.KX_FORCE_BIG)).run_batch(docs))
    blob = host.compile_flags(open(host.program_path("iso_datetime_to_json"), "rb").read(), la=True)
    docs = _lines("iso_datetime_to_json", 2000) + [b"2016-01-0", b""]
    _check(blob, docs, Program(blob).run_batch(docs))
    blob = host.compile_regex("([a-z]+)([0-9]*)")
    docs = [b"abc123", b"x", b"", b"12", b"ab1c"] * 50
    _check(blob, docs, Program(blob).run_batch(docs))


def test_capacity_query_exact_cap_and_one_byte_short():
    import ctypes
    import torch
    blob = blob_of("apache_log")
    docs = _lines("apache_log", 500)
    values, offs = host.pack_batch(docs)
    prog = Program(blob)
    v = torch.frombuffer(bytearray(values), dtype=torch.uint8).cuda()
    o = torch.tensor(offs, dtype=torch.int64).cuda()
    ooff = torch.empty(len(docs) + 1, dtype=torch.int64, device="cuda")
    recs = torch.empty((len(docs), 2), dtype=torch.int64, device="cuda")
    want = b"".join(oracle.run(blob, d) for d in docs)

    def call(buf, cap):
        ol = ctypes.c_size_t()
        st = host.KxBatchStats()
        rc = prog._lib.kx_run_batch(prog._h, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(o.data_ptr()), len(docs),
                                    ctypes.c_void_p(buf), cap, ctypes.c_void_p(ooff.data_ptr()), ctypes.c_void_p(recs.data_ptr()),
                                    ctypes.byref(ol), ctypes.byref(st), None)
        return rc, ol.value
    assert call(None, 0) == (-3, len(want))
    assert ooff[-1].item() == len(want)
    out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    assert call(out.data_ptr(), len(want) - 1) == (-3, len(want))
    assert call(out.data_ptr(), len(want)) == (0, len(want))
    assert out.cpu().numpy().tobytes() == want


def test_zero_one_documents_and_no_side_effects_on_single_stream_runs():
    import torch
    blob = blob_of("apache_log")
    prog = Program(blob)
    assert prog.run_batch([]) == []
    out, ooff, status, _, _ = prog.run_batch_tensor(torch.empty(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert out.numel() == 0 and ooff.tolist() == [0] and status.numel() == 0
    data = workloads.generate("apache_log", 1 << 20, seed=9)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    first = prog.run_tensor(t).cpu().numpy().tobytes()
    form = [prog.stage_delayed_form(s) for s in range(prog.num_stages)]
    assert prog.run_batch([data]) == [first]
    long_docs = [data[:300000], data[:300000][:-1]]   # routed: the single-document driver, which may move the delayed form's state
    prog.configure(batch_doc_max=4096)
    _check(blob, long_docs, prog.run_batch(long_docs))
    assert [prog.stage_delayed_form(s) for s in range(prog.num_stages)] == form
    assert prog.run_tensor(t).cpu().numpy().tobytes() == first


def test_decreasing_offsets_are_refused_on_the_device():
    import torch
    prog = Program(blob_of("flip_ab"))
    v = torch.zeros(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(host.EngineError, match="decrease"):
        prog.run_batch_tensor(v, torch.tensor([0, 8, 4, 16], dtype=torch.int64, device="cuda"))
