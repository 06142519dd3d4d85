"""Batched runs (kx_run_batch): documents/s and input GB/s of one engine call over many documents, checked byte for byte
against the CPU oracle per document.  One JSON line per run on stdout (and appended to --json).

  python profiles/batch_bench.py --program apache_log --docs 1048576               # one document per apache_log line
  python profiles/batch_bench.py --program csv2json --docs 1048576                 # one per csv row
  python profiles/batch_bench.py --program apache_log --mix skewed --docs 16384    # whole-line documents, lengths log-uniform 0..64 KiB

The step is the kx_run_batch call with an exactly sized output (HIP events on the current stream, after --warmup calls).  For
apache_log the concatenated documents are themselves a valid input: kx_run_device over them gives the single-stream rate.  The
one-call-per-document rate is measured on a subsample (at most 2 000 documents) and extrapolated."""
import argparse
import ctypes
import json
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from kleenexlang_amd import compile_file, host, workloads  # noqa: E402
from oracle import oracle  # noqa: E402


def make_docs(program, mix, ndocs, seed):
    shape = workloads.PROGRAM_INPUT[program]
    gen = workloads._LINE[shape]
    r = random.Random(seed)
    if mix == "lines":
        return [(gen(r)).encode("ascii") for _ in range(ndocs)]
    docs = []
    for _ in range(ndocs):   # whole lines up to a length drawn log-uniform from [1, 64 KiB] (0 with the weight of one octave)
        want = 0 if r.random() < 1 / 17 else int(math.exp(r.uniform(0, math.log(64 << 10))))
        parts, n = [], 0
        while True:
            ln = gen(r)
            if n + len(ln) > want:
                break
            parts.append(ln)
            n += len(ln)
        docs.append("".join(parts).encode("ascii"))
    return docs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="apache_log")
    ap.add_argument("--mix", choices=["lines", "skewed"], default="lines")
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--doc-max", type=int, default=0, help="kx_config::batch_doc_max (0 = the engine's default)")
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    blob = compile_file(a.program)
    docs = make_docs(a.program, a.mix, a.docs, a.seed)
    values, offs = host.pack_batch(docs)
    dev = torch.device("cuda", 0)
    v = torch.frombuffer(bytearray(values), dtype=torch.uint8).to(dev)
    o = torch.tensor(offs, dtype=torch.int64).to(dev)
    prog = host.Program(blob, config=host.config_from_env({}, batch_doc_max=a.doc_max), collect_timing=True)
    out, ooff, status, fpos, fstage = prog.run_batch_tensor(v, o)
    torch.cuda.synchronize()
    need = out.numel()
    buf = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    n = len(docs)
    ooff2 = torch.empty(n + 1, dtype=torch.int64, device=dev)
    recs = torch.empty((n, 2), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)

    def step():
        ol = ctypes.c_size_t()
        st = host.KxBatchStats()
        rc = prog._lib.kx_run_batch(prog._h, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(o.data_ptr()), n, ctypes.c_void_p(buf.data_ptr()),
                                    buf.numel(), ctypes.c_void_p(ooff2.data_ptr()), ctypes.c_void_p(recs.data_ptr()), ctypes.byref(ol),
                                    ctypes.byref(st), ctypes.c_void_p(stream.cuda_stream))
        if rc not in (0, 1):
            raise host.EngineError(prog._err())
        return st

    for _ in range(a.warmup):
        step()
    times, splits = [], []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = step()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
        splits.append(st.as_dict())
    med = statistics.median(times)
    res = {"program": a.program, "mix": a.mix, "docs": n, "in_bytes": len(values), "out_bytes": need,
           "doc_len_max": max(len(d) for d in docs), "batch_doc_max": a.doc_max or 65536,
           "step_ms": {"median": med, "min": min(times), "max": max(times), "repeats": a.repeats, "warmup": a.warmup},
           "in_GBps": len(values) / med / 1e6, "docs_per_s": n / med * 1e3,
           "split_ms_median_step": {k: statistics.median(s[k] for s in splits) for k in ("forward_ms", "back_ms", "scan_ms", "emit_ms", "routed_ms", "total_ms")},
           "docs_rejected": splits[-1]["docs_rejected"], "docs_routed": splits[-1]["docs_routed"]}
    if a.program == "apache_log":   # the concatenation is itself a valid input: the single-stream rate over the same bytes
        single = host.Program(blob)
        so = torch.empty(single.out_capacity(len(values), 3), dtype=torch.uint8, device=dev)
        for _ in range(2):
            single.run_device(v.data_ptr(), len(values), so.data_ptr(), so.numel(), stream.cuda_stream)
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            single.run_device(v.data_ptr(), len(values), so.data_ptr(), so.numel(), stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        res["single_stream"] = {"step_ms_median": statistics.median(ts), "in_GBps": len(values) / statistics.median(ts) / 1e6}
    sub = random.Random(1).sample(range(n), min(n, 2000))   # one engine call per document, on a subsample
    single = host.Program(blob)
    so = torch.empty(single.out_capacity(max(len(docs[i]) for i in sub), 3), dtype=torch.uint8, device=dev)
    dts = [torch.frombuffer(bytearray(docs[i]), dtype=torch.uint8).to(dev) if docs[i] else torch.empty(0, dtype=torch.uint8, device=dev) for i in sub]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in dts:
        try:
            single.run_device(t.data_ptr(), t.numel(), so.data_ptr(), so.numel(), stream.cuda_stream)
        except host.MatchError:
            pass
    torch.cuda.synchronize()
    per_doc = (time.perf_counter() - t0) / len(sub)
    res["per_document_loop"] = {"subsample": len(sub), "s_per_doc": per_doc, "extrapolated_step_ms": per_doc * n * 1e3,
                                "extrapolated_docs_per_s": 1 / per_doc, "note": "extrapolated from the subsample"}
    if not a.no_check:   # every output byte against the oracle, document by document
        ob = buf[:need].cpu().numpy().tobytes()
        oo, stt, fp = ooff2.tolist(), recs[:, 1].cpu().tolist(), recs[:, 0].cpu().tolist()
        bad = 0
        for i, d in enumerate(docs):
            try:
                w = oracle.run(blob, d)
                ok = (stt[i] & 0xFFFFFFFF) == 0 and ob[oo[i]:oo[i + 1]] == w
            except oracle.OracleMatchError as e:
                ok = (stt[i] & 0xFFFFFFFF) == 1 and fp[i] == e.pos and oo[i] == oo[i + 1]
            bad += 0 if ok else 1
        res["checked_docs"], res["mismatches"] = n, bad
    line = json.dumps(res)
    print(line, flush=True)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")
    if res.get("mismatches"):
        sys.exit(1)


if __name__ == "__main__":
    main()
