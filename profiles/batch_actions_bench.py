"""Batched runs over stages with register actions: the batch replay (kx_config::batch_actions = 2) against the single-document
route, on the two programs of profiles/actions_bench.py with one document per line.  One JSON line per case on stdout (and
appended to --json); every output byte of every document is checked against the CPU oracle.

  python profiles/batch_actions_bench.py                      # replay: 2^20 documents each; route: 2 000 documents, extrapolated
  python profiles/batch_actions_bench.py --route-only         # the route case alone (also runs on a tree without the switch)

The step is one kx_run_batch call with an exactly sized output: HIP events on the current stream, median of --repeats after
--warmup calls.  long_lines runs three times: lanes / waves chosen by the engine, waves only, lanes only (kx_config::act_lanes)."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from kleenexlang_amd import host  # noqa: E402
from oracle import oracle  # noqa: E402

PROGRAMS = {   # (profiles/actions_bench.py)
    "swap_fields": ('main := (a@/[a-z]*/ ~/,/ b@/[0-9]*/ !b "," !a /\\n/)*\n',
                    lambda r: b"%s,%d\n" % (bytes(r.choice(b"abcdefgh") for _ in range(r.randrange(1, 9))), r.randrange(10 ** 6))),
    "long_lines": ('main := (l@/[^\\n]*/ ~/\\n/ "<" !l ">\\n")*\n',
                   lambda r: bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz ") for _ in range(r.randrange(150, 400))) + b"\n"),
}
HAS_SWITCH = "batch_actions" in [f[0] for f in host.KxConfig._fields_]
SPLITS = ("forward_ms", "back_ms", "scan_ms", "emit_ms", "routed_ms", "total_ms") + (("actions_ms",) if HAS_SWITCH else ())


def run_case(name, ndocs, repeats, warmup, **fields):
    src, line = PROGRAMS[name]
    r = random.Random(5)
    pool = [line(r) for _ in range(20000)]
    docs = [pool[r.randrange(len(pool))] for _ in range(ndocs)]
    blob = host.compile_source(src)
    want = {d: oracle.run(blob, d) for d in set(docs)}
    values, offs = host.pack_batch(docs)
    dev = torch.device("cuda", 0)
    v = torch.frombuffer(bytearray(values), dtype=torch.uint8).to(dev)
    o = torch.tensor(offs, dtype=torch.int64).to(dev)
    prog = host.Program(blob, config=host.config_from_env({}, **fields), collect_timing=True)
    need = sum(len(want[d]) for d in docs)
    buf = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    ooff = torch.empty(ndocs + 1, dtype=torch.int64, device=dev)
    recs = torch.empty((ndocs, 2), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)

    def step():
        ol = ctypes.c_size_t()
        st = host.KxBatchStats()
        rc = prog._lib.kx_run_batch(prog._h, ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(o.data_ptr()), ndocs, ctypes.c_void_p(buf.data_ptr()),
                                    buf.numel(), ctypes.c_void_p(ooff.data_ptr()), ctypes.c_void_p(recs.data_ptr()), ctypes.byref(ol),
                                    ctypes.byref(st), ctypes.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise host.EngineError(prog._err())
        return st

    for _ in range(warmup):
        step()
    times, splits = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = step()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
        splits.append(st.as_dict())
    ob, oo = buf[:need].cpu().numpy().tobytes(), ooff.tolist()
    bad = sum(ob[oo[i]:oo[i + 1]] != want[d] for i, d in enumerate(docs)) + (oo[ndocs] != need)
    med = statistics.median(times)
    return {"program": name, "docs": ndocs, "in_bytes": len(values), "out_bytes": need, "config": fields,
            "step_ms": {"median": med, "min": min(times), "max": max(times), "repeats": repeats, "warmup": warmup},
            "us_per_doc": med / ndocs * 1e3, "docs_per_s": ndocs / med * 1e3, "in_GBps": len(values) / med / 1e6,
            "split_ms_median_step": {k: statistics.median(s[k] for s in splits) for k in SPLITS},
            "docs_routed": splits[-1]["docs_routed"], "docs_replayed": splits[-1].get("docs_replayed", 0),
            "checked_docs": ndocs, "mismatches": bad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--route-docs", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cases = []
    if not a.route_only:
        cases += [("swap_fields", a.docs, a.repeats, a.warmup, {"batch_actions": 2}), ("swap_fields", 1 << 16, a.repeats, a.warmup, {"batch_actions": 2})]
        cases += [("long_lines", a.docs, a.repeats, a.warmup, {"batch_actions": 2, "act_lanes": k}) for k in (0, 1, 2)]
    route = {"batch_actions": 1} if HAS_SWITCH else {}     # (a tree without the switch routes every document of an action stage)
    cases += [(name, a.route_docs, 3, 1, route) for name in ("swap_fields", "long_lines")]
    bad = 0
    for name, ndocs, repeats, warmup, fields in cases:
        res = run_case(name, ndocs, repeats, warmup, **fields)
        if res["docs_routed"]:
            res["extrapolated_to_2^20_docs_s"] = res["us_per_doc"] * (1 << 20) / 1e6
        line = json.dumps(res)
        print(line, flush=True)
        if a.json:
            with open(a.json, "a") as f:
                f.write(line + "\n")
        bad += res["mismatches"]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
