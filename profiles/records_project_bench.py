"""Field mode, projected (`BIN --records --field=LIST --only`, kx_run_batch_field_project) against the list path it shares every
step but the last two with, on records_field_list_bench.py's data: 2^20 CSV lines of six columns,
`word,stamp,word,stamp,stamp,stamp\\n`, through the `stamp` rule of programs/iso_datetime_to_json.kex.  The batch call alone, device
tensors in and a preallocated output: no file, no split.  One JSON line on stdout (and appended to --json):

  list_24      kx_run_batch_field_list with the list 2,4: every column stays where it was
  only_24      kx_run_batch_field_project with the items 2,4 and OFS = the comma: the two outputs alone
  only_42      the same with the items 4,2

The three variants ALTERNATE, --rounds times (at least three) of --reps calls each after one warm-up call per variant, so that the
run-to-run spread of every figure is known: per variant and round the median milliseconds per call and the HIP-event times of field
mode's own kernel groups (kx_fields_stats); over the rounds the median, the minimum and the maximum of those medians, GB/s of input
bytes, and splice_ms per output megabyte — the figure to compare: the projection writes fewer bytes and reads no gap bytes, so its
splice should cost no more per byte written than the list's.  Every output is compared with the expected bytes, spelled out by hand
from the lines.  The device's clocks as rocm-smi reports them are noted next to the numbers (read only; nothing is set).

  python profiles/records_project_bench.py --json profiles/records_project_bench.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from records_field_bench import clocks, med   # noqa: E402
from records_field_list_bench import csv_lines, want_line   # noqa: E402
from records_field_bench import stamp_program   # noqa: E402

GROUPS = ("locate_ms", "gather_ms", "scan_ms", "splice_ms")


def stamp_json(t):
    return want_line(t + b"\n", [1])[:-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=37)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds: at least 3, so that the spread is known")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from kleenexlang_amd import host
    pool, picks = csv_lines(a.lines, a.seed)
    data = b"".join(pool[i] for i in picks)
    plen = np.array([len(p) for p in pool], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(plen[np.array(picks)])))
    v = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    o = torch.from_numpy(offs).cuda()
    prog = host.Program(host.compile_source(stamp_program()), collect_timing=True)
    res = {"lines": a.lines, "in_bytes": len(data), "reps": a.reps, "rounds": a.rounds, "clocks": clocks()}
    kw = dict(fs=b",", sep_len=1)

    def projected(line, order):
        cols = line[:-1].split(b",")
        return b",".join(stamp_json(cols[k - 1]) for k in order) + b"\n"

    variants = {
        "list_24": ([want_line(p, [2, 4]) for p in pool], lambda out: prog.run_batch_field_list_tensor(v, o, host.parse_field_list("2,4"), out=out, **kw)),
        "only_24": ([projected(p, (2, 4)) for p in pool], lambda out: prog.run_batch_field_project_tensor(v, o, host.parse_field_order("2,4"), b",", out=out, **kw)),
        "only_42": ([projected(p, (4, 2)) for p in pool], lambda out: prog.run_batch_field_project_tensor(v, o, host.parse_field_order("4,2"), b",", out=out, **kw)),
    }
    outs, needs, rounds = {}, {}, {name: [] for name in variants}

    def calls(name, reps):
        want, call = variants[name]
        ms, own = [], []
        for _ in range(reps):
            before = prog.fields_kernel_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call(outs[name])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            after = prog.fields_kernel_stats()
            assert r[0].numel() == needs[name] and int(r[2].max()) == 0, name
            own.append({k: after[k] - before[k] for k in GROUPS})
        return ms, own

    for name, (want, _) in variants.items():                              # the buffers, one warm-up call each, and the bytes
        needs[name] = sum(len(want[i]) for i in picks)
        outs[name] = torch.empty(needs[name], dtype=torch.uint8, device="cuda")
        calls(name, 1)
        assert outs[name].cpu().numpy().tobytes() == b"".join(want[i] for i in picks), "%s: the output differs from the expected bytes" % name
    for _ in range(a.rounds):                                             # the variants alternate
        for name in variants:
            ms, own = calls(name, a.reps)
            rounds[name].append({"ms": statistics.median(ms), **{k: statistics.median(x[k] for x in own) for k in GROUPS}})
    for name in variants:
        per = rounds[name]
        m = statistics.median(r["ms"] for r in per)
        res[name] = {"out_bytes": needs[name], "ms": med([r["ms"] for r in per]), "in_gbps": len(data) / m / 1e6,
                     "own_kernels": {k: med([r[k] for r in per]) for k in GROUPS},
                     "splice_ms_per_out_mb": med([r["splice_ms"] / (needs[name] / 1e6) for r in per]), "rounds": per}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
