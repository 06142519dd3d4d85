"""Field mode by key (`BIN --records --blanks --keys --field=LIST`, kx_run_batch_field_keys) on 2^20 generated logfmt lines,
`ts=… level=… msg=… dur=…\\n`, through a program that copies its input: what is timed is the selection, not the program.  The batch
call alone, device tensors in and a preallocated output: no file, no split.  One JSON line on stdout (and appended to --json):

  keys_1, keys_2     kx_run_batch_field_keys with the lists msg / ts,msg on words: milliseconds per call (median / min / max of
                     --reps calls after one warm-up), GB/s of input bytes, and the HIP-event times of field mode's own kernel groups
                     (kx_fields_stats; count and locate are both in locate_ms)
  words_1, words_2   the positional selection of the SAME words, `--blanks --field=3` / `--blanks --field=1,3`
                     (kx_run_batch_field_words), on the same data with a build of the PARENT commit: --parent-root names a checkout
                     of it in which `python -m kleenexlang_amd.build` has run; the numbers come from a child process that imports
                     that tree (`--role positional`).  The key `msg=` is then part of the word, so the outputs differ by design
                     and are only compared in length.

Every keyed output is compared with the expected bytes (the program copies: the lines themselves).  The device's clocks as
rocm-smi reports them are noted next to the numbers (read only; nothing is set).

  python profiles/records_keys_bench.py --parent-root ../parent --json profiles/records_keys_bench.json"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY = 'main := /[^\\n]*/\n'


def logfmt_lines(nlines, seed):
    r = random.Random(seed)
    word = lambda: bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(1, 12)))   # noqa: E731
    pool = [b"ts=2026-10-%02dT%02d:%02d:%02dZ level=%s msg=%s dur=%dms\n" % (r.randrange(1, 29), r.randrange(24), r.randrange(60), r.randrange(60),
                                                                           r.choice((b"info", b"warn", b"error")), word(), r.randrange(1000))
            for _ in range(8192)]
    return pool, [r.randrange(len(pool)) for _ in range(nlines)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=41)
    ap.add_argument("--json", default=None)
    ap.add_argument("--parent-root", required=True, help="a built checkout of the parent commit, for the positional runs")
    ap.add_argument("--role", default="keyed", choices=("keyed", "positional"))
    a = ap.parse_args()
    sys.path.insert(0, a.parent_root if a.role == "positional" else ROOT)
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    import numpy as np
    import torch
    from kleenexlang_amd import host
    from records_field_bench import clocks, med
    pool, picks = logfmt_lines(a.lines, a.seed)
    data = b"".join(pool[i] for i in picks)
    offs = np.concatenate(([0], np.cumsum(np.array([len(p) for p in pool], dtype=np.int64)[np.array(picks)])))
    v = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    o = torch.from_numpy(offs).cuda()
    prog = host.Program(host.compile_source(COPY), collect_timing=True)
    res = {"role": a.role, "lines": a.lines, "in_bytes": len(data), "reps": a.reps, "clocks": clocks()}

    def measure(name, call, check):
        out = torch.empty(len(data), dtype=torch.uint8, device="cuda")
        ms, own = [], []
        for rep in range(a.reps + 1):                                     # (the first call is the warm-up)
            before = prog.fields_kernel_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call(out)
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            after = prog.fields_kernel_stats()
            assert r[0].numel() == len(data) and int(r[2].max()) == 0, name
            if rep:
                ms.append(t)
                own.append({k: after[k] - before[k] for k in ("locate_ms", "gather_ms", "scan_ms", "splice_ms")})
        if check:
            assert out.cpu().numpy().tobytes() == data, "%s: the output differs from the expected bytes" % name
        m = statistics.median(ms)
        res[name] = {"ms": med(ms), "spread_ms": max(ms) - min(ms), "in_gbps": len(data) / m / 1e6,
                     "own_kernels": {k: med([x[k] for x in own]) for k in own[0]}}

    if a.role == "keyed":
        for name, names in (("keys_1", [b"msg"]), ("keys_2", [b"ts", b"msg"])):
            measure(name, lambda out, names=names: prog.run_batch_field_keys_tensor(v, o, names, blanks=True, sep_len=1, out=out), True)
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--role", "positional", "--parent-root", a.parent_root, "--lines", str(a.lines),
                                "--reps", str(a.reps), "--seed", str(a.seed)], stdout=subprocess.PIPE, check=True, timeout=3600)
        res["parent"] = json.loads(child.stdout.decode().strip().splitlines()[-1])
    else:
        for name, text in (("words_1", "3"), ("words_2", "1,3")):
            ranges = host.parse_field_list(text)
            measure(name, lambda out, ranges=ranges: prog.run_batch_field_words_tensor(v, o, ranges, sep_len=1, out=out), False)
    line = json.dumps(res)
    print(line)
    if a.json and a.role == "keyed":
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
