"""Escape-aware record mode (`BIN --records --escape`, kx_split_records_escaped) against the plain and the quoted splits.  One
JSON line on stdout (and appended to --json):

  split        the split alone on one 1 GiB window of apache_log lines resident on the device (seeded 64 MiB chunk repeated):
               one blocking kx_split_records / kx_split_records_quoted / kx_split_records_escaped (no quote, and with a quote)
               call with a large enough offsets buffer, host round trip included; median of --split-reps after one warm-up.  The
               lines hold no backslash and balanced quotes, so all four give the same records
  csv_escaped  wall time of examples/csv_escaped.kex's binary with `--records --quote --escape` on about --csv-gib GiB of
               generated rows (seeded 8 MiB chunk of csv.writer(escapechar='\\', doublequote=False) rows repeated), to /dev/null,
               median of --repeats after one warm-up, and kx_records_stats of one in-process kx_run_records_fd_escaped with
               collect_timing

  python profiles/records_escaped_bench.py --csv-gib 1 --dir /tmp/receb
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o rece -- /tmp/receb/csv_escaped.bin --records --quote --escape < /tmp/receb/csv_escaped.in > /dev/null

Kernel times are taken from a separate rocprofv3 run of the binary (second command above), not from this script."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from kleenexlang_amd import build, host, workloads  # noqa: E402
from records_quoted_bench import make_input, summary, wall  # noqa: E402

EXAMPLE = os.path.join(ROOT, "kleenexlang_amd", "examples", "csv_escaped.kex")


def split_times(base, reps):
    """Median ms of one blocking split call on a 1 GiB device window of `base` repeated, for each split."""
    import time
    import torch
    lib = host.load_engine()
    v = torch.frombuffer(bytearray(base), dtype=torch.uint8).cuda().repeat((1 << 30) // len(base) + 1)[:1 << 30]
    nlines = len(host.split_records_model(base)) * ((1 << 30) // len(base) + 1) + 2
    off = torch.empty(nlines, dtype=torch.int64, device="cuda")
    n, po = ctypes.c_uint64(), ctypes.c_uint32()
    vp, op = ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(off.data_ptr())
    calls = {"plain": lambda: lib.kx_split_records(vp, v.numel(), 10, 0, op, off.numel(), ctypes.byref(n), None),
             "quoted": lambda: lib.kx_split_records_quoted(vp, v.numel(), 10, 34, 0, 0, op, off.numel(), ctypes.byref(n), ctypes.byref(po), None),
             "escaped": lambda: lib.kx_split_records_escaped(vp, v.numel(), 10, -1, 92, 0, 0, op, off.numel(), ctypes.byref(n), ctypes.byref(po),
                                                             None),
             "escaped_quoted": lambda: lib.kx_split_records_escaped(vp, v.numel(), 10, 34, 92, 0, 0, op, off.numel(), ctypes.byref(n),
                                                                    ctypes.byref(po), None)}
    res, counts = {}, {}
    for k, f in calls.items():
        assert f() == 0
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = f()
            ts.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        res[k] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}
        counts[k] = n.value
    assert len(set(counts.values())) == 1, counts
    res["records"] = counts["plain"]
    for k in ("escaped", "escaped_quoted"):
        res[k + "_over_quoted"] = res[k]["ms_median"] / res["quoted"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csv-gib", type=float, default=1.0)
    ap.add_argument("--dir", default="/tmp/records_escaped_bench")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--split-reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per binary run")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    kexc = os.path.join(build.OUT, "kexc")
    res = {"window_bytes": 1 << 30, "repeats": a.repeats}
    res["split_1GiB_apache_log"] = split_times(workloads.generate("apache_log", 64 << 20, seed=a.seed), a.split_reps)

    data = os.path.join(a.dir, "csv_escaped.in")
    exe = os.path.join(a.dir, "csv_escaped.bin")
    base = workloads.generate("csv_escaped", 8 << 20, seed=a.seed)
    nrows = len(host.split_escaped_records_model(base, quote=b'"')[0]) - 1
    nbytes, _, reps = make_input(data, base, "csv_escaped", a.csv_gib)
    subprocess.run([kexc, "compile", "--quiet", EXAMPLE, "--out", exe], check=True, timeout=600)
    args = ["--records", "--quote", "--escape"]
    wall([exe, *args], data, a.timeout)
    v = [wall([exe, *args], data, a.timeout) for _ in range(a.repeats)]
    prog = host.Program(host.compile_file(EXAMPLE), collect_timing=True)
    with open(data, "rb") as fi, open(os.devnull, "wb") as fo:
        st = prog.run_records_fd(fi.fileno(), fo.fileno(), quote=b'"', escape=b"\\")
    assert st["records"] == nrows * reps and st["records_rejected"] == 0 and not st["rejected"], st
    res["csv_escaped"] = {"in_bytes": nbytes, "records": nrows * reps, "records_quote_escape": summary(v, nbytes), "kx_records_stats": st}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
