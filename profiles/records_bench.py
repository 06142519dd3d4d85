"""Record mode (`BIN --records`, kx_run_records_fd) against the whole-stream run (`BIN`), wall time of the produced binary on
apache_log lines from a page-cached regular file (seeded; about --gib GiB).  One JSON line on stdout (and appended to --json).

  python profiles/records_bench.py --gib 4 --dir /tmp/recbench
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o rec -- /tmp/recbench/apache_log.bin --records < /tmp/recbench/apache_log.in > /dev/null

Every binary run writes to /dev/null, so the writer thread still copies device to host and calls write().  kx_records_stats
comes from one in-process kx_run_records_fd with collect_timing (split_ms / batch_ms: HIP events).  Kernel times are taken
from a separate rocprofv3 run of the binary (second command above), not from this script."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kleenexlang_amd import build, host, program_path, workloads  # noqa: E402


def make_input(path, gib, seed):
    base = workloads.generate("apache_log", 64 << 20, seed=seed)
    reps = max(1, int(gib * (1 << 30)) // len(base))
    if not (os.path.exists(path) and os.path.getsize(path) == reps * len(base)):
        with open(path, "wb") as f:
            for _ in range(reps):
                f.write(base)
    with open(path, "rb") as f:   # into the page cache
        while f.read(64 << 20):
            pass
    return reps * len(base), base.count(b"\n") * reps


def wall(cmd, path, timeout):
    with open(path, "rb") as fi, open(os.devnull, "wb") as fo:
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", str(timeout), *cmd], stdin=fi, stdout=fo, stderr=subprocess.PIPE, timeout=timeout + 30)
        dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (%d): %s" % (" ".join(cmd), r.returncode, r.stderr[-400:].decode("utf-8", "replace")))
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--dir", default="/tmp/records_bench")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per binary run")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    data = os.path.join(a.dir, "apache_log.in")
    exe = os.path.join(a.dir, "apache_log.bin")
    nbytes, nlines = make_input(data, a.gib, a.seed)
    subprocess.run([os.path.join(build.OUT, "kexc"), "compile", "--quiet", program_path("apache_log"), "--out", exe], check=True, timeout=600)
    runs = {"whole": [], "records": []}
    wall([exe], data, a.timeout)                 # warm-up: page cache, code objects
    for _ in range(a.repeats):                   # interleaved, so that drift hits both alike
        runs["whole"].append(wall([exe], data, a.timeout))
        runs["records"].append(wall([exe, "--records"], data, a.timeout))
    prog = host.Program(host.compile_file("apache_log"), collect_timing=True)
    with open(data, "rb") as fi, open(os.devnull, "wb") as fo:
        st = prog.run_records_fd(fi.fileno(), fo.fileno())
    res = {"program": "apache_log", "in_bytes": nbytes, "records": nlines, "window_bytes": 1 << 30, "repeats": a.repeats}
    for k, v in runs.items():
        med = statistics.median(v)
        res[k] = {"wall_s_median": med, "wall_s_min": min(v), "wall_s_max": max(v), "in_GBps": nbytes / med / 1e9}
    res["records_over_whole"] = res["records"]["wall_s_median"] / res["whole"]["wall_s_median"]
    res["kx_records_stats"] = st
    assert st["records"] == nlines and st["records_rejected"] == 0 and not st["rejected"], st
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
