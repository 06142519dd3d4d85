"""Quote-aware record mode (`BIN --records --quote`, kx_split_records_quoted) against the unquoted one (`BIN --records`,
kx_split_records).  One JSON line on stdout (and appended to --json):

  split     the split alone on one 1 GiB window of apache_log lines resident on the device (seeded 64 MiB chunk repeated): one
            blocking kx_split_records / kx_split_records_quoted call with a large enough offsets buffer, host round trip
            included; median of --split-reps after one warm-up
  apache    wall time of the produced binary on about --gib GiB of apache_log lines from a page-cached regular file, to /dev/null,
            `--records` and `--records --quote` interleaved, median of --repeats after one warm-up (every line holds balanced
            quotes, so both give the same records)
  rfc4180   wall time of examples/csv_rfc4180.kex's binary with `--records --quote` on about --csv-gib GiB of generated RFC 4180
            rows (seeded 16 MiB chunk repeated, about 10 % of the rows with a quoted line break), and kx_records_stats of one
            in-process kx_run_records_fd_quoted with collect_timing

  python profiles/records_quoted_bench.py --gib 4 --csv-gib 1 --dir /tmp/recqbench
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o recq -- /tmp/recqbench/apache_log.bin --records --quote < /tmp/recqbench/apache_log.in > /dev/null

Kernel times are taken from a separate rocprofv3 run of the binary (second command above), not from this script."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kleenexlang_amd import build, host, program_path, workloads  # noqa: E402

EXAMPLE = os.path.join(ROOT, "kleenexlang_amd", "examples", "csv_rfc4180.kex")


def make_input(path, base, shape, gib):
    reps = max(1, int(gib * (1 << 30)) // len(base))
    if not (os.path.exists(path) and os.path.getsize(path) == reps * len(base)):
        with open(path, "wb") as f:
            for _ in range(reps):
                f.write(base)
    with open(path, "rb") as f:   # into the page cache
        while f.read(64 << 20):
            pass
    return reps * len(base), len(host.split_records_model(base, quote=b'"')) - 1 if shape == "rfc4180" else base.count(b"\n"), reps


def wall(cmd, path, timeout):
    with open(path, "rb") as fi, open(os.devnull, "wb") as fo:
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", str(timeout), *cmd], stdin=fi, stdout=fo, stderr=subprocess.PIPE, timeout=timeout + 30)
        dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (%d): %s" % (" ".join(cmd), r.returncode, r.stderr[-400:].decode("utf-8", "replace")))
    return dt


def summary(v, nbytes):
    med = statistics.median(v)
    return {"wall_s_median": med, "wall_s_min": min(v), "wall_s_max": max(v), "in_GBps": nbytes / med / 1e9}


def split_times(base, reps):
    """Median ms of one blocking split call on a 1 GiB device window of `base` repeated, unquoted and quoted."""
    import torch
    lib = host.load_engine()
    v = torch.frombuffer(bytearray(base), dtype=torch.uint8).cuda().repeat((1 << 30) // len(base) + 1)[:1 << 30]
    nlines = len(host.split_records_model(base)) * ((1 << 30) // len(base) + 1) + 2
    off = torch.empty(nlines, dtype=torch.int64, device="cuda")
    n, po = ctypes.c_uint64(), ctypes.c_uint32()
    vp, op = ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(off.data_ptr())
    calls = {"unquoted": lambda: lib.kx_split_records(vp, v.numel(), 10, 0, op, off.numel(), ctypes.byref(n), None),
             "quoted": lambda: lib.kx_split_records_quoted(vp, v.numel(), 10, 34, 0, 0, op, off.numel(), ctypes.byref(n), ctypes.byref(po), None)}
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
    assert counts["quoted"] == counts["unquoted"], counts
    res["records"] = counts["quoted"]
    res["quoted_over_unquoted"] = res["quoted"]["ms_median"] / res["unquoted"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--csv-gib", type=float, default=1.0)
    ap.add_argument("--dir", default="/tmp/records_quoted_bench")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--split-reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per binary run")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    kexc = os.path.join(build.OUT, "kexc")
    res = {"window_bytes": 1 << 30, "repeats": a.repeats}
    base = workloads.generate("apache_log", 64 << 20, seed=a.seed)
    res["split_1GiB_apache_log"] = split_times(base, a.split_reps)

    data = os.path.join(a.dir, "apache_log.in")
    exe = os.path.join(a.dir, "apache_log.bin")
    nbytes, nlines, reps = make_input(data, base, "apache_log", a.gib)
    subprocess.run([kexc, "compile", "--quiet", program_path("apache_log"), "--out", exe], check=True, timeout=600)
    runs = {"records": [], "records_quote": []}
    wall([exe, "--records", "--quote"], data, a.timeout)   # warm-up: page cache, code objects
    for _ in range(a.repeats):                             # interleaved, so that drift hits both alike
        runs["records"].append(wall([exe, "--records"], data, a.timeout))
        runs["records_quote"].append(wall([exe, "--records", "--quote"], data, a.timeout))
    res["apache_log"] = {"in_bytes": nbytes, "records": nlines * reps, **{k: summary(v, nbytes) for k, v in runs.items()}}
    res["apache_log"]["quote_over_records"] = res["apache_log"]["records_quote"]["wall_s_median"] / res["apache_log"]["records"]["wall_s_median"]

    data = os.path.join(a.dir, "rfc4180.in")
    exe = os.path.join(a.dir, "rfc4180.bin")
    nbytes, nrows, reps = make_input(data, workloads.generate("rfc4180", 16 << 20, seed=a.seed), "rfc4180", a.csv_gib)
    subprocess.run([kexc, "compile", "--quiet", EXAMPLE, "--out", exe], check=True, timeout=600)
    wall([exe, "--records", "--quote"], data, a.timeout)
    v = [wall([exe, "--records", "--quote"], data, a.timeout) for _ in range(a.repeats)]
    prog = host.Program(host.compile_file(EXAMPLE), collect_timing=True)
    with open(data, "rb") as fi, open(os.devnull, "wb") as fo:
        st = prog.run_records_fd(fi.fileno(), fo.fileno(), quote=b'"')
    assert st["records"] == nrows * reps and st["records_rejected"] == 0 and not st["rejected"], st
    res["rfc4180"] = {"in_bytes": nbytes, "records": nrows * reps, "records_quote": summary(v, nbytes), "kx_records_stats": st}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
