"""Record mode with a multi-byte separator (`BIN --records --rs=STR`, kx_split_records_rs) against the plain split.  One JSON line
on stdout (and appended to --json):

  split   the split alone on one 1 GiB window of CRLF log lines resident on the device (a seeded 64 MiB chunk of apache_log
          lines with every \\n turned into \\r\\n, and a blank line behind every 16th, repeated): one blocking call with a large
          enough offsets buffer, host round trip included; median of --split-reps after one warm-up, for
            plain         kx_split_records, separator \\n
            crlf          kx_split_records_rs, separator \\r\\n (border-free: every candidate is selected)
            blank_line    kx_split_records_rs, separator \\r\\n\\r\\n (self-overlapping: maps, their scans and counts per state)
            double_lf     kx_split_records_rs, separator \\n\\n (self-overlapping; no candidate in this data)

  python profiles/records_rs_bench.py --json profiles/records_rs_bench.json
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o rs -- python profiles/records_rs_bench.py --split-reps 3

Kernel times are taken from a separate rocprofv3 run (second command above), not from this script's clock."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kleenexlang_amd import host, workloads  # noqa: E402


def crlf_lines(nbytes, seed):
    """apache_log lines ended by \\r\\n, a blank line (\\r\\n\\r\\n) behind every 16th."""
    lines = workloads.generate("apache_log", nbytes, seed=seed).split(b"\n")[:-1]
    return b"".join(l + (b"\r\n\r\n" if i % 16 == 15 else b"\r\n") for i, l in enumerate(lines))


def split_times(base, reps):
    import torch
    lib = host.load_engine()
    times = (1 << 30) // len(base) + 1
    v = torch.frombuffer(bytearray(base), dtype=torch.uint8).cuda().repeat(times)[:1 << 30]
    off = torch.empty(base.count(b"\n") * times + 2, dtype=torch.int64, device="cuda")
    n = ctypes.c_uint64()
    vp, op = ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(off.data_ptr())
    rs = lambda s: lambda: lib.kx_split_records_rs(vp, v.numel(), s, len(s), b"", 0, 0, op, off.numel(), ctypes.byref(n), None, None, None, None)
    calls = {"plain": lambda: lib.kx_split_records(vp, v.numel(), 10, 0, op, off.numel(), ctypes.byref(n), None),
             "crlf": rs(b"\r\n"), "blank_line": rs(b"\r\n\r\n"), "double_lf": rs(b"\n\n")}
    res = {}
    for k, f in calls.items():
        assert f() == 0
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = f()
            ts.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        res[k] = {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "records": n.value}
    assert res["plain"]["records"] == res["crlf"]["records"] and res["double_lf"]["records"] == 1, res
    for k in ("crlf", "blank_line", "double_lf"):
        res[k + "_over_plain"] = res[k]["ms_median"] / res["plain"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--split-reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"window_bytes": 1 << 30, "split_1GiB_crlf_log": split_times(crlf_lines(64 << 20, a.seed), a.split_reps)}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
