"""Field mode (`BIN --records --field=2 --fs=,`, kx_run_batch_fields) on 2^20 CSV lines of three columns with an ISO date-time in
the middle, through the `stamp` rule of programs/iso_datetime_to_json.kex (stamp_program below: the shipped program reads
newline-terminated stamps, a field holds one stamp and no newline).  One JSON line on stdout (and
appended to --json):

  field    kx_run_records_fd_fields, file to file: wall time, split_ms and batch_ms of kx_records_stats (HIP events), and the summed
           HIP-event time of field mode's own kernels (kx_fields_stats: locate, gather, the two scans, splice); median / min /
           max of --reps runs after one warm-up
  copy     the yardstick: plain `--records` of a copy-through program over the same file (kx_run_records_fd).  On an engine
           library without kx_run_batch_fields (the parent commit, --package-root) only this run is made.

The device's clocks as rocm-smi reports them are noted next to the numbers (read only; nothing is set).

  python profiles/records_field_bench.py --json profiles/records_field_bench.json
  python profiles/records_field_bench.py --package-root PARENT_CHECKOUT --json profiles/records_field_bench.json"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY = 'main := /[^\\n]*\\n?/\n'


def csv_lines(nlines, seed):
    r = random.Random(seed)
    word = lambda: bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(1, 12)))   # noqa: E731
    stamp = lambda: b"%04d-%02d-%02dT%02d:%02d:%02d%s" % (r.randrange(1970, 2040), r.randrange(1, 13), r.randrange(1, 29), r.randrange(24),   # noqa: E731
                                                         r.randrange(60), r.randrange(60), r.choice((b"Z", b"+01:00", b"-05:30")))
    pool = [word() + b"," + stamp() + b"," + word() + b"\n" for _ in range(8192)]
    picks = [r.randrange(len(pool)) for _ in range(nlines)]
    return b"".join(pool[i] for i in picks), pool, picks


def want_line(line):
    """What field mode must write for a pool line: the stamp rule's output, spelled out by hand."""
    a, t, b = line[:-1].split(b",")
    js = b"{'year'='%s', 'month'='%s', 'day'='%s', 'hours'='%s', 'minutes'='%s', 'seconds'='%s', 'tz'='%s'}" % (
        t[0:4], t[5:7], t[8:10], t[11:13], t[14:16], t[17:19], t[19:])
    return a + b"," + js + b"," + b + b"\n"


def stamp_program():
    """programs/iso_datetime_to_json.kex for one stamp without a newline: its text with the two places that name the newline changed."""
    with open(os.path.join(ROOT, "kleenexlang_amd", "programs", "iso_datetime_to_json.kex")) as f:
        src = f.read()
    for old, new in (("stamps := (stamp ~/\\n/)+", "stamps := stamp"), ('"}\\n"', '"}"')):
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    return src


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "--json"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=30).stdout.decode()[:2000]
    except Exception as e:   # noqa: BLE001
        return "unavailable: %s" % e


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose kleenexlang_amd package (and engine library) is measured")
    ap.add_argument("--label", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from kleenexlang_amd import host
    fields = hasattr(host, "KxBatchFields")
    data, pool, picks = csv_lines(a.lines, a.seed)
    res = {"label": a.label or ("this commit" if fields else "without kx_run_batch_fields"), "lines": a.lines, "in_bytes": len(data),
           "reps": a.reps, "clocks": clocks()}
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "in")
        with open(src, "wb") as f:
            f.write(data)

        def run(prog, name, **kw):
            fi, fo = os.open(src, os.O_RDONLY), os.open(os.path.join(d, "out_" + name), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
            try:
                t0 = time.perf_counter()
                st = prog.run_records_fd(fi, fo, **kw)
                st["wall_ms"] = (time.perf_counter() - t0) * 1e3
            finally:
                os.close(fi)
                os.close(fo)
            assert st["records"] == a.lines and not st["rejected"], st
            return st

        copy = host.Program(host.compile_source(COPY), collect_timing=True)
        run(copy, "copy")
        sts = [run(copy, "copy") for _ in range(a.reps)]
        res["copy"] = {k: med([s[k] for s in sts]) for k in ("wall_ms", "split_ms", "batch_ms")}
        with open(os.path.join(d, "out_copy"), "rb") as f:
            assert f.read() == data
        if fields:
            prog = host.Program(host.compile_source(stamp_program()), collect_timing=True)
            run(prog, "field", field=2, fs=b",")
            sts, own = [], []
            for _ in range(a.reps):
                before = prog.fields_kernel_stats()
                sts.append(run(prog, "field", field=2, fs=b","))
                after = prog.fields_kernel_stats()
                own.append({k: after[k] - before[k] for k in ("locate_ms", "gather_ms", "scan_ms", "splice_ms")})
            res["field"] = {k: med([s[k] for s in sts]) for k in ("wall_ms", "split_ms", "batch_ms")}
            res["field"]["out_bytes"] = sts[0]["out_bytes"]
            res["field"]["own_kernels"] = {k: med([o[k] for o in own]) for k in own[0]}
            sums = [sum(o.values()) for o in own]
            res["field"]["own_kernels_ms"] = med(sums)
            res["field"]["own_share_of_compute"] = statistics.median(s / (st["split_ms"] + st["batch_ms"]) for s, st in zip(sums, sts))
            with open(os.path.join(d, "out_field"), "rb") as f:
                got = f.read()
            want = [want_line(x) for x in pool]
            assert got == b"".join(want[i] for i in picks), "field mode's output differs from the expected bytes"
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
