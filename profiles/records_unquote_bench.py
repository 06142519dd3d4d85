"""Field mode on unquoted values (`BIN --records --quote --field=2,4 --fs=, --unquote`, kx_run_records_fd_field_values) against the
parent commit's `--field=2,4` on the same file: 2^20 QUOTE_ALL lines `"word","stamp","word","stamp"\\n` with ISO date-times
(the size of profiles/records_field_bench.py's file), file to file through Program.run_records_fd in one window.

  unquote   this commit: the `stamp` rule of programs/iso_datetime_to_json.kex (as profiles/records_field_bench.py makes it) runs on
            the VALUE of columns 2 and 4; its output holds the field separator, so it is spelled inside quotes again
  parent    a checkout of the parent commit (--parent-root, built): the same rule between two copied quote bytes runs on the raw
            columns 2 and 4 — the way to get these bytes without --unquote

Both write the same bytes, and every run's output is compared with them, spelled out by hand.  The two alternate --rounds times
(at least 3), each run a process of its own with --reps timed calls after one warm-up; per round the medians of wall_ms, split_ms
and batch_ms (kx_records_stats) and of field mode's kernel groups (kx_fields_stats), and over the rounds the spread of those
medians.  One JSON line on stdout, appended to --json (profiles/records_unquote_bench.json unless given).  Without --parent-root
nothing runs: a figure of this commit alone is no comparison.  The device's clocks as rocm-smi reports them are noted (read only).

  python profiles/records_unquote_bench.py --parent-root PARENT_CHECKOUT"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from records_field_bench import clocks, med, stamp_program   # noqa: E402


def csv_lines(nlines, seed):
    r = random.Random(seed)
    word = lambda: bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(1, 12)))   # noqa: E731
    stamp = lambda: b"%04d-%02d-%02dT%02d:%02d:%02d%s" % (r.randrange(1970, 2040), r.randrange(1, 13), r.randrange(1, 29), r.randrange(24),   # noqa: E731
                                                         r.randrange(60), r.randrange(60), r.choice((b"Z", b"+01:00", b"-05:30")))
    pool = [b",".join(b'"' + x + b'"' for x in (word(), stamp(), word(), stamp())) + b"\n" for _ in range(8192)]
    picks = [r.randrange(len(pool)) for _ in range(nlines)]
    return pool, picks


def want_line(line):
    """What both runs must write for a pool line: the stamp rule's output in columns 2 and 4, inside quotes."""
    cols = [c[1:-1] for c in line[:-1].split(b",")]
    for k in (1, 3):
        t = cols[k]
        cols[k] = b"{'year'='%s', 'month'='%s', 'day'='%s', 'hours'='%s', 'minutes'='%s', 'seconds'='%s', 'tz'='%s'}" % (
            t[0:4], t[5:7], t[8:10], t[11:13], t[14:16], t[17:19], t[19:])
    return b",".join(b'"' + c + b'"' for c in cols) + b"\n"


def quoted_stamp_program():
    """The stamp rule between two copied quote bytes: what the parent commit runs on the raw field."""
    src = stamp_program()
    assert src.count("stamps := stamp") == 1
    return src.replace("stamps := stamp", 'stamps := /"/ stamp /"/')


def one(a):
    """One process: --reps timed runs of one variant after a warm-up; the result as a JSON line on stdout."""
    sys.path.insert(0, os.path.abspath(a.package_root))
    from kleenexlang_amd import host
    unquote = a.one == "unquote"
    pool, picks = csv_lines(a.lines, a.seed)
    data = b"".join(pool[i] for i in picks)
    want = [want_line(p) for p in pool]
    prog = host.Program(host.compile_source(stamp_program() if unquote else quoted_stamp_program()), collect_timing=True)
    kw = dict(quote=b'"', fields=[2, 4], fs=b",", **({"unquote": True} if unquote else {}))
    sts, own = [], []
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in"), os.path.join(d, "out")
        with open(src, "wb") as f:
            f.write(data)
        for rep in range(a.reps + 1):                                     # (the first run is the warm-up)
            before = prog.fields_kernel_stats()
            fi, fo = os.open(src, os.O_RDONLY), os.open(dst, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
            try:
                t0 = time.perf_counter()
                st = prog.run_records_fd(fi, fo, **kw)
                st["wall_ms"] = (time.perf_counter() - t0) * 1e3
            finally:
                os.close(fi)
                os.close(fo)
            after = prog.fields_kernel_stats()
            assert st["records"] == a.lines and not st["rejected"], st
            if rep:
                sts.append(st)
                own.append({k: after[k] - before[k] for k in ("locate_ms", "gather_ms", "scan_ms", "splice_ms")})
        with open(dst, "rb") as f:
            assert f.read() == b"".join(want[i] for i in picks), "%s: the output differs from the expected bytes" % a.one
    res = {k: med([s[k] for s in sts]) for k in ("wall_ms", "split_ms", "batch_ms")}
    res.update(in_bytes=len(data), out_bytes=sts[0]["out_bytes"], own_kernels={k: med([o[k] for o in own]) for k in own[0]})
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=41)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (required: the two are compared)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "records_unquote_bench.json"), help="the file the result line is appended to")
    ap.add_argument("--one", choices=("unquote", "parent"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    if a.rounds < 3:
        ap.error("--rounds: at least 3, so that the spread between runs shows")
    if not a.parent_root or not os.path.isdir(os.path.join(a.parent_root, "kleenexlang_amd")):
        ap.error("--parent-root: a built checkout of the parent commit is required; a figure without the parent's on the same device says nothing")
    variants = [("unquote", ROOT), ("parent", a.parent_root)]
    res ={"lines": a.lines, "reps": a.reps, "rounds": a.rounds, "clocks": clocks(), "runs": {name: [] for name, _ in variants}}
    for _ in range(a.rounds):                                             # the two alternate, each run a fresh process
        for name, root in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--package-root", root, "--lines", str(a.lines), "--reps", str(a.reps),
                   "--seed", str(a.seed)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=1800)
            if p.returncode:
                raise SystemExit("%s: exit status %d" % (name, p.returncode))
            res["runs"][name].append(json.loads(p.stdout.decode().splitlines()[-1]))
    res["spread_of_medians"] = {name: {k: med([r[k]["median"] for r in runs]) for k in ("wall_ms", "split_ms", "batch_ms")}
                                for name, runs in res["runs"].items()}
    line = json.dumps(res)
    print(line)
    with open(a.json, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
