"""Record mode's framing (`BIN --records … --chomp --ors=STR`, kx_run_batch_framed) against the plain run.  One JSON line on stdout
(and appended to --json).  The same 2^20 seeded CSV lines go through

  plain    --records: the program consumes the newline itself and writes one ("fields" below WITH its newline handling),
           kx_run_batch / kx_run_records_fd
  chomp    --records --chomp --ors='\\n': the same program minus its newline handling, kx_run_batch_framed (trim 1, suffix "\\n") /
           kx_run_records_fd_opts

and both outputs must be the same bytes.  Two measurements each, median / min / max of --reps after one warm-up:

  batch    the batch call alone: the lines resident on the device, the offsets split once, the output buffer given
  fd       the whole stream: a file in, a file out (reader and writer threads, split, batch)

On an engine library without kx_run_batch_framed (the parent commit) only the plain runs are made: that is how the parent's time
for the plain run is taken, with this script and that commit's package on the path (--package-root).

  python profiles/records_chomp_bench.py --json profiles/records_chomp_bench.json
  python profiles/records_chomp_bench.py --package-root PARENT_CHECKOUT --json profiles/records_chomp_bench.json"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = 'main := f (~/,/ " | " f)* /\\n/\nf := "<" /[a-z]*/ ">"\n'
CHOMP = 'main := f (~/,/ " | " f)*\nf := "<" /[a-z]*/ ">"\n'


def csv_lines(nlines, seed):
    r = random.Random(seed)
    word = lambda: bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(1, 12)))   # noqa: E731
    pool = [b",".join(word() for _ in range(r.randrange(2, 8))) + b"\n" for _ in range(8192)]
    return b"".join(r.choice(pool) for _ in range(nlines))


def times(f, reps):
    import torch
    f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=29)
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose kleenexlang_amd package (and engine library) is measured")
    ap.add_argument("--label", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import torch
    from kleenexlang_amd import host
    framed = hasattr(host, "KxBatchFrame")
    data = csv_lines(a.lines, a.seed)
    v = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    offs = host.split_records_tensor(v, b"\n")
    assert offs.numel() == a.lines + 1
    out = torch.empty(len(data) * 4, dtype=torch.uint8, device="cuda")
    res = {"label": a.label or ("this commit" if framed else "without kx_run_batch_framed"), "lines": a.lines, "in_bytes": len(data)}
    outputs = {}
    cases = [("plain", PLAIN, {})] + ([("chomp", CHOMP, {"trim": 1, "suffix": b"\n"})] if framed else [])
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "in")
        with open(src, "wb") as f:
            f.write(data)
        for name, source, frame in cases:
            prog = host.Program(host.compile_source(source))

            def batch():
                outputs[name] = prog.run_batch_tensor(v, offs, out=out, **frame)

            def fd():
                fi, fo = os.open(src, os.O_RDONLY), os.open(os.path.join(d, "out_" + name), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
                try:
                    st = prog.run_records_fd(fi, fo, **({"chomp": True, "ors": b"\n"} if frame else {}))
                finally:
                    os.close(fi)
                    os.close(fo)
                assert st["records"] == a.lines and not st["rejected"], st
            res[name] = {"batch": times(batch, a.reps), "fd": times(fd, a.reps)}
            o, ooff, status = outputs[name][:3]
            assert int(status.sum()) == 0
            res[name]["out_bytes"] = int(ooff[-1])
            outputs[name] = o.cpu().numpy().tobytes()
            with open(os.path.join(d, "out_" + name), "rb") as f:
                assert f.read() == outputs[name]
    if framed:
        assert outputs["plain"] == outputs["chomp"]
        for k in ("batch", "fd"):
            res["chomp_over_plain_" + k] = res["chomp"][k]["ms_median"] / res["plain"][k]["ms_median"]
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
