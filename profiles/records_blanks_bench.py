"""Field mode on words (`BIN --records --field=LIST --blanks`, kx_run_batch_field_words) against field mode with `--fs=' '`
(kx_run_batch_field_list) on the SAME single-spaced data: 2^20 lines of six words, `word stamp word stamp stamp stamp\\n` with ISO
date-times, through the `stamp` rule of programs/iso_datetime_to_json.kex (the lines of profiles/records_field_list_bench.py with a
space for the comma).  On such lines the two paths select the same bytes, so the outputs are the same and only the count and
locate kernels differ.  The batch call alone, device tensors in and a preallocated output: no file, no split.  One JSON line on
stdout (and appended to --json):

  blanks_1, blanks_2, blanks_4   kx_run_batch_field_words with the lists 2 / 2,4 / 2,4-6: milliseconds per call (median / min / max
                                 of --reps calls after one warm-up), GB/s of input bytes, and the HIP-event times of field mode's
                                 own kernel groups (kx_fields_stats; count and locate are both in locate_ms)
  fs_1, fs_2, fs_4               kx_run_batch_field_list with fs = ' ' and the same lists: the yardstick
  locate_ratio                   per list, locate_ms of the words path over locate_ms of the fs path (medians)

No target is fixed: the fs path's locate time is the yardstick.  Every output is compared with the expected bytes, spelled out by
hand from the lines.  The device's clocks as rocm-smi reports them are noted next to the numbers (read only; nothing is set).

  python profiles/records_blanks_bench.py --json profiles/records_blanks_bench.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from records_field_bench import clocks, med, stamp_program   # noqa: E402
from records_field_list_bench import csv_lines   # noqa: E402


def want_line(line, columns):
    """What either path must write for a pool line: the stamp rule's output in the selected words, spelled out by hand (it holds
    blanks of its own: nothing re-reads the record)."""
    cols = line[:-1].split(b" ")
    for k in columns:
        t = cols[k - 1]
        cols[k - 1] = b"{'year'='%s', 'month'='%s', 'day'='%s', 'hours'='%s', 'minutes'='%s', 'seconds'='%s', 'tz'='%s'}" % (
            t[0:4], t[5:7], t[8:10], t[11:13], t[14:16], t[17:19], t[19:])
    return b" ".join(cols) + b"\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=37)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from kleenexlang_amd import host
    pool, picks = csv_lines(a.lines, a.seed)                               # (no word and no stamp holds a comma or a blank)
    spaced = [p.replace(b",", b" ") for p in pool]
    data = b"".join(spaced[i] for i in picks)
    plen = np.array([len(p) for p in pool], dtype=np.int64)
    offs = np.concatenate(([0], np.cumsum(plen[np.array(picks)])))
    v = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    o = torch.from_numpy(offs).cuda()
    prog = host.Program(host.compile_source(stamp_program()), collect_timing=True)
    res = {"lines": a.lines, "in_bytes": len(data), "reps": a.reps, "clocks": clocks()}

    def measure(name, columns, call):
        want = [want_line(p, columns) for p in spaced]
        need = sum(len(want[i]) for i in picks)
        out = torch.empty(need, dtype=torch.uint8, device="cuda")
        ms, own = [], []
        for rep in range(a.reps + 1):                                     # (the first call is the warm-up)
            before = prog.fields_kernel_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call(out)
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) * 1e3
            after = prog.fields_kernel_stats()
            assert r[0].numel() == need and int(r[2].max()) == 0, name
            if rep:
                ms.append(t)
                own.append({k: after[k] - before[k] for k in ("locate_ms", "gather_ms", "scan_ms", "splice_ms")})
        assert out.cpu().numpy().tobytes() == b"".join(want[i] for i in picks), "%s: the output differs from the expected bytes" % name
        m = statistics.median(ms)
        res[name] = {"columns": columns, "out_bytes": need, "ms": med(ms), "in_gbps": len(data) / m / 1e6,
                     "own_kernels": {k: med([x[k] for x in own]) for k in own[0]}}

    res["locate_ratio"] = {}
    for tag, text, columns in (("1", "2", [2]), ("2", "2,4", [2, 4]), ("4", "2,4-6", [2, 4, 5, 6])):
        ranges = host.parse_field_list(text)
        measure("blanks_" + tag, columns, lambda out, ranges=ranges: prog.run_batch_field_words_tensor(v, o, ranges, sep_len=1, out=out))
        measure("fs_" + tag, columns, lambda out, ranges=ranges: prog.run_batch_field_list_tensor(v, o, ranges, fs=b" ", sep_len=1, out=out))
        loc = lambda name: res[name]["own_kernels"]["locate_ms"]["median"]   # noqa: E731
        res["locate_ratio"][text] = loc("blanks_" + tag) / loc("fs_" + tag) if loc("fs_" + tag) else None
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
