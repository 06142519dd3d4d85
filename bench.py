#!/usr/bin/env python3
"""bench.py — BASELINE.json's metric on MI355X: input GB/s of apache_log.kex over a synthetic
Apache log that is already resident in HBM, with the kernel roofline and a CPU baseline beside it.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--gib G] [--program P] [--dump-outputs DIR]
  N > 1: either launched as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N … bench.py --gpus N …`
  (RANK/LOCAL_RANK/WORLD_SIZE in the environment) or plainly as `python bench.py --gpus N`, which re-executes
  itself under torch.distributed.run with N ranks on 127.0.0.1.

A "step" is one full pass of the hot path (all engine kernels, every pipeline stage) over the
rank's shard.  Weak scaling: every rank owns `--gib` GiB of the global log (cut mid-line); the only
cross-rank traffic is the boundary hand-off (kleenexlang_amd/sharded.py) over RCCL.
Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; ≈6.3 TB/s achievable)
HBM_ACHIEVABLE_GBPS = 6300.0


def counter_ceilings(program, kernels, n_cus=256):
    """Ceilings that follow from the engine's own instruction and LDS-pipe counts — read from an SQ-counter file taken with THIS engine
    build (profiles/*sq_counters*.json stamped with build.engine_sha() by profiles/collect_sq_df.sh); None when there is no such file
    (round 5 printed literals here).  Per kernel of `kernels`, per input byte of the counter run:
      issue:  (SQ_INSTS_VALU + SQ_INSTS_LDS) wave-instructions x 4 cycles on one of 4 x n_cus SIMDs (a SIMD issues one vector instruction
              every 4 cycles whatever the wave),
      lds:    SQ_LDS_IDX_ACTIVE cycles of one of n_cus LDS pipes,
    both at the shader clock of the counter run (GRBM_GUI_ACTIVE / kernel time is not in the file: 2.4 GHz nominal is used)."""
    import glob
    from kleenexlang_amd import build as kbuild
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*sq_counters*.json")), reverse=True):
        try:
            j = json.load(open(f))
        except Exception:   # noqa: BLE001
            continue
        if j.get("engine_sha") != kbuild.engine_sha() or j.get("program", "apache_log") != program or not j.get("input_bytes"):
            continue
        ks = [k for k in kernels if k in j["kernels"]]
        if not ks:
            continue
        nb, clk = float(j["input_bytes"]), 2.4e9
        issue_s = sum((j["kernels"][k]["SQ_INSTS_VALU"] + j["kernels"][k]["SQ_INSTS_LDS"]) * 4.0 / (4 * n_cus) for k in ks) / clk
        lds_s = sum(j["kernels"][k]["SQ_LDS_IDX_ACTIVE"] / n_cus for k in ks) / clk
        return {"issue_bound_frac": round(nb / issue_s / 1e9 / HBM_PEAK_GBPS, 4), "lds_pipe_bound_frac": round(nb / lds_s / 1e9 / HBM_PEAK_GBPS, 4),
                "kernels": ks, "source": os.path.basename(f)}
    return None


def gpu_clocks():
    """sclk / mclk / power of device 0 as rocm-smi reports them (explains the boxes that run every kernel 1.3-1.5x slower); None if the
    tool is missing or silent."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--showperflevel", "--json"], stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, timeout=20)
        j = json.loads(r.stdout.decode() or "{}")
        card = next(iter(j.values())) if j else {}
        keep = {k: v for k, v in card.items() if any(t in k.lower() for t in ("sclk", "mclk", "fclk", "power", "performance"))}
        return keep or None
    except Exception:   # noqa: BLE001
        return None


def cpu_baseline(program, base, sample_bytes):
    """Time the reference CPU path on a bounded sample of the same workload, the reference's way:
    `BIN -t < file > /dev/null`, wall ms from the binary's own stderr line (bench/runningtime.sh:32)."""
    from oracle import oracle
    kind, exe = "own-codegen+ref-crt", oracle.ref_binary(program, 3)
    if exe is None:  # no prebuilt reference-runtime binary: build generated C against the restated runtime
        kind = "port"
        from kleenexlang_amd import build, program_path
        exe = os.path.join(tempfile.gettempdir(), "kx_cpu_%s" % program)
        subprocess.check_call([os.path.join(build.OUT, "kexc"), "compile", "--quiet", "--backend=c", "--crt-dir",
                               os.path.join(ROOT, "oracle", "crt_port"), program_path(program), "--out", exe])
    k = max(1, sample_bytes // len(base))
    with tempfile.NamedTemporaryFile(prefix="kx_cpu_in_", delete=False) as f:
        for _ in range(k):
            f.write(base)
        path = f.name
    try:
        best = None
        for _ in range(2):
            with open(path, "rb") as fin, open(os.devnull, "wb") as devnull:
                env = {k: v for k, v in os.environ.items() if not (k.startswith("ROCP") or k in ("LD_PRELOAD", "HSA_TOOLS_LIB"))}
                r = subprocess.run([exe, "-t"], stdin=fin, stdout=devnull, stderr=subprocess.PIPE, check=True, env=env)
            ms = int(re.findall(r"\(ms\):\s*(\d+)", r.stderr.decode())[-1])
            best = ms if best is None else min(best, ms)
        nbytes = k * len(base)
        return {"value": round(nbytes / 1e9 / (best / 1e3), 4), "unit": "GB/s", "cores": 1, "kind": kind,
                "sample": "%d B (base chunk ×%d) of the same synthetic log through `%s -t < file > /dev/null`, best of 2; "
                          "generated C (kexc --backend=c --opt 3, reference shape) + %s"
                          % (nbytes, k, os.path.basename(exe),
                             "the reference's own crt/crt.c (the reference's literal generated C needs GHC and does not exist here)" if kind != "port" else "restated runtime oracle/crt_port/crt.c")}
    finally:
        os.unlink(path)


DUMP_SAMPLE = 1 << 22   # output bytes --dump-outputs keeps over ALL ranks: 4 B (float32 value) + 8 B (float64 position) each, 48 MiB in all
DUMP_SEED = 0x4B4C4558


def dump_outputs(d, out, olen, m, suffix=""):
    """What a caller of the timed path receives from one step — the output length and the output bytes — as .npy files in `d`:
      output_length.npy      float64 [1]   bytes written
      output_bytes.npy       float32 [k]   byte values (0-255) at the positions below
      output_positions.npy   float64 [k]   their offsets in the output: 0 .. olen-1 when olen <= m (k = olen), else k = m distinct
                                           sorted offsets, one drawn with a fixed seed from each of m equal strata of [0, olen)
    m is the rank's share of DUMP_SAMPLE.  Two builds that give the same input the same output write identical files."""
    import numpy as np
    import torch
    os.makedirs(d, exist_ok=True)
    if olen <= m:
        pos = torch.arange(olen, dtype=torch.int64)
    else:   # stratum i = [i*olen // m, (i+1)*olen // m) is at least olen // m >= 1 bytes wide: the offsets are distinct and < olen
        g = torch.Generator().manual_seed(DUMP_SEED)
        pos = torch.arange(m, dtype=torch.int64) * olen // m + torch.randint(0, olen // m, (m,), generator=g, dtype=torch.int64)
    vals = out[pos.to(out.device)].cpu()      # (every position < olen <= out.numel())
    np.save(os.path.join(d, "output_length%s.npy" % suffix), np.array([olen], dtype=np.float64))
    np.save(os.path.join(d, "output_bytes%s.npy" % suffix), vals.numpy().astype(np.float32))
    np.save(os.path.join(d, "output_positions%s.npy" % suffix), pos.numpy().astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gib", type=float, default=10.0, help="input GiB per GPU")
    ap.add_argument("--program", default="apache_log")
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--block-threads", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--escapes", type=int, default=0, help="(apache_log, 1 GPU) overwrite 7 bytes in that many evenly spaced request fields with "
                                                            "\\\"   5x — a context that two symbols do not decide (an escaped quote); the output is then "
                                                            "checked against the general engine's on the same input instead of the tiled oracle output")
    ap.add_argument("--force-dist", action="store_true", help="use the sharded protocol even with one rank")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for the boundary hand-off")
    ap.add_argument("--single-device", action="store_true", help="(validation) put every rank on cuda:0")
    ap.add_argument("--py-driver", action="store_true", help="boundary hand-off driven from Python over torch.distributed (kleenexlang_amd/sharded.py) "
                                                               "instead of the library's own driver (kx_run_sharded + RCCL communicator)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (DIR/<name>_rank<r>.npy with several ranks): "
                         "the output length and the output bytes with their positions — all of them when a rank's output fits its share "
                         "(%d / ranks), else a fixed seeded sample of that many; 48 MiB in all over every rank; see dump_outputs()" % DUMP_SAMPLE)
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become N ranks (one per GPU) under torch.distributed.run
        import socket
        sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
        os.execv(sys.executable, [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
                                  "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:])

    import torch
    from kleenexlang_amd import Program, compile_file, sharded, workloads
    from oracle import oracle

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the engine has no CPU path")
    if a.single_device:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    use_dist = world > 1 or a.force_dist
    if use_dist:
        if a.single_device and world > 1 and a.backend == "nccl":
            # RCCL refuses two ranks on one device ("Duplicate GPU detected") by comparing (host hash, PCI bus id).  A 1-GPU
            # box can still run the N-rank hand-off through RCCL when every rank claims its own host id: RCCL then treats
            # the ranks as N single-GPU nodes and carries the (≤ 300-byte) all-gathers over its socket transport on lo.
            os.environ["NCCL_HOSTID"] = "kx-single-device-rank-%d" % rank
            os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
            os.environ.setdefault("NCCL_IB_DISABLE", "1")
        import torch.distributed as dist
        # (RCCL prints a version banner on stdout when a communicator comes up; stdout must carry the one JSON line only)
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if a.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(a.backend, rank=rank, world_size=world)
    comm_dev = dev if a.backend == "nccl" else "cpu"
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    if not a.single_device and torch.cuda.device_count() < world and world > 1:
        raise SystemExit("bench.py: %d ranks but %d visible GPUs (use --single-device to stack ranks on cuda:0 for validation)"
                         % (world, torch.cuda.device_count()))

    blob = compile_file(a.program)
    prog = Program(blob, segment_bytes=a.segment, block_threads=a.block_threads, collect_timing=True)
    shape = workloads.PROGRAM_INPUT[a.program]
    per_gpu = int(a.gib * (1 << 30))
    base = workloads.generate(shape, min(32 << 20, per_gpu), seed=0x4B4C4558)
    tb = torch.frombuffer(bytearray(base), dtype=torch.uint8).to(dev)
    if world == 1:
        k = max(1, per_gpu // len(base))
        t = tb.repeat(k)
        n_local, n_global = t.numel(), t.numel()
    else:  # global log = base × K, cut into `world` shards at 4 KiB multiples (i.e. mid-line)
        K = max(1, per_gpu // len(base)) * world
        n_global = K * len(base)
        L = (n_global // world) // 4096 * 4096
        start = rank * L
        n_local = L if rank < world - 1 else n_global - start
        off = start % len(base)
        reps = (off + n_local + len(base) - 1) // len(base)
        t = tb.repeat(reps)[off:off + n_local].clone()   # fresh (16-byte aligned) allocation holding exactly the shard
    n_escapes = 0
    if a.escapes and world == 1 and a.program == "apache_log":
        pat = torch.tensor(list(b'\\"   5x'), dtype=torch.uint8, device=dev)
        for i in range(a.escapes):
            at = int((i + 0.5) * n_local / a.escapes)
            win = bytes(t[at:at + 4096].cpu().numpy().tobytes())
            k = win.find(b' HTTP/')
            if k >= 16 and b'"' not in win[k - 8:k] and b' ' not in win[k - 8:k]:
                t[at + k - 7:at + k] = pat
                n_escapes += 1
    expansion = {"apache_log": 1.30, "csv2json": 2.05, "iso_datetime_to_json": 4.35, "thousand_sep": 1.40}[a.program]
    out = torch.empty(int(n_local * expansion) + (1 << 20), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    totals = {"out": None, "off": 0, "boundary_ms": 0.0}
    comm = None
    if use_dist and not a.py_driver:
        # the library's own communicator: rank 0 makes the id, torch.distributed only carries it to the other ranks
        from kleenexlang_amd.host import Comm
        ids = [Comm.unique_id() if rank == 0 and world > 1 else None]
        if world > 1:
            dist.broadcast_object_list(ids, src=0)
        comm = Comm(rank, world, ids[0])
    if use_dist:
        dist.barrier()   # (bring the communicators up before stdout is given back)
        sys.stdout.flush()
        import ctypes
        ctypes.CDLL(None).fflush(None)   # (the banner sits in C stdio's buffer)
        os.dup2(saved_stdout, 1)
        os.close(saved_stdout)

    def step():
        if not use_dist:
            return prog.run_device(t.data_ptr(), n_local, out.data_ptr(), out.numel(), stream)
        if comm is not None:   # kx_run_sharded: every stage, the hand-off inside the library
            res = prog.run_sharded(rank, world, comm, t.data_ptr(), n_local, out.data_ptr(), out.numel(), stream)
            prog.last_stats = res.stats
            totals["out"], totals["off"] = int(res.total_out), int(res.out_offset)
            totals["boundary_ms"] += float(res.boundary_ms)
            return int(res.out_len)
        sh = prog.shard_begin(0, t.data_ptr(), n_local, rank == 0, rank == world - 1, stream)
        res = sharded.raise_on_fail(sharded.run_stage_dist(sh, n_local, comm_dev))
        sh.emit(out.data_ptr(), out.numel())
        prog.last_stats = sh.stats()
        sh.end()
        totals["out"], totals["off"] = res[3], res[2]
        return res[1]

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # (rocm-smi is a subprocess of about a second: sampled BEFORE the warm-up — between warm-up and the timed steps it would hand the
    #  first timed step an idle device at its low clock)
    clocks_before = gpu_clocks() if rank == 0 else None
    for _ in range(a.warmup):
        step()
    fence()
    kern = {}
    step_ms = []          # wall time of every step (a step blocks until its output is complete: no extra synchronisation)
    totals["boundary_ms"] = 0.0
    t0 = time.perf_counter()
    tprev = t0
    for _ in range(a.steps):
        olen = step()
        tnow = time.perf_counter()
        step_ms.append((tnow - tprev) * 1e3)
        tprev = tnow
        for kname, ms in prog.last_stats.as_dict()["kernel_ms"].items():
            kern[kname] = kern.get(kname, 0.0) + ms
    fence()
    dt = time.perf_counter() - t0
    clocks_after = gpu_clocks() if rank == 0 else None
    if dist is not None:
        tmax = torch.tensor([dt], dtype=torch.float64, device=comm_dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    if a.dump_outputs:   # (`out` still holds the last timed step's output; each rank writes its own slice)
        dump_outputs(a.dump_outputs, out, olen, DUMP_SAMPLE // world, "_rank%d" % rank if world > 1 else "")

    # Bit-exact check of EVERY output byte, outside the timed region and on the device: the expected stream of
    # the replicated input is (prefix, unit × reps, suffix) built from the CPU oracle's output on ONE base chunk
    # (workloads.tiled_parts); each rank compares its slice [out_offset, out_offset + out_len) of that stream.
    want = oracle.run(blob, base)
    parts = workloads.tiled_parts(a.program, want, n_global // len(base))
    my_off = totals["off"] if use_dist else 0
    if n_escapes:
        # the input is no longer the tiled chunk: the reference is the general engine's output on the same device buffer (that engine is
        # checked against the oracle byte for byte by the tests and by every run of this script without --escapes)
        from kleenexlang_amd import host as khost
        ref_prog = Program(blob, config=khost.config_from_env(delayed_form=1))
        ref = torch.empty_like(out)
        rlen = ref_prog.run_device(t.data_ptr(), n_local, ref.data_ptr(), ref.numel(), stream)
        torch.cuda.synchronize()
        ok = rlen == olen and bool(torch.equal(out[:olen], ref[:rlen]))
        del ref
        ref_prog.close()
    else:
        ok = workloads.check_tiled_on_device(out[:olen], my_off, parts)
    checked = olen
    total_out = totals["out"] if use_dist else olen
    if dist is not None:
        agg = torch.tensor([1 if ok else 0, checked], dtype=torch.int64, device=comm_dev)
        okt = agg[:1].clone(); dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        cnt = agg[1:].clone(); dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
        ok, checked = bool(int(okt.item())), int(cnt.item())
    ok = bool(ok) and (n_escapes > 0 or total_out == workloads.tiled_total(parts)) and checked == total_out

    if rank == 0:
        ms_step = dt / a.steps * 1e3
        value = n_global * a.steps / dt / 1e9
        kern = {k: v / a.steps for k, v in kern.items()}
        dom = max(kern, key=kern.get)
        ratio = olen / float(n_local)
        ksum = sum(kern.values())
        # which engine ran: the delayed form (round 5: one forward pass + one fused placing walk, kernels k_dforward / k_dlen / k_demit)
        # or the general engine (forward, backward, sweep: k_forward / k_backlen / k_resolve.. / k_emit)
        df_state = prog.stage_delayed_form(0)
        delayed = df_state == 1
        kname = ({"forward": "k_dforward", "resolve": "k_dlen", "emit": "k_demit"}.get(dom, "k_" + dom)) if delayed else "k_" + dom
        # algorithmic bytes = 1 B read per input byte; `achieved` = input bytes of one launch ÷ the dominant
        # kernel's mean launch duration (HIP events on the engine's stream, recorded by the engine around each kernel).
        achieved = n_local / (kern[dom] / 1e3) / 1e9 if kern[dom] > 0 else 0.0
        # the same kernel's own traffic (what it must read and write per input byte) — NOT the roofline fraction
        alg = {"sync": 0.0, "forward": 1.0, "head": 0.0, "backlen": 1.0, "resolve": 0.0, "emit": 1.0 + ratio}
        if delayed:   # (16-byte piece records per 64 input bytes: written by the forward pass, read by the placing walk)
            alg = {"sync": 0.0, "forward": 1.25, "head": 0.0, "backlen": 0.0, "resolve": 0.0, "emit": 1.25 + ratio}
        traffic, traffic_note = None, "no PMC passes for this build"
        try:   # HBM bytes per launch of the dominant kernel from the PMC passes — only if they were taken with THIS engine build
            import glob
            from kleenexlang_amd import build as kbuild
            for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*traffic.json")), reverse=True):
                tj = json.load(open(f))
                if tj.get("engine_sha") == kbuild.engine_sha() and tj.get("program", "apache_log") == a.program and abs(tj["input_bytes"] - n_local) < (1 << 20):
                    traffic = tj["per_launch"][kname]["total"]
                    traffic_note = os.path.basename(f)
                    break
        except Exception as e:   # noqa: BLE001
            traffic_note = "unreadable: %s" % e
        line = {
            "metric": "input GB/s + % HBM-read roofline, apache_log.kex over 10 GiB synthetic log",
            "value": round(value, 3), "unit": "GB/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_step, 3), "ms_per_step_median": round(sorted(step_ms)[len(step_ms) // 2], 3),
            "ms_per_step_min_max": [round(min(step_ms), 3), round(max(step_ms), 3)], "ms_of_each_step": [round(x, 3) for x in step_ms[:64]],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": "%s.kex, %.2f GiB synthetic %s per GPU (seeded 32 MiB chunk replicated, "
                                   "shards cut mid-line), input and output resident in HBM" % (a.program, n_local / 2**30, shape),
                       "input_bytes_per_gpu": n_local, "output_bytes_rank0": olen, "output_bytes_total": total_out,
                       "segment_bytes": a.segment or "auto (one round of lanes: input / (CUs x 1024), 4-64 KiB)",
                       "engine": ("delayed form (forward transducer with fixed delay, no backward pass; DESIGN.md §2e)" if delayed else
                                  "general (forward, backward, sweep)" + (" after the delayed form met an undecided context" if df_state == 2 else
                                                                           " (the delayed form was given up: the input leaves it in nearly every segment)" if df_state == 3 else "")),
                       "parallelism": "shard%d" % world, "boundary_backend": (a.backend if use_dist else None),
                       "boundary_driver": (None if not use_dist else "python (sharded.py over torch.distributed)" if a.py_driver else "kx_run_sharded (C, own RCCL communicator)"),
                       "boundary_ms_per_step_rank0": (round(totals["boundary_ms"] / a.steps, 4) if comm is not None else None),
                       "single_device_validation": bool(a.single_device)},
            "roofline": {"bound": "hbm", "kernel": kname, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 5), "traffic": traffic, "traffic_source": traffic_note,
                         "algorithmic_bytes_per_input_byte": 1.0},
            # How far `frac` is from what is possible: a perfect single-pass engine moves 1 B in + r B out per input
            # byte over a bus that sustains ≈ 6.3 TB/s in mixed traffic; this three-pass design moves 3 + r + 3/16 B.  Both are
            # bounds of the WHOLE PATH (compare `whole_path.frac_of_hbm_peak`), stated as fractions of the 8 TB/s read roofline.
            "ceilings": {"out_over_in": round(ratio, 4),
                         "single_pass_hbm_bound_frac": round(HBM_ACHIEVABLE_GBPS / (1.0 + ratio) / HBM_PEAK_GBPS, 4),
                         "this_design_hbm_bound_frac": round(HBM_ACHIEVABLE_GBPS / ((2.5 if delayed else 3.0 + 3.0 / 16.0) + ratio) / HBM_PEAK_GBPS, 4),
                         "from_counters": counter_ceilings(a.program, ["k_dforward", "k_demit"] if delayed else ["k_forward", "k_backlen", "k_emit"]),
                         "note": "fractions of 8 TB/s; north_star's 40 % is above the single-pass HBM bound for this output ratio; this design reads the "
                                 "input twice (delayed form; three times on the general engine) plus its piece records; from_counters: what the engine's "
                                 "own vector-instruction count and LDS-pipe cycles allow (SQ counters of a profile run of THIS engine build, DESIGN.md §4); "
                                 "null when no such run is committed"},
            "whole_path": {"input_GBps_over_kernel_time": round(n_local / (ksum / 1e3) / 1e9, 2) if ksum else None,
                           "frac_of_hbm_peak": round(n_local / (ksum / 1e3) / 1e9 / HBM_PEAK_GBPS, 5) if ksum else None},
            "dominant_kernel_own_traffic": {"bytes_per_input_byte": round(alg[dom], 4),
                                            "GBps": round(alg[dom] * n_local / (kern[dom] / 1e3) / 1e9, 2) if kern[dom] > 0 else None,
                                            "frac_of_hbm_peak": round(alg[dom] * n_local / (kern[dom] / 1e3) / 1e9 / HBM_PEAK_GBPS, 5) if kern[dom] > 0 else None},
            "kernels_ms": {k: round(v, 4) for k, v in kern.items()},
            "clocks": {"before_warmup": clocks_before, "after": clocks_after, "source": "rocm-smi -d 0 --showclocks --showpower --showperflevel --json"},
            "output_checked_bit_exact": ok, "output_bytes_checked": checked,
            "escaped_quotes_injected": n_escapes, "checked_against": ("general engine on the same input" if n_escapes else "CPU oracle (tiled)"),
            "delayed_form_state_after": df_state,
        }
        if not a.no_cpu and world == 1:
            line["cpu_baseline"] = cpu_baseline(a.program, base, 1 << 30)
        elif not a.no_cpu:
            line["cpu_baseline"] = None
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if not ok and not os.environ.get("KX_DEBUG_FLAGS"):   # a wrong output is a failure, not a JSON field (ablation runs excepted)
        sys.stderr.write("bench.py: output differs from the oracle's\n")
        sys.exit(1)


if __name__ == "__main__":
    main()
