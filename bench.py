#!/usr/bin/env python3
"""Headline benchmark: poses/sec of the flower-pose hot path on N MI355X (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dtype f16|bf16] [--crop 224] [--batch 256]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

(`--steps 32` -- or `--cfg4` -- with `--gpus 8` is exactly BASELINE configs[3]: 8 x 32 x 256 = 65,536 crops.)

One step = one pass of the hot path over one batch: 256 synthetic 224x224x3 crops, 16-bit
NHWC, already resident in HBM -> PoseResNet trunk (MFMA convs) -> fp32 head -> special
Procrustes -> yaw-null + 4x4 pose assembly (BASELINE configs[1]).  Ranks own independent
batches (weak scaling, no collective on the data path); the finished [K*256,16] pose records
are all-gathered ONCE over RCCL inside the timed region (BASELINE configs[3]).  Rank 0 prints
one JSON line.

The timed loop is un-instrumented.  A plain run does only what the headline needs: set-up
(engine, weights, schedule autotune), W warm-up steps, the K timed steps, the optional output
dump and the result line.  Everything else is measured only with `--full`: the per-step event
times, the `roofline` object (a second pass of the same steps in the engine's profile mode, HIP
events around every launch on the launch stream), the parity sample against the oracle, the
other dtype and the 512 x 512 crop, the fresh-process run without autotune, and the
`cpu_baseline` object (the CPU oracle, torch fp32, eval mode, timed on the host cores on a
bounded sample -- a reported baseline, never part of the product path).

`--dump-outputs DIR` writes, after the timed steps, what the last timed step computed as float32
`.npy` files: `poses.npy` ([N*B,16] pose records of every rank, as gathered on rank 0) and
`R.npy` (rank 0's [B,9] rotations).  Inputs and weights are seeded, so equal arguments give
equal inputs from run to run.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 2500.0      # dense bf16/f16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md


def source_digest() -> str:
    """sha256 over the kernel sources of the benched path (everything in csrc except the detector's and the encoder's files,
    which the bench workload never launches): ties a committed PMC traffic figure to a build."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "flope_amd", "csrc", "*.h*"))):
        if os.path.basename(f).startswith(("yolo", "tf_encoder")):
            continue
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def cpu_baseline(crop: int, batch: int = 16, budget_s: float = 12.0):
    """Oracle forward + Procrustes on the host cores (B = 16 and B = 256)."""
    from flope_amd.weights import synthetic_state_dict
    from oracle import posenet_ref as O
    # the box's CPU share, not the host's core count: affinity mask, then the cgroup quota, and never more
    # than 16 threads when neither narrows it down (a 1-GPU box owns 16 of the host's cores)
    threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            threads = min(threads, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    if threads > 32:
        threads = 16
    torch.set_num_threads(threads)
    sd = synthetic_state_dict(0)
    torch.manual_seed(0)
    x = torch.rand(batch, 3, crop, crop)
    with torch.no_grad():
        for _ in range(2 if batch <= 16 else 1):
            O.procrustes_to_rotmat(O.forward(sd, x))
        times = []
        t_end = time.perf_counter() + budget_s
        while len(times) < 3 or (time.perf_counter() < t_end and len(times) < 40):
            t0 = time.perf_counter()
            O.procrustes_to_rotmat(O.forward(sd, x))
            times.append(time.perf_counter() - t0)
    times.sort()
    med = times[len(times) // 2]
    return {"value": round(batch / med, 2), "unit": "poses/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{len(times)} x ({batch} crops {crop}x{crop} fp32, torch CPU eval-mode oracle + SVD Procrustes), median"}


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` without an outer launcher: start `python -m torch.distributed.run` (one rank per GPU) as a CHILD
    process -- before this process has touched the GPU, and never by exec -- relay rank 0's JSON line and return the child's code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith('{"metric"'):
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line, flush=True)
    elif proc.returncode == 0:
        print("bench.py: the launched ranks printed no result line", file=sys.stderr)
        return 1
    return proc.returncode


def no_autotune_child(args) -> dict | None:
    """The same run in a fresh process with the engine's default schedule and no set-up measurement (the tuned number
    next to the untuned one -- most of r04's gain was the device reaching its sustained clock during autotune, not the schedule)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--dtype", args.dtype, "--crop", str(args.crop), "--batch", str(args.batch), "--full", "--no-autotune", "--no-alt",
           "--no-cpu-baseline"]
    try:
        proc = subprocess.run(cmd, env=dict(os.environ, FLOPE_BENCH_CHILD="1"), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                              text=True, timeout=300)
        for ln in proc.stdout.splitlines():
            if ln.startswith('{"metric"'):
                j = json.loads(ln)
                return {"value": j["value"], "ms_per_step": j["ms_per_step"], "ms_per_step_median": j.get("ms_per_step_median"),
                        "note": "fresh process, default schedule, no autotune; same steps / warm-up"}
    except (subprocess.SubprocessError, ValueError, KeyError, OSError):
        pass
    return None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """Each array as float32 `<out_dir>/<name>.npy`; past 64 MB in all, a fixed seeded sample of rows (in order) of every array."""
    import numpy as np
    arrs = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrs.values())
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrs.items():
        if total > DUMP_LIMIT_BYTES:
            keep = max(1, int(a.shape[0] * DUMP_LIMIT_BYTES // total))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default=os.environ.get("FLOPE_DTYPE", "f16"), choices=["f16", "bf16"])
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--cfg4", action="store_true",
                    help="BASELINE configs[3] exactly: 32 steps of 256 crops per GPU, i.e. 65,536 crops on --gpus 8 (same as --steps 32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-alt", action="store_true", help="skip the secondary bf16/f16 measurement")
    ap.add_argument("--no-autotune", action="store_true", help="keep the engine's default launch schedule (no set-up measurement)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: per-step and per-kernel times (roofline), parity sample "
                         "against the oracle, the other dtype, the 512 x 512 crop, the run without autotune and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs as float32 DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.cfg4:
        args.steps, args.batch, args.crop = 32, 256, 224
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:      # no outer launcher: become one (nothing has touched the GPU yet)
        raise SystemExit(self_launch(args.gpus))

    from flope_amd import distributed as D
    from flope_amd import engine as E
    from flope_amd.weights import synthetic_state_dict

    if not torch.cuda.is_available():
        raise SystemExit("bench.py: no HIP device visible (the product path has no CPU fallback)")
    # FLOPE_BENCH_REHEARSE=1: rehearse the N > 1 control flow on a box with ONE GPU (every rank on cuda:0, gloo instead
    # of RCCL, poses gathered through host memory).  Never used for reported numbers.
    rehearse = os.environ.get("FLOPE_BENCH_REHEARSE") == "1"
    rank, world, local = D.init_from_env("gloo" if rehearse else "nccl")
    if rehearse:
        local = 0
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with torch.distributed.run")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    B, S, K, W = args.batch, args.crop, args.steps, args.warmup
    sd = synthetic_state_dict(0)

    tuned = {}

    def build(dtype, S=S):
        eng = E.PoseEngine(S, S, B, dtype, device=dev)
        eng.load_state_dict(sd)
        tdt = torch.float16 if dtype == "f16" else torch.bfloat16
        g = torch.Generator().manual_seed(1234 + rank)          # per-rank synthetic crops
        x = torch.rand(B, S, S, 3, generator=g).to(tdt).to(dev)
        fmt = 2 if dtype == "f16" else 1
        # engine set-up, before the warm-up steps: the launch schedule for this device and batch is picked by measurement
        # (PoseEngine.autotune: bit-identical candidates, ~0.1 s) -- what a long-running server does once at start-up
        if not args.no_autotune:
            tuned[(dtype, S)] = eng.autotune(x, fmt)
        if os.environ.get("FLOPE_BENCH_SERIES") == "1":
            print(f"[{time.perf_counter():.4f}] build done", file=sys.stderr)
        return eng, x, fmt

    def run_steps(eng, x, fmt, n, poses, R, xyz):
        for i in range(n):
            # forward + Procrustes + yaw-null + [R|t] assembly (flope_forward_poses) straight into this step's slice of
            # the pose buffer; R is kept too (the parity sample below reads it)
            eng.forward_poses_into(x, fmt, xyz, True, poses[i % poses.shape[0]], R)

    def measure(dtype, S=S, K=K, W=W):
        # (buffers first: the first torch kernel of a process -- the fill behind torch.zeros -- loads a code module, ~20 ms of host
        # time during which an already tuned, warm GPU would sit idle)
        R = torch.empty(B, 9, device=dev)
        xyz = torch.zeros(B, 3, device=dev)                      # translation comes from depth (cfg3); zeros here
        poses = torch.empty(max(K, 1), B, 16, device=dev)
        torch.cuda.synchronize(dev)
        eng, x, fmt = build(dtype, S)
        run_steps(eng, x, fmt, W, poses, R, xyz)
        D.gather_poses(poses.view(K * B, 16).cpu() if rehearse else poses.view(K * B, 16))   # untimed: RCCL communicator / channel set-up
        D.barrier(); torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if os.environ.get("FLOPE_BENCH_SERIES") == "1":
            print(f"[{t0:.4f}] timed region starts", file=sys.stderr)
        if os.environ.get("FLOPE_BENCH_SERIES") == "1":        # diagnostic: the timed steps one by one (events on the launch stream)
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(K + 1)]
            evs[0].record()
            for i in range(K):
                run_steps(eng, x, fmt, 1, poses[i:i + 1], R, xyz); evs[i + 1].record()
            torch.cuda.synchronize(dev)
            print("timed steps (ms):", " ".join(f"{evs[i].elapsed_time(evs[i + 1]):.3f}" for i in range(K)), file=sys.stderr)
        else:
            run_steps(eng, x, fmt, K, poses, R, xyz)
        allp = D.gather_poses(poses.view(K * B, 16).cpu() if rehearse else poses.view(K * B, 16))
        D.barrier(); torch.cuda.synchronize(dev)
        dt = D.max_over_ranks(time.perf_counter() - t0, "cpu" if rehearse else dev)
        assert allp.shape == (world * K * B, 16)
        return eng, x, fmt, dt, R, xyz, poses, allp

    def step_times_ms(eng, x, fmt, n, poses, R, xyz):
        """Per-step GPU time: events on the launch stream around every step (the engine forks its slice streams from
        that stream and joins them back, so the pair brackets the whole step).  A second pass, after the timed one."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        for i in range(n):
            eng.forward_poses_into(x, fmt, xyz, True, poses[i % poses.shape[0]], R)
            ev[i + 1].record()
        torch.cuda.synchronize(dev)
        return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(n))

    def oracle_sample_err(eng, x, fmt, R):
        from oracle import posenet_ref as O
        xs = x[:8].float().permute(0, 3, 1, 2).cpu()
        Rref = O.procrustes_to_rotmat(O.forward(sd, xs))
        eng.forward_into(x, fmt, None, R)
        torch.cuda.synchronize(dev)
        return {"max_abs_R": float((R[:8].view(8, 3, 3).cpu() - Rref).abs().max()),
                "max_angle_deg": float(O.geodesic_deg(R[:8].view(8, 3, 3).cpu(), Rref).max()),
                "sample": "8 crops of the bench batch vs fp32 CPU oracle"}

    eng, x, fmt, dt, R, xyz, poses, allp = measure(args.dtype)
    value = world * K * B / dt
    if rank == 0 and args.dump_outputs:
        # the last timed step's [B,16] records of every rank (gathered rank-major) and rank 0's rotations, before --full reuses R
        dump_outputs(args.dump_outputs, {"poses": allp.view(world, K, B, 16)[:, K - 1].reshape(world * B, 16), "R": R})

    out = {
        "metric": "poses_per_sec", "value": round(value, 1), "unit": "poses/s", "n_gpus": world, "steps": K,
        "warmup": W, "ms_per_step": round(dt / K * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic" + (" (REHEARSAL: all ranks on one GPU, gloo)" if rehearse else ""),
        "config": {"workload": f"PoseResNet (ResNet-18 trunk + fp32 head) forward + special Procrustes + pose assembly, "
                               f"batch {B} x {S}x{S}x3 16-bit NHWC crops resident in HBM per GPU (BASELINE configs[1]); "
                               f"one RCCL all-gather of the poses per run when N>1 (configs[3])",
                   "batch_per_gpu": B, "global_batch": B * world, "crop": S, "parallelism": f"dp{world}",
                   "weights": "synthetic_state_dict(seed 0), eval-mode BN folded",
                   "gflop_per_pose": round(eng.flops(1) / 1e9, 4)},
    }
    if rank == 0 and (args.dtype, S) in tuned:
        out["autotune"] = tuned[(args.dtype, S)]

    if rank == 0 and args.full:
        st = step_times_ms(eng, x, fmt, K, poses, R, xyz)
        out["ms_per_step_median"] = round(st[len(st) // 2], 4)
        out["ms_per_step_min"] = round(st[0], 4)
        out["poses_per_sec_at_median_step"] = round(B / (st[len(st) // 2] * 1e-3), 1)
        # ---- roofline: per-launch HIP-event times of the same steps (profile mode) ------------------
        eng.set_option("profile", 1)
        info = eng.launch_info(B)
        acc = [0.0] * len(info)
        nprof = max(4, min(K, 16))
        run_steps(eng, x, fmt, 2, poses, R, xyz)
        for _ in range(nprof):
            run_steps(eng, x, fmt, 1, poses, R, xyz)
            for i, ms in enumerate(eng.profile_read()):
                acc[i] += ms
        eng.set_option("profile", 0)
        per_kernel = {}
        for (layer, kern, fl), ms in zip(info, acc):
            k = per_kernel.setdefault(kern, {"ms": 0.0, "flops": 0.0, "launches": 0})
            k["ms"] += ms / nprof; k["flops"] += fl; k["launches"] += 1
        dom = max(per_kernel, key=lambda k: per_kernel[k]["ms"])
        d = per_kernel[dom]
        achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12
        out["roofline"] = {"bound": "mfma", "achieved": round(achieved, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                           "frac": round(achieved / PEAK_TFLOPS, 4), "traffic": None,
                           "kernel": dom, "launches_per_step": d["launches"],
                           "avg_launch_ms": round(d["ms"] / d["launches"], 4),
                           "gflop_per_launch": round(d["flops"] / d["launches"] / 1e9, 2),
                           "step_frac_of_peak": round(value / world * eng.flops(1) / 1e12 / PEAK_TFLOPS, 4)}
        # HBM bytes per launch of the dominant kernel: PMC counters cannot be read from inside this process, so the
        # figure is the committed rocprofv3 --pmc result for this same workload (profiles/r01_traffic.json)
        # (profiles/r<NN>_traffic.json, tied to the kernel sources by their digest: a different build => null)
        import glob
        for tf_ in sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9]*_traffic.json")), reverse=True):   # newest round first
            try:
                tj = json.load(open(tf_))
                tr = tj["kernels"].get(dom)
                if tr and (B, S, args.dtype) == (256, 224, "f16") and tj.get("source_digest") == source_digest():
                    out["roofline"]["traffic"] = tr["hbm_bytes_per_launch"]
                    out["roofline"]["traffic_source"] = f"profiles/{os.path.basename(tf_)} (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, bytes/launch)"
                    break
            except (OSError, ValueError, KeyError):
                continue
        out["source_digest"] = source_digest()
        out["kernels_ms_per_step"] = {k: round(v["ms"], 4) for k, v in sorted(per_kernel.items(), key=lambda kv: -kv[1]["ms"])}
        # ---- parity of this very configuration against the oracle on a sample ---------------------
        out["rot_err_vs_oracle"] = oracle_sample_err(eng, x, fmt, R)
    eng.close()

    if args.full and not args.no_alt and world == 1:
        alt = "bf16" if args.dtype == "f16" else "f16"
        eng2, x2, fmt2, dt2, R2, _, _, _ = measure(alt)
        err2 = oracle_sample_err(eng2, x2, fmt2, R2)
        out["alt_dtype"] = {"dtype": alt, "value": round(K * B / dt2, 1), "ms_per_step": round(dt2 / K * 1e3, 4),
                            "max_abs_R_vs_oracle": err2["max_abs_R"], "meets_1e-3": err2["max_abs_R"] <= 1e-3}
        eng2.close()
        # BASELINE.json quotes configs[1] in bf16; the headline dtype is the one that meets north_star's 1e-3 gate
        out["bf16_meets_1e-3"] = bool(out["alt_dtype"]["meets_1e-3"]) if alt == "bf16" else bool(out["rot_err_vs_oracle"]["max_abs_R"] <= 1e-3)
        out["headline_dtype_meets_1e-3"] = bool(out["rot_err_vs_oracle"]["max_abs_R"] <= 1e-3)
        # the reference's own crop size (fast_pose_predictor.py:115-116): 512 x 512, same batch
        if S == 224:
            k5 = max(5, K // 5)
            eng5, _, _, dt5, _, _, _, _ = measure(args.dtype, S=512, K=k5, W=2)
            out["alt_shapes"] = {"512": {"value": round(k5 * B / dt5, 1), "ms_per_step": round(dt5 / k5 * 1e3, 4), "steps": k5,
                                         "step_frac_of_peak": round(k5 * B / dt5 * eng5.flops(1) / 1e12 / PEAK_TFLOPS, 4),
                                         "note": "reference-true crop size, batch %d" % B}}
            eng5.close()

    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(S, 16)
        big = cpu_baseline(S, 256, budget_s=8.0)
        out["cpu_baseline"]["batch_256"] = {"value": big["value"], "sample": big["sample"]}

    if args.full and rank == 0 and world == 1 and not args.no_autotune and os.environ.get("FLOPE_BENCH_CHILD") != "1":
        out["no_autotune"] = no_autotune_child(args)

    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        D.barrier()                       # rank 0 profiles / checks after the timed region: nobody tears down before it is done
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
