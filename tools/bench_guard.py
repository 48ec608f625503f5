"""Guarded mode (GuardedPoseEngine) against the plain f16 engine in ONE process: the guard's own f16 engine
runs both arms, alternating, device events around each, both warmed, `--pairs` pairs per figure.

    python tools/bench_guard.py [--pairs 5] [--iters 10] [--shapes 256x224,16x512,31x512] [--flagged 0,1,8,32] [--e2e] [--out profiles/guard_ab.json]

Per shape and per number of flagged crops (forced through gap_min on a head re-biased as in tests/test_gpu_guard.py, so that the gaps
are small and distinct):
  * flagged = 0: device time on the caller's stream of flope_guard_forward (f16 forward; the selection kernel runs behind it on the guard's
    own stream) against flope_forward_poses; the
    host-synchronised loop (forward, repair, next forward) and the two-slot loop (forward i + 1 enqueued before repair i) in
    poses/s against the plain loop that never synchronises.
  * flagged > 0: device time of the guarded pair (forward, host wait, gather, float32 forward, scatter) against the plain forward,
    and the added time against an f32m forward of that many crops alone on the same float32 engine; the same two figures with the
    float32 engine's option f32m_ksplit = 1 (what GuardedPoseEngine(exact_dtype="f32mk") runs).
--e2e: frame -> poses with the built-in detector (synthetic weights, 1080p), FLOPE_DTYPE=guard against f16, no crop flagged,
sequential and pipelined.  One JSON document; every figure is named for what it is."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flope_amd")]
from flope_amd.engine import GuardedPoseEngine  # noqa: E402
from flope_amd.weights import synthetic_state_dict  # noqa: E402


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def device_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def wall_rate(fn, iters, batch, drain=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    if drain:
        drain()
    torch.cuda.synchronize()
    return batch * iters / (time.perf_counter() - t0)


def bench_shape(B, S, flagged, pairs, iters, sd):
    g = GuardedPoseEngine(S, S, B, 32)
    torch.manual_seed(0)
    x = torch.rand(B, 3, S, S).cuda()
    xyz = torch.rand(B, 3).cuda()
    sd0 = dict(sd)
    sd0["fc_rot.bias"] = torch.zeros(9)
    g.load_state_dict(sd0)
    r9 = torch.empty(B, 9, device="cuda")
    bufs = [[torch.empty(B, n, device="cuda") for n in (9, 16)] + [torch.empty(B, device="cuda")] for _ in range(2)]
    R, Rt, gap = bufs[0]
    g.fast.forward_into(x, 0, r9, None)
    torch.cuda.synchronize()
    sdb = dict(sd)
    sdb["fc_rot.bias"] = sd["fc_rot.bias"] * 0.03 - r9.cpu().mean(0)
    g.load_state_dict(sdb)
    g.gap_min = -1.0
    g.forward_poses_into(x, 0, xyz, True, Rt, R, gap=gap)
    torch.cuda.synchronize()
    gaps = np.sort(gap.cpu().numpy().astype(np.float64))
    rows = []

    def plain():
        g.fast.forward_poses_into(x, 0, xyz, True, Rt, R)

    def pair():
        g.guard_forward(0, x, 0, xyz, True, None, R, Rt, gap)
        return g.guard_repair(0)

    for k in sorted({min(int(f), B) for f in flagged}):
        g.gap_min = -1.0 if k == 0 else float(gaps[-1] + 1.0) if k == B else float((gaps[k - 1] + gaps[k]) / 2)
        assert pair() == k
        row = {"batch": B, "crop": S, "flagged": k, "gap_min": round(g.gap_min, 5), "pairs": pairs, "iters": iters}
        for _ in range(2):
            plain()
            pair()
        torch.cuda.synchronize()
        if k == 0:
            # the forward alone: one forward per slot (16 slots), every slot repaired (count 0: nothing launched) after the timed region
            n = g.slots
            p_us, f_us = [], []

            def forwards():
                for s in range(n):
                    g.guard_forward(s, x, 0, xyz, True, None, R, Rt, gap)

            for _ in range(pairs):
                p_us.append(device_us(plain, n))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                forwards()
                e1.record()
                e1.synchronize()
                f_us.append(e0.elapsed_time(e1) / n * 1e3)
                assert all(g.guard_repair(s) == 0 for s in range(n))
            row["plain_forward_poses_us"], row["guard_forward_us"] = stats(p_us), stats(f_us)
            row["guard_forward_over_plain_percent"] = round(100 * (statistics.median(f_us) / statistics.median(p_us) - 1), 3)
            # loops in wall time
            rate = {"plain_unsynchronised": [], "guard_one_slot_synchronised": [], "guard_two_slots": []}
            for _ in range(pairs):
                rate["plain_unsynchronised"].append(wall_rate(lambda i: plain(), 4 * iters, B))
                rate["guard_one_slot_synchronised"].append(wall_rate(lambda i: pair(), 4 * iters, B))

                def two(i):
                    R2, Rt2, gap2 = bufs[i & 1]
                    g.guard_forward(i & 1, x, 0, xyz, True, None, R2, Rt2, gap2)
                    if i:
                        g.guard_repair((i - 1) & 1)
                rate["guard_two_slots"].append(wall_rate(two, 4 * iters, B, drain=lambda: g.guard_repair((4 * iters - 1) & 1)))
            row["poses_per_s"] = {name: stats(v) for name, v in rate.items()}
        else:
            xs, xyzs = x[:k].contiguous(), xyz[:k].contiguous()
            Rs, Rts = torch.empty(k, 9, device="cuda"), torch.empty(k, 16, device="cuda")

            def exact_alone():
                g.exact.forward_poses_into(xs, 0, xyzs, True, Rts, Rs)

            for _ in range(2):
                exact_alone()
            p_us, g_us, e_us, gk_us, ek_us = [], [], [], [], []
            g.exact.set_option("f32m_ksplit", 1)              # the exact_dtype="f32mk" arm: the same guard, the float32 engine's option flipped
            for _ in range(2):
                pair()
                exact_alone()
            g.exact.set_option("f32m_ksplit", 0)
            for _ in range(pairs):
                p_us.append(device_us(plain, iters))
                g_us.append(device_us(pair, iters))
                e_us.append(device_us(exact_alone, iters))
                g.exact.set_option("f32m_ksplit", 1)
                gk_us.append(device_us(pair, iters))
                ek_us.append(device_us(exact_alone, iters))
                g.exact.set_option("f32m_ksplit", 0)
            row["guard_forward_and_repair_f32mk_us"], row["f32mk_forward_of_flagged_crops_alone_us"] = stats(gk_us), stats(ek_us)
            row["added_f32mk_us"] = round(statistics.median(gk_us) - statistics.median(p_us), 1)
            row["plain_forward_poses_us"], row["guard_forward_and_repair_us"], row["f32m_forward_of_flagged_crops_alone_us"] = stats(p_us), stats(g_us), stats(e_us)
            row["added_us"] = round(statistics.median(g_us) - statistics.median(p_us), 1)
            row["added_over_f32m_alone"] = round(row["added_us"] / statistics.median(e_us), 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    g.close()
    del x
    torch.cuda.empty_cache()
    return rows


def bench_e2e(frames_n=60):
    import yaml
    from flope_amd.yolo_weights import synthetic_frame, synthetic_yolo_state_dict
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    tmp = tempfile.mkdtemp()
    ckpt, intr, yolo_f = (os.path.join(tmp, n) for n in ("posenet.pth", "intrinsics.yaml", "yolo11n_seg.pth"))
    torch.save(synthetic_state_dict(0), ckpt)
    open(intr, "w").write(yaml.safe_dump(dict(fx=1400.0, fy=1400.0, cx=960.0, cy=540.0, h=1080, w=1920)))
    torch.save({**synthetic_yolo_state_dict(0), "imgsz": torch.tensor(1280)}, yolo_f)
    rgb = synthetic_frame(0)
    depth = (400 + np.random.default_rng(0).normal(0, 4, rgb.shape[:2])).astype(np.uint16)
    frames = [(rgb, depth)] * frames_n
    preds = {}
    for mode in ("f16", "guard"):
        os.environ["FLOPE_DTYPE"] = mode
        preds[mode] = FastPosePredictor("cuda", yolo_f, ckpt, intr)
        for _ in range(3):
            preds[mode].get_flower_poses(rgb, depth)
        list(preds[mode].iter_flower_poses(frames[:12]))
    out = {"frames": frames_n, "sequential_ms_per_frame": {"f16": [], "guard": []}, "pipelined_ms_per_frame": {"f16": [], "guard": []}}
    for _ in range(3):
        for mode, p in preds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                Rt = p.get_flower_poses(rgb, depth)
            out["sequential_ms_per_frame"][mode].append((time.perf_counter() - t0) / 20 * 1e3)
            t0 = time.perf_counter()
            list(p.iter_flower_poses(frames))
            out["pipelined_ms_per_frame"][mode].append((time.perf_counter() - t0) / frames_n * 1e3)
    out["poses_per_frame"] = 0 if Rt is None else int(Rt.shape[0])
    out["repaired_last_frame"] = preds["guard"].posenet.engine_for("cuda", (512, 512)).read_selection(0)
    for key in ("sequential_ms_per_frame", "pipelined_ms_per_frame"):
        out[key] = {m: stats(v) for m, v in out[key].items()}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="256x224,16x512,31x512")
    ap.add_argument("--flagged", default="0,1,8,32")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guard_ab.json"))
    a = ap.parse_args()
    sd = synthetic_state_dict(0)
    doc = {"tool": "tools/bench_guard.py", "device": torch.cuda.get_device_name(0), "shapes": []}
    for shape in a.shapes.split(","):
        B, S = (int(v) for v in shape.split("x"))
        doc["shapes"] += bench_shape(B, S, a.flagged.split(","), a.pairs, a.iters, sd)
    if a.e2e:
        doc["frame_to_poses_builtin_detector_no_crop_flagged"] = bench_e2e()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
