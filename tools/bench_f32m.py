"""Float32 trunk: naive_conv_kernel (f32mfma = 0) against conv_f32m_kernel (f32mfma = 1) on ONE engine in ONE process, the option
flipped between forwards.  Device events around whole forwards, both modes warmed at each shape, alternating pairs; per shape one
JSON line with the median and the spread (min .. max) of each side.

    python tools/bench_f32m.py [--pairs 7] [--iters 3] [--shapes 64x224,256x224,16x512] [--per-launch]

--per-launch: afterwards one profiled forward (engine option profile = 1: an event around every launch, one slice) of the f32m
mode per shape, each conv's time and its share of the 155 TFLOP/s the instruction sustains on this chip."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flope_amd.engine import PoseEngine  # noqa: E402
from flope_amd.weights import synthetic_state_dict  # noqa: E402

PEAK_TFLOPS = 155.0


def timed(eng, x, R, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        eng.forward_into(x, 0, None, R)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shapes", default="64x224,256x224,16x512")
    ap.add_argument("--per-launch", action="store_true")
    a = ap.parse_args()
    sd = synthetic_state_dict(0)
    for shape in a.shapes.split(","):
        B, S = (int(v) for v in shape.split("x"))
        eng = PoseEngine(S, S, B, "f32")
        eng.load_state_dict(sd)
        torch.manual_seed(0)
        x = torch.rand(B, 3, S, S).cuda()
        R = torch.empty(B, 9, device="cuda")
        for mode in (0, 1, 0, 1):                           # warm-up of both sides
            eng.set_option("f32mfma", mode)
            eng.forward_into(x, 0, None, R)
        torch.cuda.synchronize()
        ms = {0: [], 1: []}
        for _ in range(a.pairs):
            for mode in (0, 1):
                eng.set_option("f32mfma", mode)
                ms[mode].append(timed(eng, x, R, a.iters if mode else 1))
        fl = eng.flops(B)
        row = {"batch": B, "crop": S, "pairs": a.pairs}
        for mode, name in ((0, "naive"), (1, "f32m")):
            med = statistics.median(ms[mode])
            row[name] = {"ms_median": round(med, 3), "ms_min": round(min(ms[mode]), 3), "ms_max": round(max(ms[mode]), 3),
                         "poses_per_s": round(B / med * 1e3, 1), "tflops": round(fl / med / 1e9, 1)}
        row["speedup_median"] = round(row["naive"]["ms_median"] / row["f32m"]["ms_median"], 2)
        row["slowest_f32m_vs_fastest_naive"] = round(row["naive"]["ms_min"] / row["f32m"]["ms_max"], 2)
        print(json.dumps(row), flush=True)
        if a.per_launch:
            eng.set_option("f32mfma", 1)
            eng.set_option("profile", 1)
            for _ in range(2):
                eng.forward_into(x, 0, None, R)
            t = eng.profile_read()
            eng.set_option("profile", 0)
            print(f"per launch, B = {B} x {S}^2, f32mfma = 1 (one slice):")
            for (layer, kern, f), msi in zip(eng.launch_info(B), t):
                share = f / (msi * 1e-3) / 1e12 / PEAK_TFLOPS if f and kern.startswith("conv_f32m") else None
                print(f"  {layer:30s} {kern:32s} {msi * 1e3:9.1f} us" + (f"  {f / (msi * 1e-3) / 1e12:6.1f} TFLOP/s  {100 * share:5.1f} % of peak" if share is not None else ""))
            print(f"  total {sum(t):.3f} ms", flush=True)
        eng.close()
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
