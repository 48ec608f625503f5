"""Float32 MFMA trunk at small batches: option f32m_ksplit = 0 (every workgroup walks all of K: the parent's code path, untouched)
against f32m_ksplit = 1 (split-K per launch by plan.h's cost model) on ONE float32 engine with f32mfma = 1 in ONE process, the
option flipped between forwards.  Device events around whole forwards, both sides warmed at each shape, alternating pairs; per
shape one JSON line with the median and the spread (min .. max) of each side and the three verdicts of DESIGN.md 17:
  intervals_disjoint      the slowest option-1 forward is faster than the fastest option-0 forward (asked at B = 1 and B = 4)
  within_spread           the option-1 median is no slower than the option-0 median by more than option 0's own max - min
  same_plan               both sides launch the same list (the control, B = 64 x 224^2: two slices, nothing may split)

    python tools/bench_f32m_ksplit.py [--pairs 7] [--iters 5] [--shapes 1x224,...] [--json out.json] [--per-launch] [--forced 2,4,8,16,32]

--per-launch: per shape the engine's profile = 1 table (an event around every launch; a split conv's entry holds its split launch and
its finalize launch) for option values 0, 1 and the forced 2 .. 32, side by side: the table plan.h's kF32mStepCycles and
kF32mFinalizeCycles are to be fitted from, and the check that value 1 picked the best measured S per conv."""
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

SHAPES = ",".join(f"{b}x{s}" for s in (224, 512) for b in (1, 2, 4, 8, 16, 31)) + ",64x224"


def timed(eng, x, R, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        eng.forward_into(x, 0, None, R)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def profiled(eng, x, R, value, reps=3):
    """-> ([layer names], [per-launch us, the smallest of `reps` profiled forwards]) under f32m_ksplit = value"""
    eng.set_option("f32m_ksplit", value)
    eng.set_option("profile", 1)
    eng.forward_into(x, 0, None, R)
    runs = []
    for _ in range(reps):
        eng.forward_into(x, 0, None, R)
        runs.append(eng.profile_read())
    eng.set_option("profile", 0)
    return [layer for layer, _, _ in eng.launch_info(x.shape[0])], [min(r[i] for r in runs) * 1e3 for i in range(len(runs[0]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--json", default="")
    ap.add_argument("--per-launch", action="store_true")
    ap.add_argument("--forced", default="2,4,8,16,32")
    a = ap.parse_args()
    assert a.pairs >= 5, "at least five alternating pairs"
    sd = synthetic_state_dict(0)
    rows = []
    for shape in a.shapes.split(","):
        B, S = (int(v) for v in shape.split("x"))
        eng = PoseEngine(S, S, B, "f32")
        eng.load_state_dict(sd)
        eng.set_option("f32mfma", 1)
        torch.manual_seed(0)
        x = torch.rand(B, 3, S, S).cuda()
        R = torch.empty(B, 9, device="cuda")
        info = {}
        for mode in (0, 1, 0, 1):                           # warm-up of both sides
            eng.set_option("f32m_ksplit", mode)
            for _ in range(3):
                eng.forward_into(x, 0, None, R)
            info[mode] = eng.launch_info(B)
        torch.cuda.synchronize()
        ms = {0: [], 1: []}
        for _ in range(a.pairs):
            for mode in (0, 1):
                eng.set_option("f32m_ksplit", mode)
                ms[mode].append(timed(eng, x, R, a.iters))
        row = {"batch": B, "crop": S, "pairs": a.pairs, "iters": a.iters,
               "split": {layer.split("[")[0].replace("base.", ""): int(layer.split("x")[-1].rstrip("]")) for layer, _, _ in info[1] if "[split-K x" in layer}}
        for mode, name in ((0, "ksplit0"), (1, "ksplit1")):
            med = statistics.median(ms[mode])
            row[name] = {"ms_median": round(med, 4), "ms_min": round(min(ms[mode]), 4), "ms_max": round(max(ms[mode]), 4)}
        spread0 = row["ksplit0"]["ms_max"] - row["ksplit0"]["ms_min"]
        row["ratio_median"] = round(row["ksplit0"]["ms_median"] / row["ksplit1"]["ms_median"], 3)
        row["intervals_disjoint"] = row["ksplit1"]["ms_max"] < row["ksplit0"]["ms_min"]
        row["within_spread"] = row["ksplit1"]["ms_median"] <= row["ksplit0"]["ms_median"] + spread0
        row["same_plan"] = info[0] == info[1]
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.per_launch:
            values = [0, 1] + [int(v) for v in a.forced.split(",") if v]
            names, cols = None, {}
            for v in values:
                layers, cols[v] = profiled(eng, x, R, v)
                if v == 0:
                    names = layers
                cols[(v, "S")] = [int(layer.split("x")[-1].rstrip("]")) if "[split-K x" in layer else 1 for layer in layers]
            print(f"per launch, B = {B} x {S}^2, f32mfma = 1 (one slice), us (xS = the share count that ran); columns: f32m_ksplit = " +
                  ", ".join(str(v) for v in values))
            for i, layer in enumerate(names):
                cells = "".join(f" {cols[v][i]:8.1f}" + (f" x{cols[(v, 'S')][i]:<2d}" if cols[(v, 'S')][i] > 1 else "    ") for v in values)
                best = min(values[1:], key=lambda v: cols[v][i]) if layer.startswith("base.layer") else None
                note = ""
                if best is not None and cols[(1, "S")][i] != cols[(best, "S")][i] and cols[best][i] < 0.95 * cols[1][i]:
                    note = f"   <- x{cols[(best, 'S')][i]} measured {cols[1][i] / cols[best][i]:.2f} x faster than value 1's choice"
                print(f"  {layer:26s}{cells}{note}")
            print("  total (ms)               " + "".join(f" {sum(cols[v]) / 1e3:8.3f}    " for v in values), flush=True)
            eng.set_option("f32m_ksplit", 0)
        eng.close()
        del x
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
