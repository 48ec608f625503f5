"""Sliding-window attention on the 16-bit MFMA kernels (option window_mfma) against the generic kernel the same call
takes without the option, on ONE handle in ONE process (tools/bench_tf_causal.py's method): every side warmed, alternating windows,
device events around `iters` calls per window; per timed thing one JSON line with the median and the spread (min .. max) of each
side, all of them also written to --out.

    python tools/bench_tf_window_mfma.py [--pairs 9] [--iters 5] [--out profiles/tf_window_mfma_ab.json]

f16, the cfg5 dims (d = 384, 6 heads of 64, 12 layers), attn_tiled = 1, B = 16, L = 2048, W = 256; timed: enc.attention alone, and the
whole forward.  Sides:
  A  window_mfma = 0: tf_attn_generic's WINDOW instantiation, what this very call runs without the option
  B  window_mfma = 1: tf_attn_tiled's WINDOW instantiation
  C  is_causal=True without a window on tf_attn_tiled; reported, no condition
Condition (attention alone): B's slowest window is faster than A's fastest.  Exit status 1 when it is missed.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flope_amd.tf_encoder import TransformerEncoder  # noqa: E402
from oracle.tf_encoder_ref import synthetic_state_dict  # noqa: E402  (weights only; nothing is checked here)

KERNELS = {0: "tf_attn_generic", 1: "tf_attn_mfma", 2: "tf_attn_tiled", 3: "tf_attn_f32m"}
DIMS = (32, 384, 9, 6, 12, 1536)
B, L, W, TILED = 16, 2048, 256, 1
SIDES = [("A_window_generic", 0, W), ("B_window_mfma", 1, W), ("C_causal_no_window", 1, 0)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_window_mfma_ab.json"))
    a = ap.parse_args()
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=B * L, attn_tiled=TILED)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, L, DIMS[0])).astype(np.float32)).cuda()
    qkv = torch.randn(B, L, 3 * DIMS[1], device="cuda").to(torch.float16)
    att = torch.empty(B, L, DIMS[1], dtype=torch.float16, device="cuda")

    def run(what, opt, w):
        enc.set_option("window_mfma", opt)
        if what == "attention":
            enc.attention(qkv, out=att, is_causal=True, window=w)
        else:
            enc(x, is_causal=True, window=w)

    rows, missed = [], False
    for what in ("attention", "forward"):
        kernel = {}
        for _ in range(3):                                   # warm-up of every side
            for side, opt, w in SIDES:
                run(what, opt, w)
                if what == "attention":
                    kernel[side] = KERNELS.get(enc.last_attn_kernel)
        torch.cuda.synchronize()
        t = {s: [] for s, _, _ in SIDES}
        for _ in range(a.pairs):
            for side, opt, w in SIDES:
                t[side].append(timed(lambda: run(what, opt, w), a.iters))
        row = {"timed": what, "dtype": "f16", "dims_in_d_out_heads_layers_ff": DIMS, "batch": B, "seq_len": L, "window": W,
               "head_dim": DIMS[1] // DIMS[3], "attn_tiled": TILED, "pairs": a.pairs, "calls_per_window": a.iters, "gated": what == "attention"}
        for side, _, _ in SIDES:
            row[side] = stats(t[side])
            if side in kernel:
                row[side]["attention_kernel"] = kernel[side]
        row["ratio_of_medians_B_over_A"] = round(row["B_window_mfma"]["ms_median"] / row["A_window_generic"]["ms_median"], 3)
        row["ratio_of_medians_B_over_C"] = round(row["B_window_mfma"]["ms_median"] / row["C_causal_no_window"]["ms_median"], 3)
        if what == "attention":
            row["condition_slowest_B_faster_than_fastest_A"] = row["B_window_mfma"]["ms_max"] < row["A_window_generic"]["ms_min"]
            missed = missed or not row["condition_slowest_B_faster_than_fastest_A"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    sys.exit(1 if missed else 0)


if __name__ == "__main__":
    main()
