"""Post-norm ReLU (the default architecture: the kernels of before) against pre-norm GELU with a final norm on the live step, by
tools/bench_tf_skinny_ln.py's method: ONE process, both handles made and warm first, the architecture
alternating between windows, device events around every window, median / minimum / maximum over the windows.  The architecture is
fixed per handle, so the two sides are two handles of the same dtype with the same layer weights.  Both run with skinny = 1 and
skinny_ln = 1: by count, not recorded here, a step is 64 launches on either side (post-norm folds 23 LayerNorms and launches one;
pre-norm folds 24 and launches the final norm; enc.last_ln is recorded per side).  What differs is the GELU epilogue of the twelve
linear1 launches and one more folded LayerNorm.  Nothing is gated: the exit status is 0 whatever comes out.  JSON lines on stdout,
the list in --out.

    python tools/bench_tf_arch.py [--pairs 9] [--calls 20] [--out profiles/tf_arch_ab.json]

  cfg5 (d = 384, 6 heads, 12 layers, ff = 1536), f16 and bf16; a windowed stream, W = 64 = capacity, every window full (a prefill of 64
  tokens per track first): one step() of n = 1, 16 and 31 rows; a window is `calls` steps between two events, its figure the time per step.
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

DIMS = (32, 384, 9, 6, 12, 1536)          # cfg5: in, d, out, heads, layers, ff
WINDOW = 64
ROWS = (1, 16, 31)
SIDES = {"post_relu": {}, "pre_gelu_fn": {"norm_first": True, "activation": "gelu", "final_norm": True}}


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # us per call


def stats(v):
    return {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_arch_ab.json"))
    a = ap.parse_args()
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    sd = {k: torch.from_numpy(v) for k, v in sd.items()}
    g = torch.Generator().manual_seed(50)
    sd_fn = dict(sd)
    sd_fn["transformer_encoder.norm.weight"] = 1.0 + 0.1 * torch.randn(DIMS[1], generator=g)
    sd_fn["transformer_encoder.norm.bias"] = 0.1 * torch.randn(DIMS[1], generator=g)
    rng = np.random.default_rng(1)
    rows = []
    for dtype in ("f16", "bf16"):
        encs = {}
        for side, arch in SIDES.items():
            encs[side] = TransformerEncoder(*DIMS, dtype=dtype, max_tokens=max(ROWS) * WINDOW, skinny=1, skinny_ln=1, **arch)
            encs[side].load_state_dict(sd_fn if arch.get("final_norm") else sd)
        for n in ROWS:
            hist = torch.from_numpy(rng.standard_normal((n, WINDOW + 1, DIMS[0])).astype(np.float32)).cuda()
            col, y = hist[:, WINDOW].contiguous(), torch.empty(n, DIMS[2], device="cuda")
            sts = {}
            for side, enc in encs.items():
                sts[side] = enc.open_stream(n, WINDOW, window=WINDOW)
                sts[side].prefill(hist[:, :WINDOW].contiguous())       # every window full from the first timed step on; a ring is never full
            torch.cuda.synchronize()
            t, seen = {s: [] for s in SIDES}, {}
            for rep in range(2 + a.pairs):                             # two warm-up rounds of both sides, then the alternating windows
                for side in SIDES:
                    us = timed(lambda: sts[side].step(col, out=y), a.calls)
                    seen[side] = encs[side].last_ln
                    if rep >= 2:
                        t[side].append(us)
            row = {"measurement": "stream_step", "dtype": dtype, "dims_in_d_out_heads_layers_ff": DIMS, "window": WINDOW, "capacity": WINDOW,
                   "rows_per_step": n, "option_skinny": 1, "option_skinny_ln": 1, "windows_per_side": a.pairs, "calls_per_window": a.calls}
            for side in SIDES:
                row[side] = stats(t[side])
                row["layernorms_launched_folded_" + side] = seen[side]
            row["ratio_of_medians_pre_gelu_fn_over_post_relu"] = round(row["pre_gelu_fn"]["us_median"] / row["post_relu"]["us_median"], 3)
            row["windows_separated"] = row["pre_gelu_fn"]["us_min"] > row["post_relu"]["us_max"] or row["pre_gelu_fn"]["us_max"] < row["post_relu"]["us_min"]
            print(json.dumps(row), flush=True)
            rows.append(row)
            for st in sts.values():
                st.close()
        for enc in encs.values():
            enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
