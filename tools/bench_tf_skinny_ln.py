"""Option skinny_ln against the stand-alone LayerNorm launches it folds, on ONE handle per dtype in ONE process (tools/bench_tf_skinny.py's
method): option skinny is 1 on both sides, skinny_ln is flipped between alternating windows after both sides are
warm, device events around every window, median / minimum / maximum over the windows.  Option 0 is the parent's kernels in the same
library on the same box, never a number from another day.  Nothing is gated: the exit status is 0 whatever comes out.  JSON lines on
stdout, the list in --out.

    python tools/bench_tf_skinny_ln.py [--pairs 9] [--calls 20] [--out profiles/tf_skinny_ln_ab.json]

  cfg5 (d = 384, 6 heads, 12 layers, ff = 1536), f16 and bf16.
  stream    a windowed stream, W = 64 = capacity, every window full (a prefill of 64 tokens per track first): one step() of n = 1, 4, 16
            and 31 rows; a window is `calls` steps between two events, its figure the time per step.  Under option 1 a step is 64
            launches where it is 87 under option 0 (enc.last_ln is recorded per side).
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
ROWS = (1, 4, 16, 31)


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


def ab(enc, fn, calls, pairs):
    seen = {}

    def window(opt):
        enc.set_option("skinny_ln", opt)
        t = timed(fn, calls)
        seen[opt] = enc.last_ln
        return t
    for opt in (0, 1, 0, 1):                           # warm-up of both sides
        window(opt)
    t = {0: [], 1: []}
    for _ in range(pairs):
        for opt in (0, 1):
            t[opt].append(window(opt))
    enc.set_option("skinny_ln", 0)
    row = {"windows_per_side": pairs, "calls_per_window": calls, "layernorms_launched_folded_option_0": seen[0],
           "layernorms_launched_folded_option_1": seen[1], "option_0": stats(t[0]), "option_1": stats(t[1])}
    row["ratio_of_medians_option_0_over_option_1"] = round(row["option_0"]["us_median"] / row["option_1"]["us_median"], 3)
    row["slowest_option_1_faster_than_fastest_option_0"] = row["option_1"]["us_max"] < row["option_0"]["us_min"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_skinny_ln_ab.json"))
    a = ap.parse_args()
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    sd = {k: torch.from_numpy(v) for k, v in sd.items()}
    rng = np.random.default_rng(1)
    rows = []
    for dtype in ("f16", "bf16"):
        enc = TransformerEncoder(*DIMS, dtype=dtype, max_tokens=max(ROWS) * WINDOW, skinny=1)
        enc.load_state_dict(sd)
        for n in ROWS:
            hist = torch.from_numpy(rng.standard_normal((n, WINDOW + 1, DIMS[0])).astype(np.float32)).cuda()
            st = enc.open_stream(n, WINDOW, window=WINDOW)
            st.prefill(hist[:, :WINDOW].contiguous())  # every window full from the first timed step on; a ring is never full
            col, y = hist[:, WINDOW].contiguous(), torch.empty(n, DIMS[2], device="cuda")
            torch.cuda.synchronize()
            enc.set_option("skinny_ln", 1)
            plan = enc.linear_ln_plan("layers.0.linear1", n)
            enc.set_option("skinny_ln", 0)
            row = {"measurement": "stream_step", "dtype": dtype, "dims_in_d_out_heads_layers_ff": DIMS, "window": WINDOW, "capacity": WINDOW, "rows_per_step": n,
                   "option_skinny": 1, "linear1_kernel_under_option_1": plan}
            row.update(ab(enc, lambda: st.step(col, out=y), a.calls, a.pairs))
            print(json.dumps(row), flush=True)
            rows.append(row)
            st.close()
        enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
