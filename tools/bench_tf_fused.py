"""Float32 encoder: the launch sequence (fused = 0: 2 + 7 num_layers kernels, two more for a ragged batch) against the single launch
of option fused (tf_fused_f32, one sequence per workgroup) on ONE handle in ONE process, the option flipped between
windows.  Device events around windows of --iters forwards after a warm-up of both sides, alternating pairs; per shape one JSON line
with the median and the spread (min .. max) of each side in microseconds per forward, all of them also written to --out.  The numbers
are what a caller of `enc(x)` sees: they include the host's enqueue cost wherever the device is waiting for it.

    python tools/bench_tf_fused.py [--pairs 5] [--iters 200] [--shapes toy,single,batch256,batch256_len64,ragged] [--out profiles/tf_fused_ab.json]
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

TOY = (16, 32, 9, 4, 2, 64)      # (in, d, out, heads, layers, ff) of the reference's encoder
SHAPES = {  # name: (dims, B, L, lengths or None, note)
    "toy": (TOY, 8, 10, None, "the reference's own shape: 16 launches of a few KB each against one"),
    "single": (TOY, 1, 10, None, "one sequence: one workgroup on the whole chip"),
    "batch256": (TOY, 256, 10, None, "256 sequences: one workgroup per CU"),
    "batch256_len64": (TOY, 256, 64, None, "longer sequences on the toy's dimensions: one workgroup per sequence against grids that fill the chip"),
    "ragged": (TOY, 8, 10, [10, 1, 3, 7, 10, 2, 9, 5], "a ragged toy batch: 18 launches and an offset upload against one launch and the upload"),
}


def timed(enc, x, lengths, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        enc(x, lengths=lengths)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # microseconds per forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_fused_ab.json"))
    a = ap.parse_args()
    if a.pairs < 5 or a.iters < 200:
        ap.error("at least 5 pairs of windows of at least 200 forwards")
    rows = []
    for name in a.shapes.split(","):
        dims, B, L, lengths, note = SHAPES[name]
        sd = synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
        enc = TransformerEncoder(*dims, dtype="f32", max_tokens=B * L)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, L, dims[0])).astype(np.float32)).cuda()
        plans = {}
        for side, v in (("launches", 0), ("fused", 1)):       # warm-up of both sides, and what each side really runs
            enc.set_option("fused", v)
            plans[side] = enc.forward_plan(B, L, lengths=lengths)
            for _ in range(20):
                enc(x, lengths=lengths)
        torch.cuda.synchronize()
        us = {"launches": [], "fused": []}
        for _ in range(a.pairs):
            for side, v in (("launches", 0), ("fused", 1)):
                enc.set_option("fused", v)
                us[side].append(timed(enc, x, lengths, a.iters))
        row = {"shape": name, "note": note, "dims_in_d_out_heads_layers_ff": dims, "batch": B, "seq_len": L, "lengths": lengths,
               "pairs": a.pairs, "forwards_per_window": a.iters, "unit": "microseconds per forward, device events around a window, host enqueue included"}
        for side in ("launches", "fused"):
            row[side] = {"plan": plans[side], "us_median": round(statistics.median(us[side]), 2), "us_min": round(min(us[side]), 2),
                         "us_max": round(max(us[side]), 2), "us_windows": [round(v, 2) for v in us[side]]}
        row["ratio_of_medians_launches_over_fused"] = round(row["launches"]["us_median"] / row["fused"]["us_median"], 3)
        row["slowest_fused_over_fastest_launches"] = round(row["fused"]["us_max"] / row["launches"]["us_min"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        enc.close()
        del x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
