"""Causal attention against the same launch without the option, on ONE handle in ONE process (tools/bench_tf_attn.py's method): both
sides warmed at each shape, alternating windows, device events around `iters` calls per window; per shape one JSON line with the
median and the spread (min .. max) of each side, all of them also written to --out.

    python tools/bench_tf_causal.py [--pairs 9] [--iters 5] [--shapes tiled,resident,cfg5] [--out profiles/tf_causal_ab.json]

  tiled     tf_attn_tiled alone, f16, head_dim 64, L = 1024, B = 64 x 4 heads (2,048 workgroups of 128 queries): the GATED shape.
            Causal walks 72 of 128 block iterations; the condition is that the slowest causal window is faster than the fastest
            non-causal one (the margin of DESIGN.md 19).  Exit status 1 when it is missed.
  resident  tf_attn_mfma alone at the cfg5 attention shape (B = 256, L = 257, 6 heads of 64): staging is unchanged and a workgroup
            lasts as long as its last wave; recorded only.
  cfg5      the whole build-defined cfg5 forward (B = 256, L = 257, d = 384, 6 heads, 12 layers, f16); recorded only.
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
SHAPES = {  # name: (dims (in, d, out, heads, layers, ff), B, L, attn_tiled, what is timed, gated, note)
    "tiled": ((32, 256, 9, 4, 0, 1024), 64, 1024, 1, "attention", True, "tf_attn_tiled alone, head_dim 64: 72 of 128 block iterations under causal"),
    "resident": ((32, 384, 9, 6, 0, 1536), 256, 257, 0, "attention", False, "tf_attn_mfma alone at the cfg5 attention shape; recorded only"),
    "cfg5": ((32, 384, 9, 6, 12, 1536), 256, 257, 0, "forward", False, "the whole cfg5 forward; recorded only"),
}


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
    ap.add_argument("--shapes", default="tiled,resident,cfg5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_causal_ab.json"))
    a = ap.parse_args()
    rows, missed = [], False
    for name in a.shapes.split(","):
        dims, B, L, tiled, what, gated, note = SHAPES[name]
        enc = TransformerEncoder(*dims, dtype="f16", max_tokens=B * L, attn_tiled=tiled)
        if what == "forward":
            sd = synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
            enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, L, dims[0])).astype(np.float32)).cuda()
            run = lambda causal: enc(x, is_causal=causal)
        else:
            qkv = torch.randn(B, L, 3 * dims[1], device="cuda").to(torch.float16)
            att = torch.empty(B, L, dims[1], dtype=torch.float16, device="cuda")
            run = lambda causal: enc.attention(qkv, out=att, is_causal=causal)
        sides = [("plain", False), ("causal", True)]
        kernel = {}
        for _ in range(3):                                   # warm-up of both sides
            for side, c in sides:
                run(c)
                kernel[side] = KERNELS.get(enc.last_attn_kernel) if what == "attention" else None
        torch.cuda.synchronize()
        t = {s: [] for s, _ in sides}
        for _ in range(a.pairs):
            for side, c in sides:
                t[side].append(timed(lambda: run(c), a.iters))
        row = {"shape": name, "note": note, "timed": what, "dtype": "f16", "dims_in_d_out_heads_layers_ff": dims, "batch": B, "seq_len": L,
               "head_dim": dims[1] // dims[3], "attn_tiled": tiled, "pairs": a.pairs, "calls_per_window": a.iters, "gated": gated}
        for side, _ in sides:
            row[side] = stats(t[side])
            if kernel[side]:
                row[side]["attention_kernel"] = kernel[side]
        row["ratio_of_medians_causal_over_plain"] = round(row["causal"]["ms_median"] / row["plain"]["ms_median"], 3)
        row["slowest_causal_over_fastest_plain"] = round(row["causal"]["ms_max"] / row["plain"]["ms_min"], 3)
        if what == "attention":
            row["plain"]["tflops"] = round(4.0 * B * L * L * dims[1] / row["plain"]["ms_median"] / 1e9, 2)
            row["causal"]["tflops"] = round(2.0 * B * L * (L + 1) * dims[1] / row["causal"]["ms_median"] / 1e9, 2)
        if gated:
            row["condition_slowest_causal_faster_than_fastest_plain"] = row["causal"]["ms_max"] < row["plain"]["ms_min"]
            missed = missed or not row["condition_slowest_causal_faster_than_fastest_plain"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        enc.close()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    sys.exit(1 if missed else 0)


if __name__ == "__main__":
    main()
