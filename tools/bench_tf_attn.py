"""16-bit encoder: the attention kernel a launch takes today (attn_tiled = 0) against the streaming MFMA kernel tf_attn_tiled
(attn_tiled = 1 or 2) on ONE handle in ONE process, the option flipped between forwards.  Device events around whole forwards and,
separately, around the attention launch alone (flope_tf_attention on a random qkv buffer); both sides warmed at each shape,
alternating pairs; per shape one JSON line with the median and the spread (min .. max) of each side, all of them also written to
--out.

    python tools/bench_tf_attn.py [--pairs 7] [--dtype f16] [--shapes long,hd32,hd128,throughput] [--out profiles/tf_attn_tiled_ab.json]

Shapes that run tf_attn_generic today (option 1 against 0): `long` (B = 16, L = 1024, d = 256, 4 heads: head_dim 64, more keys than
tf_attn_mfma holds), `hd32` (B = 256, L = 257, d = 384, 12 heads), `hd128` (B = 32, L = 577, d = 512, 4 heads); two layers each.
`throughput` is the build-defined cfg5 shape (B = 256, L = 257, d = 384, 6 heads, 12 layers), where option 0 runs tf_attn_mfma:
option 2 against 0, recorded only."""
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
SHAPES = {  # name: (dims (in, d, out, heads, layers, ff), B, L, option of the new side, note)
    "long": ((32, 256, 9, 4, 2, 1024), 16, 1024, 1, "head_dim 64, L > 512: more keys than tf_attn_mfma holds"),
    "hd32": ((32, 384, 9, 12, 2, 1536), 256, 257, 1, "head_dim 32"),
    "hd128": ((32, 512, 9, 4, 2, 2048), 32, 577, 1, "head_dim 128"),
    "throughput": ((32, 384, 9, 6, 12, 1536), 256, 257, 2, "build-defined cfg5 throughput shape: option 0 runs tf_attn_mfma; recorded only"),
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
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    ap.add_argument("--shapes", default="long,hd32,hd128,throughput")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_attn_tiled_ab.json"))
    a = ap.parse_args()
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}[a.dtype]
    rows = []
    for name in a.shapes.split(","):
        dims, B, L, opt, note = SHAPES[name]
        sd = synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
        enc = TransformerEncoder(*dims, dtype=a.dtype, max_tokens=B * L)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, L, dims[0])).astype(np.float32)).cuda()
        qkv = torch.randn(B, L, 3 * dims[1], device="cuda").to(tdt)
        att = torch.empty(B, L, dims[1], dtype=tdt, device="cuda")
        sides = [("option0", 0), (f"option{opt}", opt)]
        kernel = {}
        for _ in range(2):                                   # warm-up of every side
            for side, v in sides:
                enc.set_option("attn_tiled", v)
                enc(x)
                enc.attention(qkv, out=att)
                kernel[side] = KERNELS[enc.last_attn_kernel]
        torch.cuda.synchronize()
        fwd = {s: [] for s, _ in sides}
        alone = {s: [] for s, _ in sides}
        for _ in range(a.pairs):
            for side, v in sides:
                enc.set_option("attn_tiled", v)
                fwd[side].append(timed(lambda: enc(x), a.iters))
                alone[side].append(timed(lambda: enc.attention(qkv, out=att), a.iters))
        row = {"shape": name, "note": note, "dtype": a.dtype, "dims_in_d_out_heads_layers_ff": dims, "batch": B, "seq_len": L,
               "head_dim": dims[1] // dims[3], "pairs": a.pairs, "forwards_per_sample": a.iters,
               "attention_gflop": round(4.0 * B * L * L * dims[1] / 1e9, 3)}
        for side, _ in sides:
            row[side] = {"attention_kernel": kernel[side], "forward": stats(fwd[side]), "attention_alone": stats(alone[side])}
            row[side]["attention_alone"]["tflops"] = round(4.0 * B * L * L * dims[1] / statistics.median(alone[side]) / 1e9, 2)
        new = sides[1][0]
        for what in ("forward", "attention_alone"):
            row[f"{what}_ratio_of_medians_option0_over_{new}"] = round(row["option0"][what]["ms_median"] / row[new][what]["ms_median"], 3)
            row[f"{what}_fastest_option0_over_slowest_{new}"] = round(row["option0"][what]["ms_min"] / row[new][what]["ms_max"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        enc.close()
        del x, qkv, att
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
