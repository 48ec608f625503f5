"""Encoder, ragged batches: the packed forward `enc(x, lengths=...)` (flope_tf_forward_varlen) against the only one-launch-sequence
way the fixed-length path has to push the same batch through -- `enc(x)` on the padded [B, L] batch, whose answers are WRONG for ragged
data (padding is attended to); it is the time yardstick only.  ONE handle in ONE process, both sides warmed, alternating pairs,
device events around whole forwards; per shape one JSON line with the median and the spread (min .. max) of each side and the token
fraction T / (B L), all of them also written to --out.

    python tools/bench_tf_varlen.py [--pairs 7] [--iters 3] [--dtype f16] [--shapes cfg5,flower,cfg5_full] [--out profiles/tf_varlen_ab.json]

`cfg5`: B = 256, L = 257, d = 384, 6 heads, two layers, lengths drawn once (seeded) uniform in [L / 4, L].  `flower`: the dataset's
shape, B = 256 frames padded to L = 15 flowers, lengths uniform in [1, 15], the toy dimensions widened to d = 128.  `cfg5_full`:
cfg5 with every length = L: the cost of the gather, the scatter and the table upload alone (recorded, not gated)."""
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

CFG5 = (32, 384, 9, 6, 2, 1536)
FLOWER = (16, 128, 9, 4, 2, 256)
SHAPES = {  # name: (dims (in, d, out, heads, layers, ff), B, L, lowest length or None for all = L, note)
    "cfg5": (CFG5, 256, 257, 257 // 4, "cfg5 dims, two layers; lengths uniform in [L/4, L]"),
    "flower": (FLOWER, 256, 15, 1, "frames padded to 15 flowers; lengths uniform in [1, 15]; toy dims widened to d = 128"),
    "cfg5_full": (CFG5, 256, 257, None, "every length = L: gather + scatter + table upload alone; recorded only"),
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
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32", "f32m"])
    ap.add_argument("--shapes", default="cfg5,flower,cfg5_full")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_varlen_ab.json"))
    a = ap.parse_args()
    rows = []
    for name in a.shapes.split(","):
        dims, B, L, lo, note = SHAPES[name]
        sd = synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
        enc = TransformerEncoder(*dims, dtype=a.dtype, max_tokens=B * L)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        rng = np.random.default_rng(1)
        x = torch.from_numpy(rng.standard_normal((B, L, dims[0])).astype(np.float32)).cuda()
        lengths = [L] * B if lo is None else [int(v) for v in np.random.default_rng(7).integers(lo, L + 1, B)]
        sides = [("padded", lambda: enc(x)), ("ragged", lambda: enc(x, lengths=lengths))]
        for _ in range(2):                                   # warm-up of both sides
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        fwd = {s: [] for s, _ in sides}
        for _ in range(a.pairs):
            for side, fn in sides:
                fwd[side].append(timed(fn, a.iters))
        T = sum(lengths)
        row = {"shape": name, "note": note, "dtype": a.dtype, "dims_in_d_out_heads_layers_ff": dims, "batch": B, "seq_len": L,
               "tokens": T, "longest": max(lengths), "token_fraction": round(T / (B * L), 4),
               "attention_fraction": round(sum(v * v for v in lengths) / (B * L * L), 4),
               "gflop_padded": round(enc.flops(B, L) / 1e9, 3), "gflop_ragged": round(enc.flops(B, L, lengths=lengths) / 1e9, 3),
               "pairs": a.pairs, "forwards_per_sample": a.iters,
               "padded": stats(fwd["padded"]), "ragged": stats(fwd["ragged"])}
        row["ratio_of_medians_padded_over_ragged"] = round(row["padded"]["ms_median"] / row["ragged"]["ms_median"], 3)
        row["fastest_padded_over_slowest_ragged"] = round(row["padded"]["ms_min"] / row["ragged"]["ms_max"], 3)
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
