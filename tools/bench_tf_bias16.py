"""A compiled per-head bias on the 16-bit MFMA attention (option "bias_mfma") against the path it replaces and against its
floors, on ONE handle in ONE process (tools/bench_tf_attn.py's method): every side warmed, alternating windows, device
events around `iters` calls per window; one JSON line per point, side and level and one per point for the comparison, all of them also
written to --out.

    python tools/bench_tf_bias16.py [--pairs 9] [--iters 5] [--out profiles/tf_bias16_ab.json]

The handle is the build-defined cfg5 (d = 384, 6 heads of 64, 12 layers, f16) under the per-head causal ALiBi bias, slopes 2^-(h + 1), at
two points -- B = 64, L = 256 (DESIGN.md 39's) and B = 4, L = 2048 (planes of 96 MiB: not to be assumed in L2) -- measured at
enc.attention (one launch) and at the whole forward:

  A  bias_mfma = 0: tf_attn_masked<T, VARLEN, BIASED = true>, the only path this call had
  B  bias_mfma = 1: tf_attn_tiled_masked<T, 2, VARLEN, BIASED = true>
  C  the compiled causal mask under mask_mfma = 1: tf_attn_tiled_masked, the floor without bias traffic
  D  enc(x, is_causal=True): the dedicated causal kernel

The condition (as DESIGN.md 38's): B's slowest window is faster than A's fastest, at both levels and both points.  Recorded beside the
times: B / A and B / C of the medians and the bias bytes one launch of B addresses (4 KiB per taken 32 x 32 step tile and head, shared by
the batch).
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
from flope_amd.tf_encoder import TransformerEncoder, alibi_bias  # noqa: E402
from oracle.tf_encoder_ref import synthetic_state_dict  # noqa: E402  (weights only; nothing is checked here)

DIMS = (32, 384, 9, 6, 12, 1536)
POINTS = ((64, 256), (4, 2048))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_bias16_ab.json"))
    a = ap.parse_args()
    H = DIMS[3]
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=max(B * L for B, L in POINTS))
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    rng = np.random.default_rng(1)
    rows = []
    for B, L in POINTS:
        x = torch.from_numpy(rng.standard_normal((B, L, DIMS[0])).astype(np.float32)).cuda()
        qkv = torch.from_numpy(rng.standard_normal((B, L, 3 * DIMS[1])).astype(np.float32)).to(torch.float16).cuda()
        att = torch.empty((B, L, DIMS[1]), dtype=torch.float16, device="cuda")
        i = torch.arange(L)
        mask = enc.make_mask(i[None, :] > i[:, None])
        bias = enc.make_bias(alibi_bias(L, [2.0 ** -(h + 1) for h in range(H)]))

        def side(bias_mfma, mask_mfma, run):
            def go():
                enc.set_option("bias_mfma", bias_mfma)
                enc.set_option("mask_mfma", mask_mfma)
                return run()
            return go

        levels = {"attention": [("A", side(0, 0, lambda: enc.attention(qkv, out=att, mask=bias))), ("B", side(1, 0, lambda: enc.attention(qkv, out=att, mask=bias))),
                                ("C", side(0, 1, lambda: enc.attention(qkv, out=att, mask=mask))), ("D", side(0, 0, lambda: enc.attention(qkv, out=att, is_causal=True)))],
                  "forward": [("A", side(0, 0, lambda: enc(x, mask=bias))), ("B", side(1, 0, lambda: enc(x, mask=bias))),
                              ("C", side(0, 1, lambda: enc(x, mask=mask))), ("D", side(0, 0, lambda: enc(x, is_causal=True)))]}
        kernels, by = {}, {}
        for level, sides in levels.items():
            for _ in range(2):                                   # warm-up of every side
                for name, run in sides:
                    run()
                    kernels[level, name] = None if (level, name) == ("forward", "D") else enc.last_attn_kernel      # an unmasked forward records none
            torch.cuda.synchronize()
            t = {name: [] for name, _ in sides}
            for _ in range(a.pairs):
                for name, run in sides:
                    t[name].append(timed(run, a.iters))
            for name, _ in sides:
                row = {"level": level, "side": name, "attn_kernel": kernels[level, name], "dtype": "f16", "dims_in_d_out_heads_layers_ff": DIMS, "batch": B,
                       "seq_len": L, "pairs": a.pairs, "calls_per_window": a.iters, **stats(t[name])}
                print(json.dumps(row), flush=True)
                rows.append(row)
                by[level, name] = row
        ts = bias.tile_stats
        cmp_row = {"comparison": True, "batch": B, "seq_len": L, "allowed_pairs": bias.allowed, "bias_planes": bias.planes, "tile_stats": ts,
                   "bias_bytes_allocated": H * L * L * 4, "bias_bytes_addressed_per_launch_B": (ts["steps_some"] + ts["steps_all"]) * 32 * 32 * 4 * H}
        for level in levels:
            A_, B_, C_ = by[level, "A"], by[level, "B"], by[level, "C"]
            cmp_row[f"B_over_A_{level}"] = round(B_["ms_median"] / A_["ms_median"], 4)
            cmp_row[f"B_over_C_{level}"] = round(B_["ms_median"] / C_["ms_median"], 4)
            cmp_row[f"B_slowest_faster_than_A_fastest_{level}"] = bool(B_["ms_max"] < A_["ms_min"])
        print(json.dumps(cmp_row), flush=True)
        rows.append(cmp_row)
        mask.close()
        bias.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    enc.close()


if __name__ == "__main__":
    main()
