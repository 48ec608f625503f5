"""A compiled per-head additive bias against the compiled mask of the same allowed set, on ONE handle in ONE process
(tools/bench_tf_attn.py's method): both sides warmed, alternating windows, device events around `iters` calls per
window; one JSON line per side and level and one for the comparison, all of them also written to --out.

    python tools/bench_tf_bias.py [--pairs 9] [--iters 5] [--out profiles/tf_bias_ab.json]

The handle is the build-defined cfg5 (d = 384, 6 heads, 12 layers, f16) at B = 64, L = 256, measured at enc.attention (one launch) and
at the whole forward:

  mask   (a) the compiled causal mask: tf_attn_masked
  bias   (b) the per-head causal ALiBi bias (slopes 2^-(h + 1)): tf_attn_masked<T, VARLEN, BIASED = true> -- the same walk plus one float32 load and one add
         per allowed pair

Nothing is gated: the feature replaces nothing.  Recorded beside the times: the bias bytes one launch reads, H * L^2 * 4 per layer
(the masked half of every plane is never read), shared by the batch.
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
B, L = 64, 256


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_bias_ab.json"))
    a = ap.parse_args()
    H = DIMS[3]
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=B * L)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((B, L, DIMS[0])).astype(np.float32)).cuda()
    qkv = torch.from_numpy(rng.standard_normal((B, L, 3 * DIMS[1])).astype(np.float32)).to(torch.float16).cuda()
    att = torch.empty((B, L, DIMS[1]), dtype=torch.float16, device="cuda")
    i = torch.arange(L)
    mask = enc.make_mask(i[None, :] > i[:, None])
    bias = enc.make_bias(alibi_bias(L, [2.0 ** -(h + 1) for h in range(H)]))
    zero = enc.make_bias(torch.zeros(H, L, L).masked_fill((i[None, :] > i[:, None])[None], float("-inf")))
    levels = {"attention": [("mask", lambda: enc.attention(qkv, out=att, mask=mask)), ("bias", lambda: enc.attention(qkv, out=att, mask=bias))],
              "forward": [("mask", lambda: enc(x, mask=mask)), ("bias", lambda: enc(x, mask=bias))]}
    rows, kernels = [], {}
    same = {"zero_bias_equals_mask_in_bits_attention": bool(torch.equal(enc.attention(qkv, mask=zero), enc.attention(qkv, mask=mask))),
            "zero_bias_equals_mask_in_bits_forward": bool(torch.equal(enc(x, mask=zero), enc(x, mask=mask)))}
    for level, sides in levels.items():
        for _ in range(2):                                   # warm-up of both sides
            for name, run in sides:
                run()
                kernels[level, name] = enc.last_attn_kernel
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
    by = {(r["level"], r["side"]): r for r in rows}
    cmp_row = {"comparison": True, **same, "allowed_pairs": mask.allowed, "bias_planes": bias.planes,
               "bias_bytes_per_launch_allocated": H * L * L * 4, "bias_bytes_per_launch_read": bias.allowed * H * 4,
               "ratio_of_medians_bias_over_mask_attention": round(by["attention", "bias"]["ms_median"] / by["attention", "mask"]["ms_median"], 3),
               "ratio_of_medians_bias_over_mask_forward": round(by["forward", "bias"]["ms_median"] / by["forward", "mask"]["ms_median"], 3)}
    print(json.dumps(cmp_row), flush=True)
    rows.append(cmp_row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    enc.close()


if __name__ == "__main__":
    main()
