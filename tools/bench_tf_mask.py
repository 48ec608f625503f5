"""A compiled attention mask against the forwards that can say the same thing, on ONE handle in ONE process (tools/bench_tf_attn.py's
method): every side warmed, alternating windows, device events around `iters` calls per window; one JSON line per side
and one for the comparison, all of them also written to --out.

    python tools/bench_tf_mask.py [--pairs 9] [--iters 5] [--out profiles/tf_mask_ab.json]

The handle is the build-defined cfg5 (d = 384, 6 heads, 12 layers, f16) with option generic = 1, so that every side runs the same
family of kernel, at B = 64, L = 256:

  dense      (a) enc(x): tf_attn_generic over all 256 keys
  clear      (b) enc(x, mask=<compiled all-clear mask>): tf_attn_masked over all 256 keys -- the cost of the bit tests on a mask that
             masks nothing
  blocks     (c) enc(x, mask=<block-diagonal, 8 blocks of 32>): tf_attn_masked over an eighth of the keys
  lengths    (d) the same tokens as 512 sequences of 32 through lengths=: the way to say (c) without a mask

GATED: (c) does an eighth of (a)'s key work, so its slowest window must be faster than (a)'s fastest window; exit status 1 when it is
missed.  (b) against (a) and (c) against (d) are recorded only.
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

DIMS = (32, 384, 9, 6, 12, 1536)
B, L, BLOCK = 64, 256, 32


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_mask_ab.json"))
    a = ap.parse_args()
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=B * L)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    enc.set_option("generic", 1)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, L, DIMS[0])).astype(np.float32)).cuda()
    xs = x.reshape(B * L // BLOCK, BLOCK, DIMS[0]).contiguous()
    lens = [BLOCK] * (B * L // BLOCK)
    clear = enc.make_mask(torch.zeros(L, L, dtype=torch.bool))
    i = torch.arange(L)
    blocks = enc.make_mask((i[:, None] // BLOCK) != (i[None, :] // BLOCK))
    sides = [("dense", lambda: enc(x)), ("clear", lambda: enc(x, mask=clear)), ("blocks", lambda: enc(x, mask=blocks)),
             ("lengths", lambda: enc(xs, lengths=lens))]
    out = {}
    for _ in range(2):                                       # warm-up of every side
        for name, run in sides:
            out[name] = run()
    torch.cuda.synchronize()
    same = {"clear_equals_dense_in_bits": bool(torch.equal(out["clear"], out["dense"])),
            "blocks_equals_lengths_in_bits": bool(torch.equal(out["blocks"].reshape(-1), out["lengths"].reshape(-1)))}
    t = {name: [] for name, _ in sides}
    for _ in range(a.pairs):
        for name, run in sides:
            t[name].append(timed(run, a.iters))
    rows = []
    flops = {"dense": enc.flops(B, L), "clear": enc.flops(B, L, mask=clear), "blocks": enc.flops(B, L, mask=blocks),
             "lengths": enc.flops(len(lens), BLOCK, lengths=lens)}
    for name, _ in sides:
        row = {"side": name, "dtype": "f16", "generic": 1, "dims_in_d_out_heads_layers_ff": DIMS, "batch": B, "seq_len": L, "pairs": a.pairs,
               "calls_per_window": a.iters, **stats(t[name])}
        row["tflops"] = round(flops[name] / row["ms_median"] / 1e9, 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
    by = {r["side"]: r for r in rows}
    cmp_row = {"comparison": True, **same,
               "allowed_pairs": {"clear": clear.allowed, "blocks": blocks.allowed},
               "ratio_of_medians_clear_over_dense": round(by["clear"]["ms_median"] / by["dense"]["ms_median"], 3),
               "ratio_of_medians_blocks_over_lengths": round(by["blocks"]["ms_median"] / by["lengths"]["ms_median"], 3),
               "ratio_of_medians_blocks_over_dense": round(by["blocks"]["ms_median"] / by["dense"]["ms_median"], 3),
               "slowest_blocks_over_fastest_dense": round(by["blocks"]["ms_max"] / by["dense"]["ms_min"], 3),
               "condition_slowest_blocks_faster_than_fastest_dense": by["blocks"]["ms_max"] < by["dense"]["ms_min"]}
    print(json.dumps(cmp_row), flush=True)
    rows.append(cmp_row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    enc.close()
    sys.exit(0 if cmp_row["condition_slowest_blocks_faster_than_fastest_dense"] else 1)


if __name__ == "__main__":
    main()
