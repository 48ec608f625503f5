"""Option mask_mfma against the path the same call takes without it, on ONE handle in ONE process (tools/bench_tf_attn.py's method,
DESIGN.md 24): every side warmed, alternating windows, device events around `iters` calls per window; one JSON line per side and level
and one for the comparison, all of them also written to --out.

    python tools/bench_tf_mask16.py [--pairs 9] [--iters 5] [--out profiles/tf_mask16_ab.json]

The handle is the build-defined cfg5 (d = 384, 6 heads of 64, 12 layers, f16) at B = 4, L = 2048 under a block-diagonal mask of 16
blocks of 128 tokens (short tracks packed into one row), timed at two levels: enc.attention alone and the 12-layer forward.

  A  generic   mask_mfma = 0: tf_attn_masked, what this very call runs without the option
  B  mfma      mask_mfma = 1: tf_attn_tiled_masked over the mask's tile map
  C  lengths   the same tokens as 64 sequences of 128 through lengths= on tf_attn_tiled: the way to say the mask without a mask
  D  dense     enc(x) on tf_attn_tiled: all 2048 keys
  E  clear     a compiled all-clear mask under mask_mfma = 1: what the class test costs when nothing is masked (against D)

GATED: B's slowest window must be faster than A's fastest window at both levels; exit status 1 when it is missed.  Every other ratio is
recorded only, beside the mask's tile_stats (blocks listed of query_blocks * ceil(L / 64)).
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
B, L, BLOCK = 4, 2048, 128


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_mask16_ab.json"))
    a = ap.parse_args()
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=B * L, attn_tiled=2)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((B, L, DIMS[0])).astype(np.float32)).cuda()
    xs = x.reshape(B * L // BLOCK, BLOCK, DIMS[0]).contiguous()
    qkv = torch.from_numpy(rng.standard_normal((B, L, 3 * DIMS[1])).astype(np.float32)).to(torch.float16).cuda()
    qs = qkv.reshape(B * L, 3 * DIMS[1])
    lens = [BLOCK] * (B * L // BLOCK)
    i = torch.arange(L)
    blocks = enc.make_mask((i[:, None] // BLOCK) != (i[None, :] // BLOCK))
    clear = enc.make_mask(torch.zeros(L, L, dtype=torch.bool))

    def masked(opt, m, at):
        def run():
            enc.set_option("mask_mfma", opt)
            return enc.attention(qkv, mask=m) if at else enc(x, mask=m)
        return run

    kernels = {}
    levels = {
        "attention": [("A", masked(0, blocks, True)), ("B", masked(1, blocks, True)), ("C", lambda: enc.attention(qs, lengths=lens)),
                      ("D", lambda: enc.attention(qkv)), ("E", masked(1, clear, True))],
        "forward": [("A", masked(0, blocks, False)), ("B", masked(1, blocks, False)), ("C", lambda: enc(xs, lengths=lens)),
                    ("D", lambda: enc(x)), ("E", masked(1, clear, False))],
    }
    flops = {"A": enc.flops(B, L, mask=blocks), "B": enc.flops(B, L, mask=blocks), "C": enc.flops(len(lens), BLOCK, lengths=lens),
             "D": enc.flops(B, L), "E": enc.flops(B, L, mask=clear)}
    rows, cmp_row = [], {"comparison": True, "tile_stats": {"blocks": blocks.tile_stats, "clear": clear.tile_stats},
                         "blocks_of_the_full_grid": ((L + 127) // 128) * ((L + 63) // 64),
                         "allowed_pairs": {"blocks": blocks.allowed, "clear": clear.allowed}}
    ok = True
    for level, sides in levels.items():
        out = {}
        for _ in range(2):                                   # warm-up of every side
            for name, run in sides:
                out[name] = run()
                if level == "attention":
                    kernels[name] = enc.last_attn_kernel
        torch.cuda.synchronize()
        cmp_row[level + "_B_equals_C_in_bits"] = bool(torch.equal(out["B"].reshape(-1), out["C"].reshape(-1)))
        cmp_row[level + "_E_equals_D_in_bits"] = bool(torch.equal(out["E"], out["D"]))
        t = {name: [] for name, _ in sides}
        for _ in range(a.pairs):
            for name, run in sides:
                t[name].append(timed(run, a.iters))
        by = {}
        for name, _ in sides:
            row = {"level": level, "side": name, "dtype": "f16", "attn_kernel": kernels.get(name), "dims_in_d_out_heads_layers_ff": DIMS, "batch": B,
                   "seq_len": L, "block": BLOCK, "pairs": a.pairs, "calls_per_window": a.iters, **stats(t[name])}
            if level == "forward":
                row["tflops"] = round(flops[name] / row["ms_median"] / 1e9, 2)
            print(json.dumps(row), flush=True)
            rows.append(row)
            by[name] = row
        for num, den in (("B", "A"), ("B", "C"), ("B", "D"), ("E", "D")):
            cmp_row[f"{level}_ratio_of_medians_{num}_over_{den}"] = round(by[num]["ms_median"] / by[den]["ms_median"], 4)
        cmp_row[level + "_slowest_B_over_fastest_A"] = round(by["B"]["ms_max"] / by["A"]["ms_min"], 4)
        cmp_row[level + "_condition_slowest_B_faster_than_fastest_A"] = by["B"]["ms_max"] < by["A"]["ms_min"]
        ok = ok and cmp_row[level + "_condition_slowest_B_faster_than_fastest_A"]
    print(json.dumps(cmp_row), flush=True)
    rows.append(cmp_row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    enc.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
