"""Float32 encoder: the generic kernels (f32mfma = 0, the parent's float32 mode) against tf_linear_f32m / tf_attn_f32m (f32mfma = 1)
on ONE handle in ONE process, the option flipped between forwards.  Device events around whole forwards, both sides warmed at each
shape, alternating pairs; per shape one JSON line with the median and the spread (min .. max) of each side, all of them also
written to --out.

    python tools/bench_tf_f32m.py [--pairs 5] [--shapes throughput,toy,long] [--lds 84[,0,...]] [--out profiles/tf_f32m_ab.json]

Shapes: `throughput` is the build-defined cfg5 shape (B = 256, L = 257, d = 384, 6 heads, 12 layers, ff = 1536; not from the
reference), `toy` the reference's own configuration (B = 8, L = 10: a measurement of launch overhead, 16 launches of a few
microseconds of work), `long` a sequence longer than the 16-bit attention kernel takes (B = 16, L = 1024, d = 256, 4 heads, 2 layers).
--lds: KiB of untouched LDS every tf_linear_f32m launch reserves (option f32mlds; more than 80 = one workgroup per CU); several
values measure the f32m side once per value, in the same alternation."""
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

PEAK_TFLOPS = 155.0
SHAPES = {  # name: (dims (in, d, out, heads, layers, ff), B, L, note)
    "throughput": ((32, 384, 9, 6, 12, 1536), 256, 257, "build-defined cfg5 throughput shape (not from the reference)"),
    "toy": ((16, 32, 9, 4, 2, 64), 8, 10, "the reference's toy: a measurement of launch overhead, not of the kernels"),
    "long": ((32, 256, 9, 4, 2, 1024), 16, 1024, "L > 512: more keys than the 16-bit attention kernel takes"),
}


def timed(enc, x, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        enc(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--shapes", default="throughput,toy,long")
    ap.add_argument("--lds", default="", help="KiB values of option f32mlds to measure (default: the handle's own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_f32m_ab.json"))
    a = ap.parse_args()
    rows = []
    for name in a.shapes.split(","):
        dims, B, L, note = SHAPES[name]
        sd = synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
        enc = TransformerEncoder(*dims, dtype="f32", max_tokens=B * L)
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, L, dims[0])).astype(np.float32)).cuda()
        default_lds = enc.set_option("f32mlds", 0)
        enc.set_option("f32mlds", default_lds)
        lds = [int(v) for v in a.lds.split(",")] if a.lds else [default_lds]
        sides = [("generic", 0, default_lds)] + [(f"f32m_lds{v}" if a.lds else "f32m", 1, v) for v in lds]
        iters = {s[0]: (1 if s[1] == 0 and name != "toy" else 3 if name != "toy" else 50) for s in sides}
        for _ in range(2):                                   # warm-up of every side
            for side, mode, v in sides:
                enc.set_option("f32mfma", mode); enc.set_option("f32mlds", v)
                enc(x)
        torch.cuda.synchronize()
        ms = {s[0]: [] for s in sides}
        for _ in range(a.pairs):
            for side, mode, v in sides:
                enc.set_option("f32mfma", mode); enc.set_option("f32mlds", v)
                ms[side].append(timed(enc, x, iters[side]))
        fl = enc.flops(B, L)
        row = {"shape": name, "note": note, "dims_in_d_out_heads_layers_ff": dims, "batch": B, "seq_len": L, "pairs": a.pairs,
               "gflop_per_forward": round(fl / 1e9, 3)}
        for side, _, _ in sides:
            med = statistics.median(ms[side])
            row[side] = {"ms_median": round(med, 4), "ms_min": round(min(ms[side]), 4), "ms_max": round(max(ms[side]), 4),
                         "tokens_per_s": round(B * L / med * 1e3), "tflops": round(fl / med / 1e9, 2),
                         "share_of_155_tflops_peak": round(fl / med / 1e9 / PEAK_TFLOPS, 4)}
            if side != "generic":
                row[side]["ratio_of_medians_vs_generic"] = round(row["generic"]["ms_median"] / med, 2)
                row[side]["fastest_generic_over_slowest_f32m"] = round(row["generic"]["ms_min"] / max(ms[side]), 2)
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
