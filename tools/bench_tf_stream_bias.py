"""A stream state with a distance table (enc.open_stream(..., bias=table)) against the same state without one, on ONE
handle in ONE process (tools/bench_tf_stream.py's method): both sides warmed, alternating windows of `iters` calls, device events
around the calls of a window; the result is printed as JSON lines and written to --out.

    python tools/bench_tf_stream_bias.py [--pairs 9] [--iters 5] [--out profiles/tf_stream_bias_ab.json]

cfg5 (d = 384, 6 heads, 12 layers, f16), 256 tracks, per-head ALiBi 2^-(h + 1).  A window is `iters` consecutive calls on all 256
tracks; in front of every window the tracks are put back to the point's position by a prefill outside the timed region.
  side a    an unbiased state (tf_attn_step / tf_attn_extend as they were)
  side b    the biased state (their BIASED instantiations)
  points    step_linear   a step at position 255 of a linear state, capacity 512
            step_ring     a step at position 300 of a ring, W = capacity = 256: past the wrap
            extend8       extend() of 8 tokens per track behind 256, capacity 512
  no gate   the feature replaces nothing: median [min .. max] of both sides and the ratio of medians b / a are reported.
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
from flope_amd.tf_encoder import TransformerEncoder, alibi_distances  # noqa: E402
from oracle.tf_encoder_ref import synthetic_state_dict  # noqa: E402  (weights only; nothing is checked here)

DIMS = (32, 384, 9, 6, 12, 1536)          # cfg5: in, d, out, heads, layers, ff
TRACKS, CHUNK = 256, 8
POINTS = {"step_linear": dict(capacity=512, window=0, pos=255), "step_ring": dict(capacity=256, window=256, pos=300),
          "extend8": dict(capacity=512, window=0, pos=256)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_stream_bias_ab.json"))
    a = ap.parse_args()
    longest = max(p["pos"] for p in POINTS.values()) + CHUNK * a.iters
    if POINTS["extend8"]["pos"] + CHUNK * a.iters > POINTS["extend8"]["capacity"]:
        sys.exit(f"--iters {a.iters}: the extends pass their capacity")
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=TRACKS * longest)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    hist = torch.from_numpy(np.random.default_rng(1).standard_normal((TRACKS, longest, DIMS[0])).astype(np.float32)).cuda()
    cols = [hist[:, t].contiguous() for t in range(longest)]
    y = torch.empty(TRACKS, DIMS[2], device="cuda")
    y8 = torch.empty(TRACKS, CHUNK, DIMS[2], device="cuda")
    slopes = [2.0 ** -(h + 1) for h in range(DIMS[3])]
    out = []
    for name, p in POINTS.items():
        past = hist[:, :p["pos"]].contiguous()
        big = torch.empty(TRACKS, p["pos"], DIMS[2], device="cuda")
        table = alibi_distances(p["window"] or p["capacity"], slopes)
        sides = {"a": enc.open_stream(TRACKS, p["capacity"], window=p["window"]),
                 "b": enc.open_stream(TRACKS, p["capacity"], window=p["window"], bias=table)}
        plans = {s: (st.step_plan, st.extend_plan()) for s, st in sides.items()}
        assert plans == {"a": ("row", "row"), "b": ("biased", "biased")}, plans

        def put_back(st):
            st.prefill(past, out=big)
            torch.cuda.synchronize()
            assert st.position(0) == p["pos"]

        def call(st):
            if name == "extend8":
                return lambda: st.extend(hist[:, st.position(0):st.position(0) + CHUNK].contiguous(), out=y8)
            return lambda: st.step(cols[st.position(0)], out=y)

        for st in sides.values():                              # warm-up of both sides
            put_back(st)
            for _ in range(a.iters):
                call(st)()
        torch.cuda.synchronize()
        t = {s: [] for s in sides}
        for _ in range(a.pairs):
            for s, st in sides.items():
                put_back(st)
                t[s].append(timed(call(st), a.iters))
        res = {"measurement": "stream_bias", "point": name, "dtype": "f16", "dims_in_d_out_heads_layers_ff": DIMS, "tracks": TRACKS, "pairs": a.pairs,
               "calls_per_window": a.iters, "capacity": p["capacity"], "window": p["window"], "first_position": p["pos"],
               "tokens_per_call_and_track": CHUNK if name == "extend8" else 1, "table": "per-head ALiBi 2^-(h+1)",
               "a": dict(stats(t["a"]), plan=plans["a"][name == "extend8"]), "b": dict(stats(t["b"]), plan=plans["b"][name == "extend8"])}
        res["ratio_of_medians_b_over_a"] = round(res["b"]["ms_median"] / res["a"]["ms_median"], 3)
        res["b_median_inside_a_min_max"] = res["a"]["ms_min"] <= res["b"]["ms_median"] <= res["a"]["ms_max"]
        print(json.dumps(res), flush=True)
        out.append(res)
        for st in sides.values():
            st.close()
    enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
