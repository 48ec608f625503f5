"""One step of a windowed stream state (a ring cache, sliding-window attention) against one step of a state without a
window at the same absolute position, on ONE handle in ONE process (tools/bench_tf_stream.py's method): every side warmed,
alternating windows of `iters` calls, device events around the calls of a window; the result is printed as JSON lines and written to
--out.

    python tools/bench_tf_stream_window.py [--pairs 9] [--iters 5] [--out profiles/tf_stream_window_ab.json]

cfg5 (d = 384, 6 heads, 12 layers, f16), 256 tracks.  A window is `iters` consecutive steps of all 256 tracks; in front of every
window the tracks are put back to the side's position by a prefill outside the timed region.
  side A    a state without a window, capacity 2048, steps from position 2040: a wave walks about 2040 keys
  side B    a windowed state, W = capacity = 256, the tracks at the same absolute position 2040 and stepped there: 256 keys over the ring
  side C    a state without a window at position 255: the same key count (256 .. 256 + iters - 1) without a ring
  gate      the slowest window of B is faster than the fastest window of A (the margin of DESIGN.md 19).  Exit status 1 when missed.
  no gate   B against C: ratio of medians and both spreads, and whether B's median lies inside C's min .. max.
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

DIMS = (32, 384, 9, 6, 12, 1536)          # cfg5: in, d, out, heads, layers, ff
TRACKS, POS, CAP_A, WINDOW, POS_C, CAP_C = 256, 2040, 2048, 256, 255, 512


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_stream_window_ab.json"))
    a = ap.parse_args()
    if POS + a.iters > CAP_A:
        sys.exit(f"--iters {a.iters}: side A steps past its capacity {CAP_A}")
    # attn_tiled = 1: the put-back prefill of side A (256 x 2040 tokens) runs the streaming MFMA attention; no step depends on it
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=TRACKS * POS, attn_tiled=1)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    hist = torch.from_numpy(np.random.default_rng(1).standard_normal((TRACKS, POS + a.iters, DIMS[0])).astype(np.float32)).cuda()
    cols = [hist[:, t].contiguous() for t in range(POS + a.iters)]
    y = torch.empty(TRACKS, DIMS[2], device="cuda")
    big = torch.empty(TRACKS, POS, DIMS[2], device="cuda")
    past = {pos: hist[:, :pos].contiguous() for pos in (POS, POS_C)}
    sides = {"A": (enc.open_stream(TRACKS, CAP_A), POS), "B": (enc.open_stream(TRACKS, WINDOW, window=WINDOW), POS),
             "C": (enc.open_stream(TRACKS, CAP_C), POS_C)}

    def put_back(name):
        st, pos = sides[name]
        st.prefill(past[pos], out=big if pos == POS else None)
        torch.cuda.synchronize()
        assert st.position(0) == pos

    def step(name):
        st = sides[name][0]
        return lambda: st.step(cols[st.position(0)], out=y)

    for name in sides:                                       # warm-up of every side
        put_back(name)
        for _ in range(a.iters):
            step(name)()
    torch.cuda.synchronize()
    t = {name: [] for name in sides}
    for _ in range(a.pairs):
        for name in sides:
            put_back(name)
            t[name].append(timed(step(name), a.iters))
    res = {"measurement": "window", "dtype": "f16", "dims_in_d_out_heads_layers_ff": DIMS, "tracks": TRACKS, "pairs": a.pairs,
           "calls_per_window": a.iters,
           "A": dict(stats(t["A"]), window=0, capacity=CAP_A, step_positions=[POS, POS + a.iters - 1]),
           "B": dict(stats(t["B"]), window=WINDOW, capacity=WINDOW, step_positions=[POS, POS + a.iters - 1], keys_per_step=WINDOW),
           "C": dict(stats(t["C"]), window=0, capacity=CAP_C, step_positions=[POS_C, POS_C + a.iters - 1])}
    res["ratio_of_medians_A_over_B"] = round(res["A"]["ms_median"] / res["B"]["ms_median"], 2)
    res["ratio_of_medians_B_over_C"] = round(res["B"]["ms_median"] / res["C"]["ms_median"], 3)
    res["B_median_inside_C_min_max"] = res["C"]["ms_min"] <= res["B"]["ms_median"] <= res["C"]["ms_max"]
    res["condition_slowest_B_faster_than_fastest_A"] = res["B"]["ms_max"] < res["A"]["ms_min"]
    print(json.dumps(res), flush=True)
    for st, _ in sides.values():
        st.close()
    enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump([res], f, indent=1)
        f.write("\n")
    sys.exit(0 if res["condition_slowest_B_faster_than_fastest_A"] else 1)


if __name__ == "__main__":
    main()
