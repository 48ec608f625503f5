"""One step of the streaming forward against the causal forward a live caller had to run for the same row before it, on ONE handle
in ONE process (tools/bench_tf_causal.py's method): both sides warmed, alternating windows, device events around the calls of a
window; the result is printed as JSON lines and written to --out.

    python tools/bench_tf_stream.py [--pairs 9] [--iters 5] [--out profiles/tf_stream_ab.json]
    python tools/bench_tf_stream.py --profile 511 [--repeats 3]      (under a kernel trace of its own: steps at one position only)

  gate      cfg5 (d = 384, 6 heads, 12 layers, f16), 256 tracks.  Side "step": a window is `iters` consecutive steps of all 256
            tracks from position 256 on (positions 256 .. 256 + iters - 1; the tracks are put back to 256 tokens by a prefill outside
            the timed region).  Side "forward": enc(x, is_causal=True) of (256, 257), whose last row is the first of those steps'
            rows.  Condition (the margin of DESIGN.md 19): the slowest step window is faster than the fastest forward window.
            Exit status 1 when it is missed.
  positions one step of 256 tracks at exactly position 0, 63, 255 and 511 of a state with capacity 512: `pairs` single calls each,
            the tracks put back in front of every call; recorded only.
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
TRACKS, GATE_POS, CAPACITY = 256, 256, 512
POSITIONS = (0, 63, 255, 511)


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
    ap.add_argument("--profile", type=int, default=-1, help="only run steps at this position (for a kernel trace)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_stream_ab.json"))
    a = ap.parse_args()
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=TRACKS * CAPACITY)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    hist = torch.from_numpy(np.random.default_rng(1).standard_normal((TRACKS, CAPACITY, DIMS[0])).astype(np.float32)).cuda()
    st = enc.open_stream(TRACKS, CAPACITY)
    y = torch.empty(TRACKS, DIMS[2], device="cuda")
    cols = [hist[:, t].contiguous() for t in range(CAPACITY)]

    def put_back(pos):
        if pos:
            st.prefill(hist[:, :pos])
        else:
            st.reset()
        torch.cuda.synchronize()

    def step():
        st.step(cols[st.position(0)], out=y)

    if a.profile >= 0:
        for _ in range(a.repeats):
            put_back(a.profile)
            step()
        torch.cuda.synchronize()
        cache_bytes = TRACKS * a.profile * 2 * DIMS[1] * 2
        print(json.dumps({"profiled_position": a.profile, "steps": a.repeats, "tf_attn_step_launches": a.repeats * DIMS[4],
                          "cache_bytes_read_per_launch": cache_bytes}))
        return
    xf = hist[:, :GATE_POS + 1].contiguous()
    forward = lambda: enc(xf, is_causal=True)
    for _ in range(3):                                       # warm-up of both sides
        forward()
        put_back(GATE_POS)
        for _ in range(a.iters):
            step()
    torch.cuda.synchronize()
    t = {"step": [], "forward": []}
    for _ in range(a.pairs):
        put_back(GATE_POS)
        t["step"].append(timed(step, a.iters))
        t["forward"].append(timed(forward, a.iters))
    gate = {"measurement": "gate", "dtype": "f16", "dims_in_d_out_heads_layers_ff": DIMS, "tracks": TRACKS, "capacity": CAPACITY,
            "step_positions": [GATE_POS, GATE_POS + a.iters - 1], "forward_batch_seq_len": [TRACKS, GATE_POS + 1], "pairs": a.pairs,
            "calls_per_window": a.iters, "launches_per_step": 2 + 7 * DIMS[4] + 1, "step": stats(t["step"]), "forward": stats(t["forward"])}
    gate["ratio_of_medians_forward_over_step"] = round(gate["forward"]["ms_median"] / gate["step"]["ms_median"], 2)
    gate["condition_slowest_step_faster_than_fastest_forward"] = gate["step"]["ms_max"] < gate["forward"]["ms_min"]
    print(json.dumps(gate), flush=True)
    rows = [gate]
    for pos in POSITIONS:
        put_back(pos)
        step()                                               # warm-up at this position
        v = []
        for _ in range(a.pairs):
            put_back(pos)
            v.append(timed(step, 1))
        row = {"measurement": "position", "position": pos, "tracks": TRACKS, "capacity": CAPACITY, "single_calls": a.pairs, "step": stats(v),
               "cache_bytes_read_per_step": DIMS[4] * TRACKS * pos * 2 * DIMS[1] * 2}
        print(json.dumps(row), flush=True)
        rows.append(row)
    st.close()
    enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    sys.exit(0 if gate["condition_slowest_step_faster_than_fastest_forward"] else 1)


if __name__ == "__main__":
    main()
