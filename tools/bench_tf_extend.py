"""extend() of m tokens per track against the only way to append them before it, m consecutive step() calls, on ONE handle in ONE
process (tools/bench_tf_stream.py's method): both sides warmed, alternating windows, device events around the
calls of a window; the result is printed as JSON lines and written to --out.

    python tools/bench_tf_extend.py [--pairs 9] [--out profiles/tf_extend_ab.json]
    python tools/bench_tf_extend.py --profile extend|steps [--repeats 3]   (under a kernel trace of its own: m = 8 from position 256 only)
    python tools/bench_tf_extend.py --digest STATS.csv                     (the per-kernel statistics of such a trace -> time per attention
                                                                            launch and the bytes per second it achieved; needs no device)

  cfg5 (d = 384, 6 heads, 12 layers, f16), 256 tracks, capacity 512.  A window is ONE append of m tokens to every track from position
  256 -- side "extend": one extend() of (256, m); side "steps": m step() calls of all 256 tracks.  The tracks are put back to 256
  tokens by a prefill outside the timed region, in front of every window.
  gate      m = 8 on the linear state: the slowest extend window is faster than the fastest window of 8 steps -- an ordering of the
            two sides' windows, no ratio and no margin.  Exit status 1 when it is missed.
  repeated  at m = 2 and m = 32, and on a windowed state (W = 128, capacity 512) at m = 8; the same condition, recorded.
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
TRACKS, POS, CAPACITY, WINDOW = 256, 256, 512, 128
CASES = ((8, 0), (2, 0), (32, 0), (8, WINDOW))      # (m, window); the first is the gate


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def digest(path):
    """per-kernel statistics of a kernel trace of --profile -> one JSON line per attention kernel of the append: time per launch, and
    bytes per second against the bytes of ONE pass over the cached rows (256 tracks x 256 rows of k | v, f16) -- what a step launch
    loads, and what an extend launch has to fetch once for the eight queries of a (track, head) that load it eight times"""
    import csv
    one_pass = TRACKS * POS * 2 * DIMS[1] * 2
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            kind = "tf_attn_extend" if "tf_attn_extend" in name else "tf_attn_step" if "tf_attn_step" in name else None
            if not kind:
                continue
            us = float(r["AverageNs"]) / 1e3
            loads = 8 if kind == "tf_attn_extend" else 1
            print(json.dumps({"kernel": kind, "launches": int(r["Calls"]), "us_per_launch": round(us, 1), "us_min": round(float(r["MinNs"]) / 1e3, 1),
                              "us_max": round(float(r["MaxNs"]) / 1e3, 1), "cache_bytes_one_pass": one_pass,
                              "TB_per_s_one_pass": round(one_pass / us / 1e6, 2), "cache_bytes_loaded": loads * one_pass,
                              "TB_per_s_loaded": round(loads * one_pass / us / 1e6, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", default=None, help="kernel statistics CSV of a trace of --profile: print time per attention launch and bytes per second")
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--profile", choices=("extend", "steps"), default=None, help="only run this side at m = 8 (for a kernel trace)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_extend_ab.json"))
    a = ap.parse_args()
    if a.digest:
        digest(a.digest)
        return
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=TRACKS * CAPACITY)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    hist = torch.from_numpy(np.random.default_rng(1).standard_normal((TRACKS, CAPACITY, DIMS[0])).astype(np.float32)).cuda()
    head = hist[:, :POS].contiguous()
    cols = [hist[:, t].contiguous() for t in range(POS, POS + 32)]
    y1 = torch.empty(TRACKS, DIMS[2], device="cuda")
    states = {0: enc.open_stream(TRACKS, CAPACITY), WINDOW: enc.open_stream(TRACKS, CAPACITY, window=WINDOW)}

    def put_back(st):
        st.prefill(head)
        torch.cuda.synchronize()

    def sides(st, m):
        chunk = hist[:, POS:POS + m].contiguous()
        ym = torch.empty(TRACKS, m, DIMS[2], device="cuda")

        def extend():
            st.extend(chunk, out=ym)

        def steps():
            for t in range(m):
                st.step(cols[t], out=y1)
        return extend, steps

    if a.profile:
        st = states[0]
        fn = sides(st, 8)[a.profile == "steps"]
        for _ in range(a.repeats):
            put_back(st)
            fn()
        torch.cuda.synchronize()
        # what the attention launches of one append read from the cache: per layer, tracks x 256 rows of k | v (f16) once per query for
        # the steps, once per workgroup's four queries at best for extend
        print(json.dumps({"profiled": a.profile, "m": 8, "from_position": POS, "appends": a.repeats, "layers": DIMS[4],
                          "cache_bytes_one_pass_per_layer": TRACKS * POS * 2 * DIMS[1] * 2}))
        return
    rows = []
    for m, window in CASES:
        st = states[window]
        extend, steps = sides(st, m)
        for _ in range(3):                                   # warm-up of both sides
            put_back(st)
            extend()
            put_back(st)
            steps()
        torch.cuda.synchronize()
        t = {"extend": [], "steps": []}
        for _ in range(a.pairs):
            put_back(st)
            t["extend"].append(timed(extend))
            put_back(st)
            t["steps"].append(timed(steps))
        row = {"measurement": "gate" if (m, window) == CASES[0] else "repeat", "dtype": "f16", "dims_in_d_out_heads_layers_ff": DIMS, "tracks": TRACKS,
               "capacity": CAPACITY, "window": window, "from_position": POS, "m": m, "pairs": a.pairs,
               "launches_extend": 2 + 8 * DIMS[4] + 2, "launches_steps": m * (2 + 7 * DIMS[4] + 1),
               "extend": stats(t["extend"]), "steps": stats(t["steps"])}
        row["ratio_of_medians_steps_over_extend"] = round(row["steps"]["ms_median"] / row["extend"]["ms_median"], 2)
        row["condition_slowest_extend_faster_than_fastest_steps"] = row["extend"]["ms_max"] < row["steps"]["ms_min"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    for st in states.values():
        st.close()
    enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    sys.exit(0 if rows[0]["condition_slowest_extend_faster_than_fastest_steps"] else 1)


if __name__ == "__main__":
    main()
