"""Option step_split against the row kernel it replaces, on ONE f16 handle in ONE process (tools/bench_tf_stream.py's method; DESIGN.md
25 / 31): the option is flipped between alternating windows, both sides warmed, device events around every call, the tracks put back
by a prefill (position 0: a reset) outside the timed region in front of every call.  A window is `calls` calls at one position; its
figure is the mean of their times.  The result is printed as JSON lines and written to --out.

    python tools/bench_tf_step_split.py [--pairs 9] [--calls 5] [--out profiles/tf_step_split_ab.json]
    python tools/bench_tf_step_split.py --profile 0|1 [--repeats 3]   (under a kernel trace of its own: steps at position 511 only)
    python tools/bench_tf_step_split.py --digest STATS.csv            (the per-kernel statistics of such a trace -> time per attention
                                                                       launch and the bytes per second it achieved; needs no device)

  cfg5 (d = 384, 6 heads, 12 layers, f16; the prefills that put the tracks back run with attn_tiled = 1, which no step reads).
  steps     256 tracks, capacity 512: one step of every track at position 0, 63, 255 and 511;
            64 tracks, capacity 4096: at position 1023 and 4095.
  extend    256 tracks, capacity 512: one extend() of 16 tokens per track from position 496.
  gate      at position 511 the slowest option-1 window is faster than the fastest option-0 window -- an ordering of the two sides'
            windows, no ratio and no margin.  Exit status 1 when it is missed.  Option 0 is the parent's kernel on the same box.
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
STATES = {"short": (256, 512), "long": (64, 4096)}          # tracks, capacity
STEPS = (("short", 0), ("short", 63), ("short", 255), ("short", 511), ("long", 1023), ("long", 4095))
GATE = ("short", 511)
EXTEND_POS, EXTEND_M = 496, 16


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
    """per-kernel statistics of a kernel trace of --profile -> one JSON line per step attention kernel: time per launch and bytes per
    second against the cache rows a launch at position 511 loads (256 tracks x 511 rows of k | v, f16)"""
    import csv
    loaded = STATES["short"][0] * GATE[1] * 2 * DIMS[1] * 2
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            kind = "tf_attn_step_split" if "tf_attn_step_split" in name else "tf_attn_step" if "tf_attn_step" in name else None
            if not kind:
                continue
            us = float(r["AverageNs"]) / 1e3
            print(json.dumps({"kernel": kind, "launches": int(r["Calls"]), "us_per_launch": round(us, 1), "us_min": round(float(r["MinNs"]) / 1e3, 1),
                              "us_max": round(float(r["MaxNs"]) / 1e3, 1), "cache_bytes_loaded": loaded, "TB_per_s": round(loaded / us / 1e6, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", default=None, help="kernel statistics CSV of a trace of --profile: print time per attention launch and bytes per second")
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--profile", type=int, choices=(0, 1), default=None, help="only run steps at position 511 under this option (for a kernel trace)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_step_split_ab.json"))
    a = ap.parse_args()
    if a.digest:
        digest(a.digest)
        return
    names = ("short",) if a.profile is not None else tuple(STATES)
    max_tokens = max(STATES[k][0] * STATES[k][1] for k in names)
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=max_tokens, attn_tiled=1)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    rng = np.random.default_rng(1)
    hist, states, y1 = {}, {}, {}
    for k in names:
        tracks, capacity = STATES[k]
        hist[k] = torch.from_numpy(rng.standard_normal((tracks, capacity, DIMS[0])).astype(np.float32)).cuda()
        states[k] = enc.open_stream(tracks, capacity)
        y1[k] = torch.empty(tracks, DIMS[2], device="cuda")
    assert states["short"].step_plan == "row"

    def put_back(k, pos):
        if pos:
            states[k].prefill(hist[k][:, :pos])
        else:
            states[k].reset()
        torch.cuda.synchronize()

    def step_of(k, pos):
        col = hist[k][:, pos].contiguous()
        return lambda: states[k].step(col, out=y1[k])

    if a.profile is not None:
        enc.set_option("step_split", a.profile)
        fn = step_of(*GATE)
        for _ in range(a.repeats):
            put_back(*GATE)
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"profiled_option": a.profile, "position": GATE[1], "steps": a.repeats, "layers": DIMS[4], "plan": states["short"].step_plan,
                          "cache_bytes_loaded_per_launch": STATES["short"][0] * GATE[1] * 2 * DIMS[1] * 2}))
        return

    chunk = hist["short"][:, EXTEND_POS:EXTEND_POS + EXTEND_M].contiguous()
    ym = torch.empty(STATES["short"][0], EXTEND_M, DIMS[2], device="cuda")
    work = [("step", k, pos, step_of(k, pos)) for k, pos in STEPS]
    work.append(("extend", "short", EXTEND_POS, lambda: states["short"].extend(chunk, out=ym)))
    rows = []
    for what, k, pos, fn in work:
        def window(opt):
            enc.set_option("step_split", opt)
            t = []
            for _ in range(a.calls):
                put_back(k, pos)
                t.append(timed(fn))
            return sum(t) / len(t)
        for opt in (0, 1, 0, 1):                             # warm-up of both sides
            window(opt)
        t = {0: [], 1: []}
        for _ in range(a.pairs):
            for opt in (0, 1):
                t[opt].append(window(opt))
        row = {"measurement": "gate" if (what, k, pos) == ("step",) + GATE else "recorded", "call": what, "dtype": "f16", "dims_in_d_out_heads_layers_ff": DIMS,
               "tracks": STATES[k][0], "capacity": STATES[k][1], "position": pos, "tokens_per_track": EXTEND_M if what == "extend" else 1,
               "windows_per_side": a.pairs, "calls_per_window": a.calls, "option_0": stats(t[0]), "option_1": stats(t[1])}
        row["ratio_of_medians_option_0_over_option_1"] = round(row["option_0"]["ms_median"] / row["option_1"]["ms_median"], 3)
        row["condition_slowest_option_1_faster_than_fastest_option_0"] = row["option_1"]["ms_max"] < row["option_0"]["ms_min"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    enc.set_option("step_split", 0)
    for st in states.values():
        st.close()
    enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    gate = [r for r in rows if r["measurement"] == "gate"][0]
    sys.exit(0 if gate["condition_slowest_option_1_faster_than_fastest_option_0"] else 1)


if __name__ == "__main__":
    main()
