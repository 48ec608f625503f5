"""Option extend_mfma against the kernel it replaces, on ONE f16 handle in ONE process (tools/bench_tf_extend.py's method; DESIGN.md 29 /
33): the option is flipped between alternating windows, both sides warmed, device events around every call, the tracks put back by a
prefill outside the timed region in front of every call.  A window is `calls` calls; its figure is the mean of their times.  The result
is printed as JSON lines and written to --out.

    python tools/bench_tf_extend_mfma.py [--pairs 9] [--calls 5] [--out profiles/tf_extend_mfma_ab.json]
    python tools/bench_tf_extend_mfma.py --profile 0|1 [--repeats 3]   (under a kernel trace of its own: m = 8 from position 256 only)
    python tools/bench_tf_extend_mfma.py --digest STATS.csv --option 0|1 [--trace-out profiles/tf_extend_mfma_trace.json]
                                                                       (the per-kernel statistics of such a trace -> time per attention
                                                                        launch and the bytes per second it achieved, printed and kept in
                                                                        --trace-out beside the other option's records; needs no device)

  cfg5 (d = 384, 6 heads, 12 layers, f16; the prefills that put the tracks back run with attn_tiled = 1, which no extend reads).
  linear    256 tracks, capacity 512: one extend() of m = 2, 8, 32 tokens per track from position 256, and of m = 16 from position 496;
  windowed  256 tracks, capacity 512, W = 128: m = 8 from position 256.
  gate      at m = 8 and m = 32 (linear) the slowest option-1 window is faster than the fastest option-0 window -- an ordering of the two
            sides' windows, no ratio and no margin.  Exit status 1 when one is missed.  Option 0 is the parent's kernel on the same box.
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
TRACKS, CAPACITY, WINDOW = 256, 512, 128
ROWS = (("linear", 256, 2), ("linear", 256, 8), ("linear", 256, 32), ("linear", 496, 16), ("windowed", 256, 8))      # state, position, m
GATES = (("linear", 256, 8), ("linear", 256, 32))
PROFILE = ("linear", 256, 8)
KERNELS = ("tf_attn16_extend", "tf_attn_extend_split", "tf_attn_extend")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def owed_bytes(pos, m):
    """what one attention launch owes HBM in one pass: every track's cached k | v rows, the chunk's q | k | v rows and its output rows"""
    return TRACKS * (pos * 2 * DIMS[1] + m * 3 * DIMS[1] + m * DIMS[1]) * 2


def digest(path, option, out):
    """per-kernel statistics of a kernel trace of --profile `option` -> one JSON line per extend attention kernel: time per launch and
    bytes per second against the one pass a launch owes HBM.  `out` keeps them: the records of this option are replaced, the other
    option's stay."""
    import csv
    owed = owed_bytes(PROFILE[1], PROFILE[2])
    records = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            kind = next((k for k in KERNELS if k + "<" in r["Name"] or f"{len(k)}{k}I" in r["Name"]), None)      # demangled or mangled
            if not kind:
                continue
            us = float(r["AverageNs"]) / 1e3
            records.append({"measurement": "kernel_trace", "profiled_option": option, "tracks": TRACKS, "position": PROFILE[1], "tokens_per_track": PROFILE[2],
                            "kernel": kind, "launches": int(r["Calls"]), "us_per_launch": round(us, 1), "us_min": round(float(r["MinNs"]) / 1e3, 1),
                            "us_max": round(float(r["MaxNs"]) / 1e3, 1), "bytes_owed_one_pass": owed, "TB_per_s_of_one_pass": round(owed / us / 1e6, 2)})
            print(json.dumps(records[-1]))
    kept = []
    if os.path.exists(out):
        with open(out) as f:
            kept = [r for r in json.load(f) if r.get("profiled_option") != option]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(sorted(kept + records, key=lambda r: r["profiled_option"]), f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--digest", default=None, help="kernel statistics CSV of a trace of --profile: print time per attention launch and bytes per second")
    ap.add_argument("--option", type=int, choices=(0, 1), default=None, help="with --digest: the option the trace was taken under")
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "tf_extend_mfma_trace.json"))
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--profile", type=int, choices=(0, 1), default=None, help="only run m = 8 from position 256 under this option (for a kernel trace)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tf_extend_mfma_ab.json"))
    a = ap.parse_args()
    if a.digest:
        if a.option is None:
            ap.error("--digest needs --option: the option the trace was taken under")
        digest(a.digest, a.option, a.trace_out)
        return
    enc = TransformerEncoder(*DIMS, dtype="f16", max_tokens=TRACKS * CAPACITY, attn_tiled=1)
    sd = synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    hist = torch.from_numpy(np.random.default_rng(1).standard_normal((TRACKS, CAPACITY, DIMS[0])).astype(np.float32)).cuda()
    states = {"linear": enc.open_stream(TRACKS, CAPACITY)}
    if a.profile is None:
        states["windowed"] = enc.open_stream(TRACKS, CAPACITY, window=WINDOW)
    assert states["linear"].extend_plan() == "row"

    def put_back(k, pos):
        states[k].prefill(hist[:, :pos])
        torch.cuda.synchronize()

    def extend_of(k, pos, m):
        chunk = hist[:, pos:pos + m].contiguous()
        ym = torch.empty(TRACKS, m, DIMS[2], device="cuda")
        return lambda: states[k].extend(chunk, out=ym)

    if a.profile is not None:
        enc.set_option("extend_mfma", a.profile)
        fn = extend_of(*PROFILE)
        for _ in range(a.repeats):
            put_back(PROFILE[0], PROFILE[1])
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"profiled_option": a.profile, "position": PROFILE[1], "tokens_per_track": PROFILE[2], "calls": a.repeats, "layers": DIMS[4],
                          "plan": states["linear"].extend_plan(), "bytes_owed_one_pass_per_launch": owed_bytes(PROFILE[1], PROFILE[2])}))
        return

    rows = []
    for k, pos, m in ROWS:
        fn = extend_of(k, pos, m)

        def window(opt):
            enc.set_option("extend_mfma", opt)
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
        row = {"measurement": "gate" if (k, pos, m) in GATES else "recorded", "call": "extend", "dtype": "f16", "dims_in_d_out_heads_layers_ff": DIMS,
               "tracks": TRACKS, "capacity": CAPACITY, "window": WINDOW if k == "windowed" else 0, "position": pos, "tokens_per_track": m,
               "windows_per_side": a.pairs, "calls_per_window": a.calls, "option_0": stats(t[0]), "option_1": stats(t[1])}
        row["ratio_of_medians_option_0_over_option_1"] = round(row["option_0"]["ms_median"] / row["option_1"]["ms_median"], 3)
        row["condition_slowest_option_1_faster_than_fastest_option_0"] = row["option_1"]["ms_max"] < row["option_0"]["ms_min"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    enc.set_option("extend_mfma", 0)
    for st in states.values():
        st.close()
    enc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
    sys.exit(0 if all(r["condition_slowest_option_1_faster_than_fastest_option_0"] for r in rows if r["measurement"] == "gate") else 1)


if __name__ == "__main__":
    main()
