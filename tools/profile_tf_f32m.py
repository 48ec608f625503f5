"""Per-launch times of the float32 MFMA encoder from a rocprofv3 kernel trace, and each launch's share of the 155 TFLOP/s that
v_mfma_f32_16x16x4_f32 sustains on an MI355X (algorithmic FLOPs over kernel time); LayerNorm's share of the forward.

    rocprofv3 --kernel-trace --stats -d DIR -o tf --output-format csv -- python tools/profile_tf_f32m.py run SHAPE
    python tools/profile_tf_f32m.py digest DIR SHAPE > profiles/tf_f32m_rocprof_per_launch_SHAPE.txt

`run`: one f32m handle, two warm-up forwards and five traced ones.  `digest` (needs no GPU): the launches of the trace in start
order, one forward = embedding, per layer (in_proj, attention, out_proj, LayerNorm, linear1, linear2, LayerNorm), out_layer; per
kind the median over the layers and the last five forwards."""
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_tf_f32m import PEAK_TFLOPS, SHAPES  # noqa: E402

FORWARDS = 5


def launches(dims, B, L):
    """(label, FLOPs) of one forward in launch order."""
    din, d, dout, H, nl, ff = dims
    M = B * L
    per_layer = [("in_proj", 2.0 * M * d * 3 * d), ("attention", 4.0 * M * L * d), ("out_proj + residual", 2.0 * M * d * d), ("LayerNorm 1", 0.0),
                 ("linear1 + ReLU", 2.0 * M * d * ff), ("linear2 + residual", 2.0 * M * ff * d), ("LayerNorm 2", 0.0)]
    return [("embedding", 2.0 * M * din * d)] + per_layer * nl + [("out_layer", 2.0 * M * d * dout)]


def run(name):
    import numpy as np
    import torch
    from flope_amd.tf_encoder import TransformerEncoder
    from oracle.tf_encoder_ref import synthetic_state_dict
    dims, B, L, _ = SHAPES[name]
    sd = synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
    enc = TransformerEncoder(*dims, dtype="f32m", max_tokens=B * L)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, L, dims[0])).astype(np.float32)).cuda()
    for _ in range(2 + FORWARDS):
        enc(x)
    torch.cuda.synchronize()
    enc.close()


def digest(path, name):
    dims, B, L, note = SHAPES[name]
    seq = launches(dims, B, L)
    f = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))
                  if "tf_" in r["Kernel_Name"])
    assert len(rows) == len(seq) * (2 + FORWARDS), (len(rows), len(seq))
    rows = rows[2 * len(seq):]
    print(f"rocprofv3 kernel trace, {name}: {note}; dims {dims}, B = {B}, L = {L}, f32mfma = 1; median over layers and {FORWARDS} forwards")
    us, kern, flops, order = {}, {}, {}, []
    for k in range(FORWARDS):
        for i, (label, fl) in enumerate(seq):
            s, e, kn = rows[k * len(seq) + i]
            if label not in us:
                order.append(label)
            us.setdefault(label, []).append((e - s) / 1e3)
            kern[label], flops[label] = kn.split("(")[0].replace("(anonymous namespace)::", "").replace("void ", ""), fl
    count = {label: sum(1 for l, _ in seq if l == label) for label in order}
    total = sum(statistics.median(us[l]) * count[l] for l in order)
    for l in order:
        m = statistics.median(us[l])
        tf = flops[l] / m / 1e6
        perf = f"{tf:7.1f} TFLOP/s {100 * tf / PEAK_TFLOPS:5.1f} % of peak" if flops[l] else " " * 32
        print(f"  {l:22s} {kern[l][:44]:44s} x{count[l]:3d} {m:10.1f} us  {perf}  {100 * m * count[l] / total:5.1f} % of the forward")
    fl_all = sum(fl for _, fl in seq)
    ln = sum(statistics.median(us[l]) * count[l] for l in order if l.startswith("LayerNorm"))
    print(f"  forward: {total / 1e3:.3f} ms of kernel time, {fl_all / total / 1e6:.1f} TFLOP/s = {100 * fl_all / total / 1e6 / PEAK_TFLOPS:.1f} % of peak; LayerNorm {100 * ln / total:.1f} % of it")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        digest(sys.argv[2], sys.argv[3])
