"""Per-launch times of the float32 MFMA trunk from a rocprofv3 kernel trace, and each conv's share of the 155 TFLOP/s that
v_mfma_f32_16x16x4_f32 sustains on an MI355X (algorithmic FLOPs of flope_launch_info over kernel time).

    rocprofv3 --kernel-trace --stats -d DIR -o f32m --output-format csv -- python tools/profile_f32m.py run B S
    python tools/profile_f32m.py digest DIR B S

`run`: one engine, streams = 1, two warm-up forwards and five traced ones.  `digest`: the conv_f32m_kernel launches of the trace in
start order, 20 per forward; per position the median over the last five forwards."""
import csv
import glob
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flope_amd.engine import PoseEngine  # noqa: E402
from flope_amd.weights import synthetic_state_dict  # noqa: E402

PEAK_TFLOPS = 155.0
FORWARDS = 5


def engine(B, S):
    e = PoseEngine(S, S, B, "f32m")
    e.set_option("streams", 1)
    e.load_state_dict(synthetic_state_dict(0))
    return e


def main():
    mode, B, S = sys.argv[1], int(sys.argv[-2]), int(sys.argv[-1])
    e = engine(B, S)
    torch.manual_seed(0)
    x = torch.rand(B, 3, S, S).cuda()
    R = torch.empty(B, 9, device="cuda")
    if mode == "run":
        for _ in range(2 + FORWARDS):
            e.forward_into(x, 0, None, R)
        torch.cuda.synchronize()
        return
    e.forward_into(x, 0, None, R)
    torch.cuda.synchronize()
    convs = [(layer, kern, f) for layer, kern, f in e.launch_info(B) if kern.startswith("conv_f32m_kernel")]
    f = glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(f)) if "conv_f32m_kernel" in r["Kernel_Name"])
    assert len(rows) == len(convs) * (2 + FORWARDS), (len(rows), len(convs))
    rows = rows[2 * len(convs):]
    print(f"rocprofv3 kernel trace, B = {B} x {S}^2, f32mfma = 1, streams = 1, median of {FORWARDS} forwards")
    tot_us, tot_f = 0.0, 0.0
    for i, (layer, kern, fl) in enumerate(convs):
        us = statistics.median((rows[k * len(convs) + i][1] - rows[k * len(convs) + i][0]) / 1e3 for k in range(FORWARDS))
        tot_us += us
        tot_f += fl
        print(f"  {layer:30s} {kern:32s} {us:9.1f} us  {fl / us / 1e6:6.1f} TFLOP/s  {100 * fl / us / 1e6 / PEAK_TFLOPS:5.1f} % of peak")
    print(f"  20 convs: {tot_us / 1e3:.3f} ms  {tot_f / tot_us / 1e6:6.1f} TFLOP/s  {100 * tot_f / tot_us / 1e6 / PEAK_TFLOPS:5.1f} % of peak")


if __name__ == "__main__":
    main()
