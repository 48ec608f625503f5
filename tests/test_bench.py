"""bench.py itself: the plain run is the headline only, and `--dump-outputs` writes what the timed path computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_float32_and_seeded_sample_within_the_limit(tmp_path, monkeypatch):
    import bench
    a = torch.arange(64 * 16, dtype=torch.float16).view(64, 16)
    b = torch.arange(64 * 9, dtype=torch.float64).view(64, 9)
    bench.dump_outputs(str(tmp_path / "full"), {"poses": a, "R": b})
    pa, pb = np.load(tmp_path / "full" / "poses.npy"), np.load(tmp_path / "full" / "R.npy")
    assert pa.dtype == np.float32 and pb.dtype == np.float32
    assert np.array_equal(pa, a.float().numpy()) and np.array_equal(pb, b.float().numpy())
    limit = (pa.nbytes + pb.nbytes) // 4                          # a quarter of what the two arrays hold
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), {"poses": a, "R": b})
    sa, sb = np.load(tmp_path / "s1" / "poses.npy"), np.load(tmp_path / "s1" / "R.npy")
    assert sa.nbytes + sb.nbytes <= limit and sa.shape[1] == 16 and sb.shape[1] == 9
    assert (np.diff(sa[:, 0]) > 0).all()                          # whole rows, in order
    assert np.array_equal(sa, np.load(tmp_path / "s2" / "poses.npy"))   # the same sample every time


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    from flope_amd import engine as E
    out = _plain_run(tmp_path / "a")
    assert out["metric"] == "poses_per_sec" and out["unit"] == "poses/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f16" and out["steps"] == 3 and out["warmup"] == 1
    assert abs(out["value"] - 3 * 256 / (out["ms_per_step"] * 3e-3)) <= 1e-3 * out["value"]
    for k in ("roofline", "cpu_baseline", "alt_dtype", "alt_shapes", "rot_err_vs_oracle", "no_autotune", "ms_per_step_median"):
        assert k not in out, k                                    # measured with --full only
    poses, R = np.load(tmp_path / "a" / "poses.npy"), np.load(tmp_path / "a" / "R.npy")
    assert poses.dtype == np.float32 and poses.shape == (256, 16) and R.dtype == np.float32 and R.shape == (256, 9)
    Rm = torch.from_numpy(R).view(256, 3, 3)
    assert (Rm @ Rm.transpose(1, 2) - torch.eye(3)).abs().max() < 1e-4 and (torch.linalg.det(Rm) - 1).abs().max() < 1e-4
    # the records are the yaw-nulled [R|0] of the dumped rotations (bench.py: xyz = 0, nullify on)
    ref = E.compose_pose(torch.from_numpy(R).cuda(), torch.zeros(256, 3, device="cuda"), True).cpu()
    assert torch.equal(torch.from_numpy(poses).view(256, 4, 4), ref)
    # seeded inputs: a second run dumps the same arrays
    _plain_run(tmp_path / "b")
    assert np.array_equal(poses, np.load(tmp_path / "b" / "poses.npy")) and np.array_equal(R, np.load(tmp_path / "b" / "R.npy"))
