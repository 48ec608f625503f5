"""The multi-frame tracker on the device against the host tracker: nothing is gated on a ratio, the figures are
what they are.
  (a) one update at 4 / 16 / 31 measurements against 31 and 1024 open tracks: device events around flope_track_update (two
      launches) against the wall time of the host FlowerModel.add_poses(..., ignore=True) in the same process;
  (b) FlowerModel.add_stream frames/s with tracker="host" against tracker="device" on synthetic 1080p frames (the built-in
      detector, imgsz 1280), alternating windows in one process.
                                             python tools/bench_track.py [--out profiles/track_ab.json] [--frames 60] [--windows 3]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flope_amd")]
from flope_amd.track import DeviceTracker  # noqa: E402
from flope_amd.weights import synthetic_state_dict  # noqa: E402
from scipy.spatial.transform import Rotation as Rot  # noqa: E402
from sunflower.predictor.flower_model import FlowerModel  # noqa: E402

CAM = np.array([0.05, -0.02, 0.01, 0, 0, 0, 1.0])


def poses_at(points, rng, jitter=0.0):
    out = np.tile(np.eye(4), (len(points), 1, 1))
    out[:, :3, :3] = Rot.from_rotvec(rng.normal(0, 0.3, (len(points), 3))).as_matrix()
    out[:, :3, 3] = points + rng.uniform(-jitter, jitter, (len(points), 3))
    return out


def one_update(n, tracks, reps=200, warm=20):
    """n measurements (every one matches) against `tracks` open tracks -> (device us per update, host us per add_poses)"""
    rng = np.random.default_rng(n * 10007 + tracks)
    i = np.arange(tracks)
    grid = np.stack([0.25 * (i % 16), 0.25 * ((i // 16) % 16), 0.25 * (i // 256)], axis=1)
    opening = poses_at(grid, rng)
    frames = [poses_at(grid[rng.choice(tracks, n, replace=False)], rng, 0.01) for _ in range(warm + reps)]
    fm = FlowerModel(dist_th=50)
    fm.add_poses(opening, CAM, ignore=True)
    for f in frames[:warm]:
        fm.add_poses(f, CAM, ignore=True)
    t0 = time.perf_counter()
    for f in frames[warm:]:
        fm.add_poses(f, CAM, ignore=True)
    host_us = (time.perf_counter() - t0) / reps * 1e6
    t = DeviceTracker("cuda", max_tracks=tracks + 8, max_meas=max(tracks, n))
    t.update(opening, CAM)
    dev_frames = [torch.from_numpy(f.astype(np.float32)).cuda() for f in frames]          # float32 rows on the device, as the frame handle holds them
    for f in dev_frames[:warm]:
        t.update(f, CAM)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for f, (a, b) in zip(dev_frames[warm:], ev):
        a.record()
        t.update(f, CAM)
        b.record()
    torch.cuda.synchronize()
    dev = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    t0 = time.perf_counter()                                                                # what the host thread pays per enqueue
    for f in dev_frames[warm:]:
        t.update(f, CAM)
    enq_us = (time.perf_counter() - t0) / reps * 1e6
    torch.cuda.synchronize()
    assert t.count == tracks == len(fm.kfs)
    t.close()
    return dict(measurements=n, tracks=tracks, device_us_median=float(np.median(dev)), device_us_min=float(dev.min()), enqueue_us=enq_us,
                host_add_poses_us=host_us)


def streams(n_frames, windows):
    from flope_amd.yolo_weights import synthetic_frame, synthetic_yolo_state_dict
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    tmp = tempfile.mkdtemp()
    ckpt, intr, yolo_f = os.path.join(tmp, "posenet.pth"), os.path.join(tmp, "intrinsics.yaml"), os.path.join(tmp, "yolo11n_seg.pth")
    torch.save(synthetic_state_dict(0), ckpt)
    open(intr, "w").write(yaml.safe_dump(dict(fx=1400.0, fy=1400.0, cx=960.0, cy=540.0, h=1080, w=1920)))
    torch.save({**synthetic_yolo_state_dict(0), "imgsz": torch.tensor(1280)}, yolo_f)
    pred = FastPosePredictor("cuda", yolo_f, ckpt, intr)
    rgb = synthetic_frame(0)
    depth = (400 + np.random.default_rng(0).normal(0, 4, rgb.shape[:2])).astype(np.uint16)
    frames = [(rgb, depth, CAM)] * n_frames
    models = {k: FlowerModel(dist_th=50, pose_predictor=pred, tracker=k) for k in ("host", "device")}
    out = {k: [] for k in models}
    flowers = 0
    for k, m in models.items():                                                            # warm-up: graphs, slots, the first tracks
        flowers = max(len(pc) for pc, _ in m.add_stream(frames[:12]) if pc is not None)
    for _ in range(windows):
        for k, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(1 for _ in m.add_stream(frames))
            if k == "device":
                m.device_tracker.count                                                     # the window ends when the tracker has settled
            out[k].append(n / (time.perf_counter() - t0))
    assert list(models["device"].scores) == list(models["host"].scores)
    return dict(frames_per_window=n_frames, flowers_per_frame=flowers, host_fps=out["host"], device_fps=out["device"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_ab.json"))
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), update=[one_update(n, T) for T in (31, 1024) for n in (4, 16, 31)])
    for r in res["update"]:
        print(f"[track] {r['measurements']:2d} measurements, {r['tracks']:4d} tracks: device {r['device_us_median']:.1f} us per update (min {r['device_us_min']:.1f}), "
              f"enqueue {r['enqueue_us']:.1f} us on the host thread; host add_poses {r['host_add_poses_us']:.1f} us", flush=True)
    res["add_stream"] = streams(a.frames, a.windows)
    s = res["add_stream"]
    print(f"[track] add_stream, {s['flowers_per_frame']} flowers per 1080p frame, windows of {s['frames_per_window']} frames: host tracker "
          f"{' / '.join(f'{v:.1f}' for v in s['host_fps'])} frames/s, device tracker {' / '.join(f'{v:.1f}' for v in s['device_fps'])} frames/s", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
