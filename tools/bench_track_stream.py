"""One frame's encoder step over live tracks, fed on the device against fed through the host: nothing is gated on a
ratio, the figures are what they are.  In one process, alternating frame by frame on the same tracker updates:
  device   st.step_tracker(tracker) on a device-positioned windowed state: device events around the call (tf_stream_feed_kernel, the
           step's launch sequence for all n rows, tf_feed_fill_bias), the host thread's time to enqueue it, and the wall time of
           update + step_tracker + synchronize;
  host     what the parent offers: tracker.last_association() (a host wait), the track list and the float32 rows in numpy from the
           frame's poses, st.step(x, tracks) on a host-positioned windowed state: device events around st.step alone, and the wall
           time of read-back + numpy + upload + step + synchronize behind the same update, which has finished by then.
Shapes: 4, 16 and 31 measurements (each on a track of its own, the same tracks every frame, so that every window is full when the
timing starts) against 31 and 1024 open tracks, window 64, cfg5's encoder in f32 and f16.
                                             python tools/bench_track_stream.py [--out profiles/track_stream_ab.json] [--reps 100]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flope_amd")]
from flope_amd.tf_encoder import TransformerEncoder  # noqa: E402
from flope_amd.track import DeviceTracker  # noqa: E402
from oracle.tf_encoder_ref import synthetic_state_dict  # noqa: E402
from scipy.spatial.transform import Rotation as Rot  # noqa: E402
from sunflower.predictor.flower_model import cam_pose_to_matrix, poses_to_measurements  # noqa: E402
from sunflower.utils.mvg import pose_cam_to_world  # noqa: E402

DIMS = (32, 384, 9, 6, 12, 1536)          # cfg5: in, d, out, heads, layers, ff
WINDOW = 64
CAM = np.array([0.05, -0.02, 0.01, 0, 0, 0, 1.0])


def poses_at(points, rng, jitter=0.0):
    out = np.tile(np.eye(4), (len(points), 1, 1))
    out[:, :3, :3] = Rot.from_rotvec(rng.normal(0, 0.3, (len(points), 3))).as_matrix()
    out[:, :3, 3] = points + rng.uniform(-jitter, jitter, (len(points), 3))
    return out


def one_shape(enc, n, tracks, reps, warm=WINDOW + 6):
    rng = np.random.default_rng(n * 10007 + tracks)
    i = np.arange(tracks)
    grid = np.stack([0.25 * (i % 16), 0.25 * ((i // 16) % 16), 0.25 * (i // 256)], axis=1)
    frames = [poses_at(grid[:n], rng, 0.01).astype(np.float32) for _ in range(warm + reps)]
    dev_frames = [torch.from_numpy(f).cuda() for f in frames]
    cam = cam_pose_to_matrix(CAM)
    trk = DeviceTracker("cuda", max_tracks=tracks + 8, max_meas=max(tracks, n))
    trk.update(poses_at(grid, rng), CAM)
    dev = enc.open_stream(tracks, WINDOW, window=WINDOW, positions="device", max_rows=n)
    host = enc.open_stream(tracks, WINDOW, window=WINDOW)
    y_dev, y_host = torch.empty(n, DIMS[2], device="cuda"), torch.empty(n, DIMS[2], device="cuda")
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    wall = {"device": [], "host": []}
    enq = []
    for k, (f, fd) in enumerate(zip(frames, dev_frames)):
        timed = k >= warm
        e = ev[k - warm] if timed else [None] * 4
        # device path
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trk.update(fd, CAM)
        if timed:
            e[0].record()
        t1 = time.perf_counter()
        dev.step_tracker(trk, out=y_dev)
        t2 = time.perf_counter()
        if timed:
            e[1].record()
        torch.cuda.synchronize()
        if timed:
            wall["device"].append(time.perf_counter() - t0)
            enq.append(t2 - t1)
        # host path, on the same update (finished by now): the association comes back, the rows are made in numpy, the step takes a host list of tracks
        t0 = time.perf_counter()
        assoc = trk.last_association()
        tr = [int(a) if a >= 0 else -1 - int(a) for a in assoc]
        x = np.zeros((n, DIMS[0]), dtype=np.float32)
        x[:, :7] = poses_to_measurements(pose_cam_to_world(f.astype(np.float64), cam)).astype(np.float32)
        xg = torch.from_numpy(x).cuda()
        if timed:
            e[2].record()
        host.step(xg, tr, out=y_host)
        if timed:
            e[3].record()
        torch.cuda.synchronize()
        if timed:
            wall["host"].append(time.perf_counter() - t0)
    assert dev.positions[:n] == host.positions[:n] == [warm + reps] * n and torch.isfinite(y_dev).all()
    # the two paths saw the same tracks and (up to scipy's quaternion) the same rows
    diff = float((y_dev - y_host).abs().max())
    d = np.array([a[0].elapsed_time(a[1]) * 1e3 for a in ev])
    h = np.array([a[2].elapsed_time(a[3]) * 1e3 for a in ev])
    for o in (dev, host, trk):
        o.close()
    return dict(measurements=n, tracks=tracks, device_step_us_median=float(np.median(d)), device_step_us_min=float(d.min()),
                device_enqueue_us=float(np.median(enq) * 1e6), host_step_us_median=float(np.median(h)), host_step_us_min=float(h.min()),
                device_frame_wall_us=float(np.median(wall["device"]) * 1e6), host_frame_wall_us=float(np.median(wall["host"]) * 1e6),
                host_frame_wall_excludes="the tracker update (it is the device path's, already waited for)", max_abs_diff=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_stream_ab.json"))
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict(DIMS[0], DIMS[1], DIMS[2], DIMS[4], DIMS[5], seed=5).items()}
    res = dict(device=torch.cuda.get_device_name(0), dims_in_d_out_heads_layers_ff=DIMS, window=WINDOW, reps=a.reps, shapes=[])
    for dtype in ("f32", "f16"):
        enc = TransformerEncoder(*DIMS, dtype=dtype, max_tokens=64)
        enc.load_state_dict(sd)
        for tracks in (31, 1024):
            for n in (4, 16, 31):
                r = dict(dtype=dtype, **one_shape(enc, n, tracks, a.reps))
                res["shapes"].append(r)
                print(f"[track_stream] {dtype} {n:2d} measurements, {tracks:4d} tracks: device step {r['device_step_us_median']:.1f} us (min {r['device_step_us_min']:.1f}, "
                      f"enqueue {r['device_enqueue_us']:.1f} us), frame wall {r['device_frame_wall_us']:.1f} us | host step {r['host_step_us_median']:.1f} us "
                      f"(min {r['host_step_us_min']:.1f}), frame wall behind the update {r['host_frame_wall_us']:.1f} us | max |dy| {r['max_abs_diff']:.2e}", flush=True)
        enc.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
