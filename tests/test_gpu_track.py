"""The tracker on the device (flope_track_*, flope_frame_track; flope_amd/csrc/track.hip, flope_amd/track.py).  Cases,
oracle and checker: tests/track_cases.py (what the cases promise and which defects they notice: tests/test_track_host.py, CPU);
bound: tests/track_bound.py.

  1. every case through flope_track_update: association, track count and hit counts equal to oracle/fusion_ref.py's integer for
     integer, means and p within the derived bound of the exact recursion, sentinel words untouched;
  2. float32 rows against the same rows widened on the host: equal bits;
  3. overflow, every argument refusal, two updates on two streams in call order;
  4. behind the frame handle: FramePoses.track on three frames in flight equals DeviceTracker.update on the rows finish returned, bit for
     bit; against the host FlowerModel the integers are equal and the means within SCIPY_MARGIN x SCIPY_F32_DIFF (the measured
     difference between scipy's quaternion and track_math.h's on float32 rotations; tests/test_track_host.py asserts the figure);
     a guarded handle and an idle slot are refused;
  5. iter_flower_poses(..., tracker=, cam_poses=) yields what it yields without a tracker, and FlowerModel(tracker="device").add_stream
     ends with the tracks and scores of tracker="host".
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as Rot

import frame_cases as FC
import track_cases as TC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_guard as TG  # noqa: E402

pytestmark = pytest.mark.gpu
TOL_HOST = TC.SCIPY_MARGIN * TC.SCIPY_F32_DIFF


def _tracker(max_tracks, max_meas, **kw):
    from flope_amd.track import DeviceTracker
    return DeviceTracker("cuda", max_tracks=max_tracks, max_meas=max_meas, dist_th=TC.TH_MM, q=TC.Q, r=TC.R, p0=TC.P0, **kw)


def _same_state(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.CASE_NAMES)
def test_case_on_the_device(name):
    case = TC.cases()[name]
    t = _tracker(case.max_tracks, case.max_meas)
    trace = TC.run_case(case, t)
    fails = TC.check_case(case, trace)
    ratio, err, ratio_p = TC.worst_ratio(case, trace) if not TC.check_integers(case, trace) else (np.nan, np.nan, np.nan)
    host = TC.run_case(case, TC.HostWalk(TC.load_harness(), case.max_tracks, case.max_meas))
    print(f"{name}: error / bound {ratio:.3f} (error {err:.3g}), p {ratio_p:.3f}; bits equal to the host walk: {_same_state(trace[1:], host[1:])}")
    assert not fails, fails[:6]
    assert t.sentinels_changed() == 0 and t.count == len(TC.expected(case).tracks)
    t.close()


def test_identity_camera_keeps_the_translation_bits_and_python_reads_like_the_host_model():
    case = TC.cases()["first_frame"]
    t = _tracker(8, 8)
    assert t.state is None and t.scores is None and t.count == 0 and t.filtered_state().shape == (0, 7)
    TC.run_case(case, t)
    assert t.state[:, :3].tobytes() == np.ascontiguousarray(case.frames[0].poses[:, :3, 3]).tobytes()
    assert t.scores.dtype == np.float64 and t.scores.tolist() == [1.0] * 5 and t.p.tolist() == [TC.P0] * 5
    assert t.last_association().tolist() == [-1, -2, -3, -4, -5]
    t.reset()
    assert t.count == 0 and t.state is None
    with pytest.raises(RuntimeError, match="no update since"):
        t.last_association()
    t.close()


# ---- 2. float32 rows ---------------------------------------------------------------------------------------------------------------------
def test_float32_rows_equal_the_same_rows_widened_on_the_host():
    f32, f64 = TC.f32_frames()
    case = TC.cases()["camera_pose"]
    a, b, c = _tracker(8, 8), _tracker(8, 8), _tracker(8, 8)
    ta, tb = TC.run_case(case, a, f32), TC.run_case(case, b, f64)
    for fr in f32:                                                 # and as a device tensor the caller already holds
        c.update(torch.from_numpy(fr.poses.copy()).cuda(), fr.cam)
    assert _same_state(ta[1:], tb[1:]) and _same_state(ta[1:], c.read()) and ta.hits.sum() == 11 and len(ta.hits) == 4
    for t in (a, b, c):
        t.close()


# ---- 3. overflow, refusals, streams ------------------------------------------------------------------------------------------------------
def test_overflow_applies_nothing_and_sticks_until_reset():
    from flope_amd import _lib
    three, two_more, one_more = TC.overflow_frames()
    t = _tracker(4, 4)
    t.update(*three)
    assert t.count == 3
    before = t.raw_state(4)
    assoc_before = t.last_association()
    t.update(*two_more)                                            # matches track 0 and needs two more: 5 > 4
    assert t.lib.flope_track_count(t.handle) == _lib.ESTATE and "max_tracks (4)" in t.lib.flope_track_last_error(t.handle).decode()
    buf = np.empty((4, 7))
    assert t.lib.flope_track_read(t.handle, buf.ctypes.data, None, None, None, 4) == _lib.ESTATE
    assert t.lib.flope_track_read_assoc(t.handle, np.empty(4, np.int32).ctypes.data, 4) == _lib.ESTATE
    after = t.raw_state(4)
    assert _same_state(before[:4], after[:4]) and after[4].tolist() == [3, 1] and t.sentinels_changed() == 0
    t.update(*one_more)                                            # would fit, but the flag is sticky
    assert _same_state(before[:4], t.raw_state(4)[:4]) and t.lib.flope_track_count(t.handle) == _lib.ESTATE
    with pytest.raises(RuntimeError, match="flope_track_reset"):
        t.count
    t.reset()
    assert t.count == 0
    t.update(*three)
    t.update(*one_more)
    assert t.last_association().tolist() == [-4, 1] and t.read()[3].tolist() == [1, 2, 1, 1] and t.sentinels_changed() == 0
    assert assoc_before.tolist() == [-1, -2, -3]
    t.close()


@pytest.mark.parametrize("args,word", [((0, 4, 0.05, 1e-3, 0.1, 1.0), "max_tracks"), ((4, 0, 0.05, 1e-3, 0.1, 1.0), "max_meas"),
                                       ((4, 4, 0.0, 1e-3, 0.1, 1.0), "dist_th_m"), ((4, 4, -0.05, 1e-3, 0.1, 1.0), "dist_th_m"),
                                       ((4, 4, float("nan"), 1e-3, 0.1, 1.0), "dist_th_m"), ((4, 4, float("inf"), 1e-3, 0.1, 1.0), "dist_th_m"),
                                       ((4, 4, 0.05, 0.0, 0.1, 1.0), "q must"), ((4, 4, 0.05, 1e-3, float("nan"), 1.0), "r must"),
                                       ((4, 4, 0.05, 1e-3, 0.1, -1.0), "p0"), ((4, 4, 0.05, 1e-3, 0.1, float("inf")), "p0")])
def test_create_refuses(args, word):
    from flope_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.flope_track_create(0, *args, C.byref(h)) == _lib.EINVAL and not h.value
    assert word in lib.flope_track_last_error(None).decode()
    assert lib.flope_track_create(0, 4, 4, 0.05, 1e-3, 0.1, 1.0, None) == _lib.EINVAL


def test_update_refuses_and_enqueues_nothing():
    from flope_amd import _lib
    three, _, one_more = TC.overflow_frames()
    t = _tracker(8, 2)
    t.update(*one_more)
    state = t.read()
    with pytest.raises(RuntimeError, match=r"n = 3 outside 0 \.\. max_meas \(2\)"):
        t.update(*three)
    poses = torch.from_numpy(one_more.poses.copy()).cuda()
    cam = np.eye(4).reshape(16)
    assert t.lib.flope_track_update(t.handle, poses.data_ptr(), 1, None, 3, cam.ctypes.data, None) == _lib.EINVAL
    assert t.lib.flope_track_update(t.handle, poses.data_ptr(), 1, None, -1, cam.ctypes.data, None) == _lib.EINVAL
    assert t.lib.flope_track_update(t.handle, poses.data_ptr(), 2, None, 2, cam.ctypes.data, None) == _lib.EINVAL
    assert t.lib.flope_track_update(t.handle, None, 1, None, 2, cam.ctypes.data, None) == _lib.EINVAL
    assert t.lib.flope_track_update(t.handle, poses.data_ptr(), 1, None, 2, None, None) == _lib.EINVAL
    assert t.lib.flope_track_update(None, poses.data_ptr(), 1, None, 2, cam.ctypes.data, None) == _lib.EINVAL
    assert t.lib.flope_track_update(t.handle, None, 1, None, 0, None, None) == 0          # n = 0 is a no-op, whatever else is passed
    assert _same_state(state, t.read()) and t.last_association().tolist() == [-1, -2]
    assert t.lib.flope_track_read(t.handle, np.empty((1, 7)).ctypes.data, None, None, None, 1) == _lib.EINVAL    # two tracks, room for one
    with pytest.raises(ValueError):
        t.update(torch.zeros(2, 4, 4, dtype=torch.float16, device="cuda"), TC.IDENTITY_CAM)
    t.close()


def test_two_updates_on_two_streams_apply_in_call_order():
    """the first update waits behind a long kernel on its stream; the second, on an idle stream, must still come second (the
    handle's event): applied the other way round, the second frame's measurements would open the tracks"""
    case = TC.cases()["gate_49_51"]
    t = _tracker(8, 8)
    f0, f1 = [torch.from_numpy(fr.poses.copy()).cuda() for fr in case.frames]
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.rand(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s0):
        for _ in range(20):
            big = big @ big * 1e-3                                 # some milliseconds of work in front of the first update
        t.update(f0, case.frames[0].cam)
    with torch.cuda.stream(s1):
        t.update(f1, case.frames[1].cam)
    assert t.last_association().tolist() == [0, -2]                # (waits for the handle's last update, on whatever stream)
    trace = TC.Trace(TC.expected(case).assoc, *t.read())
    assert not TC.check_case(case, trace)
    torch.cuda.synchronize()
    t.close()


# ---- 4. behind the frame handle ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(state_dict):
    from flope_amd.engine import PoseEngine
    eng = PoseEngine(FC.CROP, FC.CROP, FC.ENGINE_BATCH, "f16")
    eng.load_state_dict(state_dict)
    g = TG._guard(state_dict, FC.CROP, FC.CROP, FC.ENGINE_BATCH)
    yield {"plain": eng, "guard": g}
    g.close()
    eng.close()


def _inputs(name):
    from sunflower.predictor.fast_pose_predictor import upload_depth
    fr, dev = FC.frame(name), torch.device("cuda")
    return (torch.from_numpy(fr.det.copy()).to(dev), torch.tensor([fr.count], dtype=torch.int32, device=dev), torch.from_numpy(fr.rgb.copy()).to(dev),
            torch.from_numpy(fr.mask.copy()).to(dev), upload_depth(fr.depth.copy(), dev))


def _start(ctx, slot, inp):
    ctx.select(slot, inp[0], inp[1])
    return ctx.enqueue(slot, *inp[2:], FC.K, depth_div=FC.DEPTH_DIV, near=FC.NEAR, far=FC.FAR)


def _cam(t, rotvec):
    return np.concatenate([np.asarray(t, dtype=np.float64), Rot.from_rotvec(rotvec).as_quat()])


def test_frame_track_equals_update_on_the_finished_rows_and_the_host_model(engines):
    from flope_amd.frame import FramePoses
    from sunflower.predictor.flower_model import FlowerModel
    ctx = FramePoses(engines["plain"], FC.FH, FC.FW, FC.MAX_BOXES, 3)
    inp = {n: _inputs(n) for n in ("F0", "F1", "F3", "F5")}
    rv = [0.2, -0.1, 0.3]
    plan = [("F0", _cam([0.1, -0.2, 0.05], rv)), ("F1", _cam([0.6, -0.2, 0.05], rv)), ("F0", _cam([0.11, -0.2, 0.05], rv)),      # three in flight
            ("F3", _cam([0.1, -0.2, 0.05], rv)), ("F5", _cam([0.1, -0.2, 0.05], rv)), ("F1", _cam([0.6, -0.19, 0.05], [0.21, -0.1, 0.3]))]
    behind, rows = _tracker(64, FC.MAX_BOXES), []
    for first in (0, 3):
        ns = []
        for slot in range(3):
            name, cam = plan[first + slot]
            ns.append(_start(ctx, slot, inp[name]))
            ctx.track(slot, behind, cam)                           # no host wait: the poses are still being computed
        assert ns == ([5, 7, 5] if first == 0 else [2, 0, 7])
        rows += [ctx.finish(slot) for slot in range(3)]
    assert [None if r is None else len(r) for r in rows] == [4, 5, 4, None, None, 5]
    direct, fm = _tracker(64, FC.MAX_BOXES), FlowerModel(dist_th=TC.TH_MM)
    for r, (_, cam) in zip(rows, plan):
        direct.update(r, cam)
        fm.add_poses(r, cam, ignore=True)
    got, want = behind.read(), direct.read()
    assert _same_state(got, want) and behind.sentinels_changed() == 0
    anchors, means, p, hits = got
    assert len(fm.kfs) == len(hits) and hits.tolist() == [int(s) for s in fm.scores] and hits.max() >= 2
    d_anchor = np.abs(anchors - fm.state).max()
    d_mean = np.abs(means - fm.filtered_state()).max()
    d_p = max(abs(kf.P[0, 0] - pv) for kf, pv in zip(fm.kfs, p))
    print(f"device tracker vs host FlowerModel on {len(hits)} tracks: anchors {d_anchor:.3g}, means {d_mean:.3g} (tolerance {TOL_HOST:.3g}), p {d_p:.3g}")
    assert d_anchor <= TOL_HOST and d_mean <= TOL_HOST and d_p <= 1e-12
    for t in (behind, direct):
        t.close()
    ctx.close()


def test_frame_track_refusals(engines):
    from flope_amd import _lib
    from flope_amd.frame import FramePoses
    lib = _lib.load()
    cam = np.eye(4).reshape(16)
    t = _tracker(16, FC.MAX_BOXES)
    small = _tracker(16, 2)
    ctx = FramePoses(engines["plain"], FC.FH, FC.FW, FC.MAX_BOXES, 2)
    inp = _inputs("F0")
    assert lib.flope_frame_track(ctx.handle, 0, t.handle, cam.ctypes.data) == _lib.ESTATE             # idle
    ctx.select(0, inp[0], inp[1])
    assert lib.flope_frame_track(ctx.handle, 0, t.handle, cam.ctypes.data) == _lib.ESTATE             # selected, not enqueued
    assert _start(ctx, 0, inp) == 5
    assert lib.flope_frame_track(ctx.handle, 1, t.handle, cam.ctypes.data) == _lib.ESTATE             # the other slot is idle
    assert lib.flope_frame_track(ctx.handle, 2, t.handle, cam.ctypes.data) == _lib.EINVAL
    assert lib.flope_frame_track(ctx.handle, 0, None, cam.ctypes.data) == _lib.EINVAL
    assert lib.flope_frame_track(ctx.handle, 0, t.handle, None) == _lib.EINVAL
    assert lib.flope_frame_track(ctx.handle, 0, small.handle, cam.ctypes.data) == _lib.EINVAL          # 5 rows > max_meas = 2
    assert "max_meas (2)" in lib.flope_frame_last_error(ctx.handle).decode()
    assert t.count == 0 and small.count == 0                                                           # nothing was enqueued
    assert lib.flope_frame_track(ctx.handle, 0, t.handle, cam.ctypes.data) == 0
    assert len(ctx.finish(0)) == 4 and t.count == 4
    with pytest.raises(RuntimeError, match="nothing enqueued"):
        ctx.track(0, t, TC.IDENTITY_CAM)                                                               # finished: idle again
    ctx.close()
    guarded = FramePoses(engines["guard"], FC.FH, FC.FW, FC.MAX_BOXES, 1)
    assert _start(guarded, 0, inp) == 5
    assert lib.flope_frame_track(guarded.handle, 0, t.handle, cam.ctypes.data) == _lib.EINVAL
    assert "guarded" in lib.flope_frame_last_error(guarded.handle).decode()
    assert len(guarded.finish(0)) == 4 and t.count == 4
    guarded.close()
    t.close()
    small.close()


# ---- 5. the predictor's loop and FlowerModel ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream(state_dict, tmp_path_factory):
    """a FastPosePredictor on 540 x 960 frames and six frames with camera poses: a scene, the same scene twice more from a camera
    that has moved a few millimetres, nothing to detect, another scene, the first again"""
    import yaml
    from flope_amd.yolo_weights import synthetic_frame, synthetic_yolo_state_dict
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    d = tmp_path_factory.mktemp("track_stream")
    H, W = 540, 960
    yolo_f, ckpt, intr = d / "yolo.pth", d / "posenet.pth", d / "intrinsics.yaml"
    torch.save({**synthetic_yolo_state_dict(0), "imgsz": torch.tensor(640)}, yolo_f)
    torch.save(state_dict, ckpt)
    intr.write_text(yaml.safe_dump(dict(fx=700.0, fy=700.0, cx=W / 2, cy=H / 2, h=H, w=W)))
    pred = FastPosePredictor("cuda", str(yolo_f), str(ckpt), str(intr))
    rng = np.random.default_rng(5)
    flat = np.full((H, W), 400, np.uint16)
    scenes = [s for s in range(20, 28) if pred.get_flower_poses(synthetic_frame(s, H, W), flat) is not None][:2]     # two scenes with flowers in them
    assert len(scenes) == 2
    frames = []
    for i, seed in enumerate((scenes[0], scenes[0], scenes[0], None, scenes[1], scenes[0])):
        img = synthetic_frame(seed, H, W) if seed is not None else np.zeros((H, W, 3), np.uint8)
        depth = (400 + rng.normal(0, 1.5, (H, W))).astype(np.uint16)
        cam = np.concatenate([rng.normal(0, 0.002, 3), Rot.from_rotvec(rng.normal(0, 0.002, 3)).as_quat()])
        frames.append((img, depth, cam))
    return pred, frames


def test_iter_flower_poses_with_a_tracker_yields_the_same_and_feeds_it_in_frame_order(stream):
    pred, frames = stream
    plain = list(pred.iter_flower_poses(((f[0], f[1]) for f in frames), detectors=2))
    t = _tracker(256, 300)
    fed = list(pred.iter_flower_poses(((f[0], f[1]) for f in frames), detectors=2, tracker=t, cam_poses=[f[2] for f in frames]))
    assert len(plain) == len(fed) == 6 and plain[3] is None and plain[0] is not None
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(plain, fed))
    direct = _tracker(256, 300)
    for rows, f in zip(plain, frames):
        direct.update(rows, f[2])
    assert _same_state(t.read(), direct.read()) and t.read()[3].max() >= 2
    with pytest.raises(ValueError, match="go together"):
        next(pred.iter_flower_poses(((f[0], f[1]) for f in frames), tracker=t))
    for x in (t, direct):
        x.close()


def test_flower_model_add_stream_on_the_device_tracker_equals_the_host_tracker(stream):
    from sunflower.predictor.flower_model import FlowerModel
    pred, frames = stream
    host, dev = FlowerModel(dist_th=TC.TH_MM, pose_predictor=pred), FlowerModel(dist_th=TC.TH_MM, pose_predictor=pred, tracker="device")
    out_h, out_d = list(host.add_stream(frames, ignore=True)), list(dev.add_stream(frames, ignore=True))
    assert len(out_h) == len(out_d) == 6 and out_h[3] == (None, None) == out_d[3]
    for (ac, aw), (bc, bw) in zip(out_h, out_d):
        assert (ac is None and bc is None) or (np.array_equal(ac, bc) and np.array_equal(aw, bw))
    assert len(host.kfs) >= 3 and dev.get_state().shape == host.get_state().shape
    assert dev.scores.tolist() == host.scores.tolist() and dev.scores.max() >= 2
    d_anchor, d_mean = np.abs(dev.get_state() - host.get_state()).max(), np.abs(dev.filtered_state() - host.filtered_state()).max()
    print(f"add_stream, device vs host tracker on {len(host.kfs)} tracks: anchors {d_anchor:.3g}, means {d_mean:.3g} (tolerance {TOL_HOST:.3g})")
    assert d_anchor <= TOL_HOST and d_mean <= TOL_HOST
    with pytest.raises(AttributeError, match="tracker='host'"):
        dev.kfs
    # frame by frame through add_poses: the same tracker once more
    again = FlowerModel(dist_th=TC.TH_MM, pose_predictor=pred, tracker="device")
    for (pc, _), f in zip(out_h, frames):
        again.add_poses(pc, f[2], ignore=True)
    assert _same_state(again.device_tracker.read(), dev.device_tracker.read())
    for m in (dev, again):
        m.device_tracker.close()
