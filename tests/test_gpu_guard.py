"""The guarded mode on the device (flope_guard_*, GuardedPoseEngine, PoseResNet(compute_dtype="guard")): the
whole batch on the f16 trunk, the crops whose own head output M has gap(M) = s2 + sign(det M) s3 below gap_min run again on the
float32 MFMA trunk.

The fixture holds both kinds of crop (checked on the CPU with oracle/posenet_ref.py): weights synthetic_state_dict(0), group A =
seed 0 rand(8,3,224,224), group B = seed 1 rand(8,3,224,224) * 0.3, fc_rot.bias = 0.03 bias0 - mean over group B of (W h).  The
float32 oracle gives gaps 0.640 - 0.683 (A) and 0.0545 - 0.0590 (B); a gap moves by at most 3 sqrt(3) max|dM| = 5.2e-3 at the f16
tolerance max|dM| <= 1e-3, so with gap_min = 0.5 no crop's classification is in doubt.
Tolerances: the north-star gate |dR| <= 1e-3 against the float32 oracle; 8 u |M|_F (u = 2^-24) for the gap, a float32 of magnitude
<= sqrt(2) |M|_F computed in float64; everything else is bit equality.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from oracle import posenet_ref as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_parity as G  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
A_ROWS, B_ROWS = list(range(8)), list(range(8, 16))


def _guard(sd, H, W, B, max_repair=32, **kw):
    from flope_amd.engine import GuardedPoseEngine
    g = GuardedPoseEngine(H, W, B, max_repair, **kw)
    g.load_state_dict(sd)
    return g


def _poses(eng, x, xyz, guard=False):
    """crops -> (r9, R, Rt) on the host with xyz and the yaw-null on: flope_forward_poses of a PoseEngine, or the guarded pair"""
    from flope_amd.engine import input_format, _stream_ptr
    x = x.cuda().contiguous()
    B = x.shape[0]
    xyz_d = xyz.cuda().contiguous()
    r9, R, Rt = (torch.empty((B, n), dtype=torch.float32, device="cuda") for n in (9, 9, 16))
    fmt = input_format(x)
    if guard:
        eng.forward_poses_into(x, fmt, xyz_d, True, Rt, R, r9)
    else:
        rc = eng.lib.flope_forward_poses(eng.handle, x.data_ptr(), fmt, B, xyz_d.data_ptr(), 1, r9.data_ptr(), R.data_ptr(), Rt.data_ptr(),
                                         _stream_ptr(eng.device))
        assert rc == 0
    torch.cuda.synchronize()
    return r9.cpu(), R.cpu(), Rt.cpu()


def _gap64(r9):
    M = r9.double().view(-1, 3, 3)
    s = torch.linalg.svdvals(M)
    return s[:, 1] + torch.sign(torch.linalg.det(M)) * s[:, 2], M.flatten(1).norm(dim=1)


@pytest.fixture(scope="module")
def both_kinds(state_dict):
    torch.manual_seed(0)
    a = torch.rand(8, 3, 224, 224)
    torch.manual_seed(1)
    b = torch.rand(8, 3, 224, 224) * 0.3
    sd0 = dict(state_dict)
    sd0["fc_rot.bias"] = torch.zeros(9)
    sd = dict(state_dict)
    sd["fc_rot.bias"] = state_dict["fc_rot.bias"] * 0.03 - O.forward(sd0, b).mean(0)
    x = torch.cat([a, b])
    ref9 = O.forward(sd, x)
    gap, _ = _gap64(ref9)
    print(f"oracle gaps: A {float(gap[:8].min()):.4f} .. {float(gap[:8].max()):.4f}, B {float(gap[8:].min()):.4f} .. {float(gap[8:].max()):.4f}")
    assert gap[:8].min() > 0.63 and gap[8:].max() < 0.07         # the margins the module docstring states
    return sd, x, ref9, O.procrustes_to_rotmat(ref9)


# ---- 4. the guarantee ------------------------------------------------------------------------------------------------------------------
def test_guarded_rotations_hold_the_gate_where_f16_does_not(both_kinds):
    """Measured on an MI355X: guarded max|dR| 2.85e-4 on group A (the f16 rows) and 2.1e-6 on group B (repaired); the plain f16
    engine gives 1.30e-3 .. 2.88e-3 on group B (the f16-emulating oracle predicted 1.36e-3 .. 2.96e-3)."""
    sd, x, _, Rref = both_kinds
    g = _guard(sd, 224, 224, 16)
    r9, R = g.forward(x.cuda())
    torch.cuda.synchronize()
    dR = (R.cpu() - Rref).abs().amax(dim=(1, 2))
    plain = G._engine(sd, 224, 224, 16, "f16")
    _, Rf = G._run(plain, x)
    dRf = (Rf - Rref).abs().amax(dim=(1, 2))
    print(f"guard: max|dR| A {float(dR[:8].max()):.3e}  B {float(dR[8:].max()):.3e};  plain f16: A {float(dRf[:8].max()):.3e}  "
          f"B {float(dRf[8:].min()):.3e} .. {float(dRf[8:].max()):.3e};  repaired {g.last_repaired}, flagged {g.read_selection()}")
    assert dR.max() <= 1e-3
    assert g.read_selection() == B_ROWS and g.last_repaired == 8
    assert dRf[8:].max() > 1e-3, "the fixture does not discriminate: plain f16 holds the gate on group B"
    plain.close()
    g.close()


# ---- 5. nothing else moved -----------------------------------------------------------------------------------------------------------
def test_unflagged_rows_are_f16_bits_and_flagged_rows_are_f32m_bits(both_kinds):
    sd, x, _, _ = both_kinds
    xyz = torch.rand(16, 3, generator=torch.Generator().manual_seed(2))
    g = _guard(sd, 224, 224, 16)
    got = _poses(g, x, xyz, guard=True)
    assert g.last_repaired == 8 and g.read_selection() == B_ROWS
    plain = G._engine(sd, 224, 224, 16, "f16")
    fast = _poses(plain, x, xyz)
    exact_e = G._engine(sd, 224, 224, 8, "f32m")
    exact = _poses(exact_e, x[8:], xyz[8:])
    for name, a, f, e in zip(("r9", "R", "Rt"), got, fast, exact):
        assert torch.equal(a[:8], f[:8]), f"{name}: a row of group A differs from the plain f16 engine's"
        assert torch.equal(a[8:], e), f"{name}: a row of group B differs from the f32m engine's forward of those crops alone"
        assert not torch.equal(f[8:], e), name                      # (the comparison above could tell the two apart)
    for e_ in (g, plain, exact_e):
        e_.close()


# ---- 6. the device's figure and its list ---------------------------------------------------------------------------------------------------
def test_gap_and_index_list_on_the_device(both_kinds):
    sd, x, _, _ = both_kinds
    plain = G._engine(sd, 224, 224, 16, "f16")
    r9f, _ = G._run(plain, x)                                         # the M the selection saw (test 5: the guard's f16 forward is this one)
    plain.close()
    want, fro = _gap64(r9f)
    g = _guard(sd, 224, 224, 16)
    lists = {}
    for gap_min in (0.5, float(want[:8].sort().values[3:5].mean()), 0.0, 1e9):     # default; a threshold inside group A; nothing; everything
        g.gap_min = gap_min
        for streams in (2, 1):
            g.set_option("streams", streams)
            g.forward(x.cuda())
            torch.cuda.synchronize()
            gap = g.last_gap.cpu()
            ratio = (gap.double() - want).abs() / (8 * U * fro)
            assert ratio.max() <= 1.0, (gap_min, streams, ratio)
            sel = g.read_selection()
            assert sel == torch.nonzero(~(gap >= gap_min)).flatten().tolist() and sel == sorted(sel)
            assert g.last_repaired == len(sel)
            lists[(gap_min, streams)] = sel
        assert lists[(gap_min, 1)] == lists[(gap_min, 2)]
    print(f"gap_dev: worst |err| / (8 u |M|_F) = {float(ratio.max()):.4f}; lists {[(k, len(v)) for k, v in lists.items()]}")
    assert len(lists[(0.5, 2)]) == 8 and len(lists[(0.0, 2)]) == 0 and len(lists[(1e9, 2)]) == 16
    assert 8 < len([v for k, v in lists.items() if k[0] not in (0.5, 0.0, 1e9)][0]) < 16
    g.close()


# ---- 7. no flagged crop ----------------------------------------------------------------------------------------------------------------
def test_no_crop_flagged_is_the_plain_f16_forward(state_dict, golden_cfg1):
    torch.manual_seed(0)
    x = torch.rand(16, 3, 224, 224)
    xyz = torch.rand(16, 3, generator=torch.Generator().manual_seed(3))
    g = _guard(state_dict, 224, 224, 16)
    got = _poses(g, x, xyz, guard=True)
    assert g.last_repaired == 0 and g.read_selection() == []
    print(f"cfg1 gaps {float(g.last_gap.min()):.3f} .. {float(g.last_gap.max()):.3f}")
    plain = G._engine(state_dict, 224, 224, 16, "f16")
    fast = _poses(plain, x, xyz)
    for a, f in zip(got, fast):
        assert torch.equal(a, f)
    err = float((got[1].view(-1, 3, 3) - torch.from_numpy(golden_cfg1["R"])).abs().max())
    print(f"cfg1 guard: |R - golden|max = {err:.3e}")
    assert err <= 1e-3
    plain.close()
    g.close()


# ---- 8. every crop flagged, more than fit ------------------------------------------------------------------------------------------------
def _as_format(x, fmt):
    if fmt == "f32":
        return x
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    return {"bf16": nhwc.to(torch.bfloat16), "f16": nhwc.to(torch.float16), "u8": (nhwc * 255).to(torch.uint8)}[fmt]


@pytest.mark.parametrize("H,W", [(96, 80), (65, 71)])
def test_every_crop_flagged_in_five_chunks_and_four_input_formats(state_dict, H, W):
    B = 37
    torch.manual_seed(5)
    x = torch.rand(B, 3, H, W)
    xyz = torch.rand(B, 3, generator=torch.Generator().manual_seed(6))
    g = _guard(state_dict, H, W, B, max_repair=8, gap_min=1e9)
    assert g.max_repair == 8
    exact = G._engine(state_dict, H, W, B, "f32m")
    for fmt in ("f32", "bf16", "f16", "u8"):
        xf = _as_format(x, fmt)
        got = _poses(g, xf, xyz, guard=True)
        assert g.last_repaired == B and g.read_selection() == list(range(B))
        want = _poses(exact, xf, xyz)
        for name, a, e in zip(("r9", "R", "Rt"), got, want):
            assert torch.equal(a, e), (fmt, name)
    exact.close()
    g.close()


# ---- 9. slots and refusals -----------------------------------------------------------------------------------------------------------------
def test_two_slots_in_flight_and_call_order(both_kinds):
    from flope_amd import _lib
    from flope_amd.engine import PoseEngine, GuardedPoseEngine
    sd, x, _, _ = both_kinds
    xd = x.cuda()
    y = torch.cat([x[8:], x[:8]]).cuda()                            # the other frame: group B first
    g = _guard(sd, 224, 224, 16)

    def bufs():
        return [torch.empty((16, n), dtype=torch.float32, device="cuda") for n in (9, 9, 16, 1)]

    seq = []
    for t in (xd, y):
        b = bufs()
        g.guard_forward(0, t, 0, None, True, b[0], b[1], b[2], b[3].view(-1))
        assert g.guard_repair(0) == 8
        torch.cuda.synchronize()
        seq.append([v.cpu() for v in b])
    b0, b1 = bufs(), bufs()
    g.guard_forward(0, xd, 0, None, True, b0[0], b0[1], b0[2], b0[3].view(-1))
    g.guard_forward(1, y, 0, None, True, b1[0], b1[1], b1[2], b1[3].view(-1))
    assert g.guard_repair(0) == 8 and g.guard_repair(1) == 8
    torch.cuda.synchronize()
    assert g.read_selection(0) == B_ROWS and g.read_selection(1) == A_ROWS
    for got, want in ((b0, seq[0]), (b1, seq[1])):
        for a, w in zip(got, want):
            assert torch.equal(a.cpu(), w)
    # call order
    with pytest.raises(RuntimeError, match="error -3.*call flope_guard_forward for this slot first"):
        g.guard_repair(1)
    g.guard_forward(1, y, 0, None, True, b1[0], b1[1], b1[2], None)
    with pytest.raises(RuntimeError, match="error -3.*awaits flope_guard_repair"):
        g.guard_forward(1, y, 0, None, True, b1[0], b1[1], b1[2], None)
    assert g.guard_repair(1) == 8                                     # the refusal left the armed forward intact
    with pytest.raises(RuntimeError, match="error -1.*bad slot"):
        g.guard_repair(g.slots)
    # a forward the engine refuses leaves the slot idle, and the slot works again
    rc = g.lib.flope_guard_forward(g.guard_handle, 0, xd.data_ptr(), 0, 17, None, 1, b0[0].data_ptr(), b0[1].data_ptr(), b0[2].data_ptr(), None, None)
    assert rc == -1 and b"batch must be within 1..max_batch" in g.lib.flope_guard_last_error(g.guard_handle)
    rc = g.lib.flope_guard_forward(g.guard_handle, 0, xd.data_ptr(), 0, 16, None, 1, None, None, None, None, None)
    assert rc == -1 and b"no output buffer" in g.lib.flope_guard_last_error(g.guard_handle)
    with pytest.raises(RuntimeError, match="error -3"):
        g.guard_repair(0)
    g.guard_forward(0, xd, 0, None, True, b0[0], b0[1], b0[2], b0[3].view(-1))
    assert g.guard_repair(0) == 8
    torch.cuda.synchronize()
    for a, w in zip(b0, seq[0]):
        assert torch.equal(a.cpu(), w)
    g.close()
    # what flope_guard_create refuses, each with its message
    lib = _lib.load()
    f16, bf16 = PoseEngine(96, 80, 8, "f16"), PoseEngine(96, 80, 8, "bf16")
    f32, f32_other, f32_narrow = PoseEngine(96, 80, 4, "f32m"), PoseEngine(65, 71, 4, "f32m"), PoseEngine(96, 80, 4, "f32m", backbone_out_dim=1024)

    def refused(fast, exact, max_repair, slots, text):
        h = C.c_void_p()
        rc = lib.flope_guard_create(fast.handle if fast else None, exact.handle if exact else None, max_repair, slots, C.byref(h))
        msg = lib.flope_guard_last_error(None).decode()
        assert rc == -1 and not h.value and text in msg, (rc, msg)

    refused(bf16, f32, 4, 1, "bf16 fast engine is refused")
    refused(f32, f32_other, 4, 1, "fast engine must be FLOPE_DT_F16")
    refused(f16, bf16, 4, 1, "exact engine must be FLOPE_DT_F32")
    refused(f16, f32_other, 4, 1, "share device, crop size and backbone_out_dim")
    refused(f16, f32_narrow, 4, 1, "share device, crop size and backbone_out_dim")
    refused(f16, f32, 5, 1, "max_repair must be within 1..max_batch of the exact engine (4)")
    refused(f16, f32, 0, 1, "max_repair must be within")
    refused(f16, f32, 4, 0, "1..16 slots")
    refused(f16, f32, 4, 17, "1..16 slots")
    refused(None, f32, 4, 1, "two distinct PoseResNet engine handles")
    h = C.c_void_p()
    assert lib.flope_guard_create(f16.handle, f32.handle, 4, 2, C.byref(h)) == 0 and h.value
    assert lib.flope_guard_set_gap_min(h, 0.25) == 0.5 and lib.flope_guard_set_gap_min(h, 0.5) == 0.25
    # (neither engine has weights: the engine's own refusal passes through and the slot stays idle)
    t = torch.zeros(1, 3, 96, 80, device="cuda")
    o = torch.empty(16, device="cuda")
    assert lib.flope_guard_forward(h, 0, t.data_ptr(), 0, 1, None, 0, None, o.data_ptr(), None, None, None) == -3
    assert b"flope_load_weights" in lib.flope_guard_last_error(h)
    assert lib.flope_guard_repair(h, 0, None) == -3
    assert lib.flope_guard_destroy(h) == 0
    for e in (f16, bf16, f32, f32_other, f32_narrow):
        e.close()
    assert isinstance(GuardedPoseEngine.SLOTS, int)


# ---- 10. the predictors ------------------------------------------------------------------------------------------------------------------
def _frame_crops_and_reliable(rgb, mask, depth, boxes, K, crop=512):
    """What both predictors feed the network for this frame (float32 crops of the in-frame boxes) and which of those rows survive
    the depth-reliability filter."""
    from flope_amd import _lib, engine as E
    from sunflower.predictor.fast_pose_predictor import select_boxes, upload_depth
    dev = torch.device("cuda")
    _, sq, good = select_boxes(boxes, rgb.shape)
    frame_d, mask_d = torch.from_numpy(np.ascontiguousarray(rgb)).to(dev), torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
    _, reliable, _ = E.depth_lift(upload_depth(depth, dev), mask_d, torch.from_numpy(good.astype(np.int32)).to(dev),
                                  (K[0][0], K[1][1], K[0][2], K[1][2]), 1000.0, 0.1, 2.5)
    crops = E.crop_resize_mask(frame_d, mask_d, torch.from_numpy(sq.astype(np.int32)).to(dev), crop, _lib.IN_F32_NCHW)
    return crops, reliable.cpu().numpy().astype(bool)


def _rebiased(state_dict, crops):
    """fc_rot.bias = 0.03 bias0 - the mean r9 a first run with a zero bias returns for these crops: small gaps on this frame"""
    sd0 = dict(state_dict)
    sd0["fc_rot.bias"] = torch.zeros(9)
    e = G._engine(sd0, crops.shape[2], crops.shape[3], crops.shape[0], "f16")
    r9, _ = e.forward(crops)
    torch.cuda.synchronize()
    e.close()
    sd = dict(state_dict)
    sd["fc_rot.bias"] = state_dict["fc_rot.bias"] * 0.03 - r9.cpu().mean(0)
    return sd


def _split_threshold(gaps):
    """midpoint of the widest space between two sorted gaps: both kinds of row occur by construction"""
    s = np.sort(np.asarray(gaps, dtype=np.float64))
    assert len(s) >= 2 and np.isfinite(s).all()
    k = int(np.argmax(np.diff(s)))
    return float((s[k] + s[k + 1]) / 2)


def _three_predictors(monkeypatch, make):
    preds = {}
    for mode in ("guard", "f16", "f32m"):
        monkeypatch.setenv("FLOPE_DTYPE", mode)
        preds[mode] = make()
        assert preds[mode].posenet.compute_dtype == mode
    return preds


def _judge_rows(got, fast, exact, flagged, what):
    assert got.shape == fast.shape == exact.shape and got.shape[0] == len(flagged) and got.shape[0] >= 3
    assert flagged.any() and not flagged.all(), (what, flagged)
    for i, fl in enumerate(flagged):
        want, other = (exact, fast) if fl else (fast, exact)
        assert np.array_equal(got[i], want[i]), f"{what}: row {i} ({'flagged' if fl else 'not flagged'}) differs from the {'f32m' if fl else 'f16'} predictor's"
    print(f"{what}: {int(flagged.sum())} of {len(flagged)} rows repaired; max |f16 - f32m| over rows {np.abs(fast - exact).max():.3e}")


def test_predictor_with_given_detections_in_guard_mode(state_dict, tmp_path, monkeypatch):
    import yaml
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    rgb, mask, depth, boxes = G._scene(22)
    K = np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]])
    crops, reliable = _frame_crops_and_reliable(rgb, mask, depth, boxes, K)
    sd = _rebiased(state_dict, crops)
    ckpt, intr = tmp_path / "posenet.pth", tmp_path / "intrinsics.yaml"
    torch.save(sd, ckpt)
    intr.write_text(yaml.safe_dump(dict(fx=600.0, fy=600.0, cx=320.0, cy=240.0, h=480, w=640)))
    preds = _three_predictors(monkeypatch, lambda: FastPosePredictor("cuda", lambda img: (boxes, mask), str(ckpt), str(intr)))
    guard = preds["guard"]
    assert guard.get_flower_poses(rgb, depth) is not None
    eng = guard.posenet.engine_for("cuda", (512, 512))
    gaps = eng.last_gap.cpu().numpy()
    assert len(gaps) == len(reliable) == crops.shape[0]
    eng.gap_min = _split_threshold(gaps[reliable])
    got = guard.get_flower_poses(rgb, depth)
    flagged = ~(eng.last_gap.cpu().numpy() >= eng.gap_min)
    assert eng.last_repaired == int(flagged.sum()) and eng.read_selection() == np.nonzero(flagged)[0].tolist()
    print(f"gaps {np.round(gaps, 4).tolist()}  gap_min {eng.gap_min:.4f}")
    _judge_rows(got, preds["f16"].get_flower_poses(rgb, depth), preds["f32m"].get_flower_poses(rgb, depth), flagged[reliable], "detections given")


def test_predictor_with_the_builtin_detector_in_guard_mode(state_dict, tmp_path, monkeypatch):
    import yaml
    from flope_amd.yolo_weights import synthetic_frame, synthetic_yolo_state_dict
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    H, W = 1080, 1920
    img = synthetic_frame(7, H, W)
    depth = (400 + np.random.default_rng(7).normal(0, 4, (H, W))).astype(np.uint16)
    K = np.array([[1400.0, 0, W / 2], [0, 1400.0, H / 2], [0, 0, 1]])
    yolo_f, ckpt0, ckpt, intr = tmp_path / "yolo11n_seg.pth", tmp_path / "posenet0.pth", tmp_path / "posenet.pth", tmp_path / "intrinsics.yaml"
    torch.save({**synthetic_yolo_state_dict(0), "imgsz": torch.tensor(1280)}, yolo_f)
    torch.save(state_dict, ckpt0)
    intr.write_text(yaml.safe_dump(dict(fx=1400.0, fy=1400.0, cx=W / 2, cy=H / 2, h=H, w=W)))
    monkeypatch.setenv("FLOPE_DTYPE", "f16")
    first = FastPosePredictor("cuda", str(yolo_f), str(ckpt0), str(intr))
    bb, mask = first.get_bbox_mask(img)
    assert bb.shape[0] >= 5
    crops, reliable = _frame_crops_and_reliable(img, mask, depth, bb, K)
    del first
    torch.save(_rebiased(state_dict, crops), ckpt)
    del crops
    torch.cuda.empty_cache()
    preds = _three_predictors(monkeypatch, lambda: FastPosePredictor("cuda", str(yolo_f), str(ckpt), str(intr)))
    guard = preds["guard"]
    assert guard.get_flower_poses(img, depth) is not None
    ctx = guard._frame_ctx()
    eng = guard.posenet.engine_for("cuda", (512, 512))
    assert ctx.engine is eng and eng.guard_handle
    gaps = ctx.read_gaps(0)
    assert len(gaps) == len(reliable)
    eng.gap_min = _split_threshold(gaps[reliable])
    got = guard.get_flower_poses(img, depth)
    gaps2 = ctx.read_gaps(0)
    assert np.array_equal(gaps, gaps2)
    flagged = ~(gaps2 >= np.float32(eng.gap_min))
    assert eng.read_selection(0) == np.nonzero(flagged)[0].tolist()
    print(f"gaps {np.round(gaps, 4).tolist()}  gap_min {eng.gap_min:.4f}")
    fast, exact = preds["f16"].get_flower_poses(img, depth), preds["f32m"].get_flower_poses(img, depth)
    _judge_rows(got, fast, exact, flagged[reliable], "built-in detector")
    # the pipelined loop gives the same rows; a consumer that stops early leaves no slot armed
    frames = [(img, depth)] * 6
    gen = guard.iter_flower_poses(frames)
    for k, poses in enumerate(gen):
        assert np.array_equal(poses, got), k
        if k == 1:
            break
    gen.close()
    assert np.array_equal(guard.get_flower_poses(img, depth), got)
    assert all(np.array_equal(p, got) for p in guard.iter_flower_poses(frames))
    assert np.array_equal(guard.get_flower_poses(img, depth), got)


def test_guarded_frame_handle_with_more_boxes_than_the_engine_holds(state_dict):
    """flope_frame_* over a guard whose f16 engine holds 3 crops, on a frame with 7 in-frame boxes: three forwards per frame, all but
    the last repaired inside flope_frame_enqueue.  Everything flagged = the rows of a frame handle over an f32m engine, nothing
    flagged = the rows of one over an f16 engine, bit for bit; then the same through two slots in flight."""
    from flope_amd.engine import PoseEngine
    from flope_amd.frame import FramePoses
    from sunflower.predictor.fast_pose_predictor import upload_depth
    rgb, mask, depth, boxes = G._scene(22)
    K = np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]])
    dev = torch.device("cuda")
    det = torch.zeros((16, 8), dtype=torch.float32)
    det[:len(boxes), :4] = torch.from_numpy(boxes.astype(np.float32))
    det, count = det.to(dev), torch.tensor([len(boxes)], dtype=torch.int32, device=dev)
    frame_d, mask_d, depth_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(mask).to(dev), upload_depth(depth, dev)
    want = {}
    for mode in ("f16", "f32m"):
        e = PoseEngine(96, 96, 8, mode)
        e.load_state_dict(state_dict)
        ctx = FramePoses(e, 480, 640, 16, 1)
        want[mode] = ctx.to_poses(det, count, frame_d, mask_d, depth_d, K)
        ctx.close()
        e.close()
    assert want["f16"].shape[0] == 6 and not np.array_equal(want["f16"], want["f32m"])
    g = _guard(state_dict, 96, 96, 3, max_repair=2)
    ctx = FramePoses(g, 480, 640, 16, 2)
    for gap_min, mode, n_flagged in ((1e9, "f32m", 7), (-1.0, "f16", 0)):
        g.gap_min = gap_min
        assert np.array_equal(ctx.to_poses(det, count, frame_d, mask_d, depth_d, K), want[mode]), mode
        assert len(ctx.read_gaps(0)) == 7 and g.read_selection(0) == list(range(1 if n_flagged else 0))   # (the last forward held one crop)
        ctx.select(0, det, count)
        ctx.select(1, det, count)
        assert ctx.enqueue(0, frame_d, mask_d, depth_d, K) == 7 and ctx.enqueue(1, frame_d, mask_d, depth_d, K) == 7
        assert np.array_equal(ctx.finish(0), want[mode]) and np.array_equal(ctx.finish(1), want[mode])
    with pytest.raises(RuntimeError, match="more slots than the guard has"):
        FramePoses(_GuardView(g), 480, 640, 16, 17)
    ctx.close()
    g.close()


class _GuardView:
    """just enough of a GuardedPoseEngine for FramePoses to ask flope_frame_create_guarded for more slots than the guard has"""

    def __init__(self, g):
        self.guard_handle, self.device, self.handle = g.guard_handle, g.device, g.handle
