"""GPU parity of the YOLO11-seg detector front end (C-ABI flope_yolo_*) against oracle/yolo_ref.py.
Tolerances: 16-bit maps (f16) against the fp32 oracle: rel-L2 <= 1e-2 per graph output (rounding accumulates over ~25
fused layers); float32 head rows <= 1e-2 rel; NMS indices bit-exact given the same head rows; boxes <= 1e-3 px given the
same rows; merged mask: identical except sign flips of ~0 values (< 0.02 % of pixels); uint8 resize: bit-exact."""
import numpy as np
import pytest
import torch

from oracle import pipeline_ref as P
from oracle import yolo_ref as Y

pytestmark = pytest.mark.gpu

LAYERS = ["0", "1", "2", "3", "4", "5", "6", "7", "8", "9", "10", "13", "16", "17", "19", "20", "22"]


@pytest.fixture(scope="module")
def ysd():
    from flope_amd.yolo_weights import synthetic_yolo_state_dict
    return synthetic_yolo_state_dict(0)


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _engine(ysd, H, W, imgsz, dtype="f16"):
    from flope_amd.yolo import YoloSeg
    y = YoloSeg(H, W, imgsz, dtype)
    y.load_state_dict(ysd)
    return y


@pytest.mark.parametrize("H,W,imgsz,dtype,tol,tol_emu", [(1080, 1920, 1280, "f16", 5e-3, None), (360, 640, 640, "f16", 5e-3, 3e-3), (300, 500, 320, "f16", 5e-3, None),
                                                         (250, 333, 640, "bf16", 8e-2, 1.5e-2)])     # measured (r04): 2.2e-3 / 2.0e-3, 1.4e-3 / 1.6e-3 / 1.2e-2; bf16 vs float32 4.3e-2
def test_every_graph_output_vs_oracle(ysd, H, W, imgsz, dtype, tol, tol_emu):
    """Every graph output and head row block against the float32 oracle (tol), and -- r04 -- against the oracle run WITH the device
    path's rounding points (Y.forward_layers(..., emulate=dtype): folded weights and stored maps in the 16-bit type, float32
    accumulation; tol_emu).  bf16 keeps BOTH bounds: the tight one against its emulation, and the loose float32 band as the
    independent check -- its 8 mantissa bits over 23 layers put the float32 forward 4e-2 away from ANY bf16 evaluation of this graph (the
    emulation itself sits there), so 8e-2 catches a shared design error (a wrong fold, a dropped rounding point) and nothing finer."""
    from flope_amd.yolo_weights import synthetic_frame
    img = synthetic_frame(3, H, W)
    y = _engine(ysd, H, W, imgsz, dtype)
    y.forward(img)
    x = Y.preprocess(img, imgsz)
    assert tuple(x.shape[2:]) == y.input_hw
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    got_in = y.read_tensor("input").cpu()
    assert torch.equal(got_in[:3], x[0].to(tdt).float()) and not got_in[3:].any()      # letterbox + BGR->RGB + /255: exact
    refs = []
    if tol is not None:
        refs.append(("float32 oracle", Y.forward_layers(ysd, x), tol))
    if tol_emu is not None:
        refs.append((f"{dtype}-emulating oracle", Y.forward_layers(ysd, x, emulate=tdt), tol_emu))
    for tag, o, t in refs:
        worst = [0.0, 0.0]
        for name in LAYERS:
            got = y.read_tensor(name).cpu()
            ref = o[int(name)][0]
            assert got.shape == ref.shape, name
            worst[0] = max(worst[0], _rel(got, ref))
            assert _rel(got, ref) <= t, (tag, name, _rel(got, ref))
        for name in ["proto_up", "proto"] + [f"{k}{i}" for i in range(3) for k in ("box", "cls", "coef")]:
            got, ref = y.read_tensor(name).cpu(), o[name][0]
            assert got.shape == ref.shape, name
            worst[1] = max(worst[1], _rel(got, ref))
            assert _rel(got, ref) <= 2 * t, (tag, name, _rel(got, ref))
        print(f"detector {dtype} {H}x{W}/{imgsz} vs {tag}: worst rel-L2 of a graph output {worst[0]:.2e}, of a head row block {worst[1]:.2e}")
    y.close()


def test_attention_kernels_agree(ysd):
    """C2PSA attention: the MFMA kernel (V^T in LDS, softmax in the accumulator layout) against the generic fp32 kernel
    on the same qkv map -- the graph output of layer 10 and everything downstream."""
    from flope_amd.yolo_weights import synthetic_frame
    img = synthetic_frame(8, 1080, 1920)
    y = _engine(ysd, 1080, 1920, 1280)
    y.forward(img)
    a10, a22 = y.read_tensor("10").cpu(), y.read_tensor("22").cpu()
    assert y.set_option("generic_attn", 1) == 0
    y.forward(img)
    b10, b22 = y.read_tensor("10").cpu(), y.read_tensor("22").cpu()
    assert _rel(a10, b10) <= 3e-3 and _rel(a22, b22) <= 5e-3, (_rel(a10, b10), _rel(a22, b22))
    y.close()


def test_level_batching_and_graph_replay_do_not_change_a_bit(ysd):
    """Default schedule: the independent ops of one dependency level (Segment-head branches, Proto, the parallel 1x1 convs
    of C3k ...) share one grid (ymulti_kernel).  One launch per op in program order, and a captured hipGraph replay of
    either, give the identical result: every graph output, the head rows, boxes and the mask."""
    from flope_amd.yolo_weights import synthetic_frame
    img = synthetic_frame(9, 1080, 1920)
    y = _engine(ysd, 1080, 1920, 1280)
    outs, launches = [], []
    for batch, graph in ((1, 1), (0, 0), (1, 0), (0, 1), (1, 1)):        # captured hipGraph replay and eager launches
        y.set_option("batch", batch)
        y.set_option("graph", graph)
        boxes, sc, cls, anchor, mask = y.detect(img, 0.1)
        boxes, sc, cls, anchor, mask = y.detect(img, 0.1)                 # second call: replay of the captured graph
        outs.append([boxes, sc, anchor, mask] + [y.read_tensor(k).cpu().numpy() for k in
                                                 ("proto", "cls2", "box0", "coef1", "4", "10", "13", "16", "19", "22")])
        launches.append(y.launches())
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)
    assert len(outs[0][2]) >= 10
    assert launches[0] == launches[2] and launches[1] == launches[3] and launches[0] < launches[1] - 20, launches
    y.close()


def test_lds_tile_and_pool_paths_equal_their_reference_paths(ysd):
    """Large maps stage an 8 x 16 output tile's input patch in LDS (default); option tile=0 reads the same fragments
    straight from global memory.  Same MFMA sequence per output pixel: every graph output and the head rows identical.
    Both options belong to one handle: a second detector of the process keeps the defaults."""
    from flope_amd.yolo_weights import synthetic_frame
    for (H, W, imgsz) in ((1080, 1920, 1280), (360, 640, 640), (250, 333, 320)):
        img = synthetic_frame(11, H, W)
        y = _engine(ysd, H, W, imgsz)
        outs = []
        for tile in (1, 0):
            y.set_option("tile", tile)
            y.forward(img)
            outs.append([y.read_tensor(k).cpu().numpy() for k in ("0", "1", "2", "3", "4", "13", "16", "19", "22", "proto", "box0", "cls0", "coef0", "box2")])
        other = _engine(ysd, H, W, imgsz)                   # built while the first handle has tile = 0
        assert other.set_option("tile", 1) == 1
        other.close()
        assert y.set_option("tile", 1) == 0
        for a, b in zip(outs[0], outs[1]):
            assert np.array_equal(a, b)
        # SPPF's three cascaded 5x5 max-pools: the LDS kernel (row / column passes) against the 13 x 13 ring sweep
        assert y.set_option("pool_lds", 0) == 1
        y.forward(img)
        ring = y.read_tensor("9").cpu().numpy()
        assert y.set_option("pool_lds", 1) == 0
        y.forward(img)
        assert np.array_equal(ring, y.read_tensor("9").cpu().numpy())
        y.close()


def test_fused_bottleneck_equals_two_conv_launches(ysd):
    """Bottleneck pairs (3x3 -> 3x3, <= 64 channels) run as ONE launch with the intermediate map in LDS (default); option
    bneck=0 launches the two convs.  On the large maps (no split-K in the unfused path) the MFMA sequence per output is the
    same: bit-identical.  On the small maps the unfused path splits K over four waves and adds the partial sums in another
    order: equal to fp32 summation order (one 16-bit rounding of a few outputs may flip)."""
    from flope_amd.yolo_weights import synthetic_frame
    for (H, W, imgsz) in ((1080, 1920, 1280), (360, 640, 640), (250, 333, 320)):
        img = synthetic_frame(12, H, W)
        y = _engine(ysd, H, W, imgsz)
        names = ("2", "4", "6", "8", "13", "16", "19", "22", "proto", "box0", "cls1", "coef2")
        outs = []
        for bneck in (1, 0):
            assert y.set_option("bneck", bneck) in (0, 1)
            y.forward(img)
            outs.append({k: y.read_tensor(k).cpu() for k in names})
        y.set_option("bneck", 1)
        for k in names:
            a, b = outs[0][k], outs[1][k]
            assert _rel(a, b) <= 2e-3, (k, _rel(a, b))
        if imgsz == 1280:
            assert torch.equal(outs[0]["2"], outs[1]["2"])            # 184 x 320 map: the unfused path does not split K either
        assert y.launches() < 75
        y.close()


def _head_rows(y):
    """the device's own float32 head rows as the oracle's `o` dict"""
    o = {}
    for i in range(3):
        for k in ("box", "cls", "coef"):
            o[f"{k}{i}"] = y.read_tensor(f"{k}{i}").cpu()[None]
    return o


@pytest.mark.parametrize("H,W,imgsz,conf,iou,max_det", [(1080, 1920, 1280, 0.25, 0.7, 300), (1080, 1920, 1280, 0.05, 0.45, 300),
                                                        (1080, 1920, 1280, 0.02, 0.7, 17), (360, 640, 640, 0.03, 0.7, 300),
                                                        (360, 640, 640, 0.9999, 0.7, 300)])
def test_decode_nms_boxes_bit_exact_given_the_head_rows(ysd, H, W, imgsz, conf, iou, max_det):
    """Detect._inference + ops.non_max_suppression + ops.scale_boxes on the device against the numpy restatement.
    Decode (DFL expectation, dist2bbox, sigmoid) from the SAME float32 head rows: to float32 round-off.  NMS from the
    device's own decoded candidates: kept anchors and their order IDENTICAL (integer / index work: bit-exact) -- two
    confidences one ulp apart may legitimately sort either way, so the index test must not depend on whose exp() it was."""
    from flope_amd.yolo_weights import synthetic_frame
    img = synthetic_frame(4, H, W)
    y = _engine(ysd, H, W, imgsz)
    boxes, sc, cls, anchor, mask = y.detect(img, conf, iou, max_det)
    _check_decode_and_nms(y, img, 1, conf, iou, max_det, boxes, sc, cls, anchor)
    if conf < 0.9:
        assert len(anchor) >= (8 if max_det > 17 else 17)
    else:
        assert len(anchor) == 0 and not mask.any()
    y.close()


def _check_decode_and_nms(y, img, nc, conf, iou, max_det, boxes, sc, cls, anchor):
    pred = Y.decode(_head_rows(y)).numpy()
    rbox, rconf, rcls = Y.candidates(pred, nc)
    cbox = y.read_tensor("cand_box").cpu().numpy()[:, 0].T
    cconf = y.read_tensor("cand_conf").cpu().numpy()[0, 0]
    ccls = y.read_tensor("cand_cls").cpu().numpy()[0, 0].astype(np.int64)
    np.testing.assert_allclose(cconf, rconf, rtol=3e-6)
    np.testing.assert_allclose(cbox, rbox, atol=2e-3)
    sure = np.abs(pred[:, 4:4 + nc].max(1) - np.sort(pred[:, 4:4 + nc], 1)[:, -2 if nc > 1 else -1]) > 1e-5 if nc > 1 else np.ones(len(rcls), bool)
    assert (ccls == rcls)[sure].all()
    keep = Y.nms_candidates(cbox, cconf, ccls, conf, iou, max_det, max_nms=4096)     # the device's candidate capacity
    assert anchor.tolist() == keep.tolist(), (len(anchor), len(keep))
    if len(keep):
        assert np.array_equal(sc, cconf[keep]) and np.array_equal(cls, ccls[keep]) and (np.diff(sc) <= 0).all()
        np.testing.assert_allclose(boxes, Y.scale_boxes(y.input_hw, cbox[keep], img.shape), atol=1e-4)
    # and against the all-oracle pipeline: the same detections unless two candidates are within round-off of each other
    if int((cconf > conf).sum()) <= 4096:
        det, idx = Y.non_max_suppression(pred, nc, conf, iou, max_det)
        assert len(set(idx.tolist()) ^ set(keep.tolist())) <= max(2, len(keep) // 20)


def test_masks_vs_oracle_given_the_head_rows(ysd):
    """ops.process_mask + get_bbox_mask's sum / clip / x255 / cv2.resize on the device, fed to the oracle from the
    device's own proto map, coefficients and boxes."""
    from flope_amd.yolo_weights import synthetic_frame
    H, W, imgsz = 1080, 1920, 1280
    img = synthetic_frame(5, H, W)
    y = _engine(ysd, H, W, imgsz)
    boxes, sc, cls, anchor, mask = y.detect(img)
    o = _head_rows(y)
    pred = Y.decode(o).numpy()
    det, idx = Y.non_max_suppression(pred, 1)
    assert anchor.tolist() == idx.tolist() and len(idx) >= 5
    proto = y.read_tensor("proto").cpu()
    ref_masks = Y.process_mask(proto, det[:, 6:], det[:, :4], y.input_hw).numpy()
    ref_lb = (np.clip(ref_masks.sum(0), 0, 1) * 255).astype(np.uint8)
    got_lb = y.read_tensor("mask_lb").cpu().numpy()[0].astype(np.uint8)
    assert got_lb.shape == ref_lb.shape and set(np.unique(got_lb)) <= {0, 255}
    assert (got_lb != ref_lb).mean() < 2e-4, float((got_lb != ref_lb).mean())
    assert 0.02 < (got_lb > 0).mean() < 0.98
    assert np.array_equal(mask, P.resize_linear_u8(got_lb, (W, H)))          # cv2.resize((W,H)) of the device's own merged mask
    y.close()


def test_detector_end_to_end_vs_fp32_oracle(ysd):
    """frame -> get_bbox_mask on the device (16-bit network) against the full fp32 CPU oracle."""
    from flope_amd.yolo_weights import synthetic_frame
    H, W = 1080, 1920
    img = synthetic_frame(6, H, W)
    y = _engine(ysd, H, W, 1280)
    bb, mask = y.get_bbox_mask(img)
    rb, rmask = Y.get_bbox_mask(ysd, img, 1280)
    assert bb.dtype == np.int16 and mask.dtype == np.uint8 and mask.shape == (H, W)
    rboxes, rconf, _ = Y.detect(ysd, img, 1280)
    boxes, conf, _, _, _ = y.detect(img)

    def iou(a, b):
        iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0])); ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
        u = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - iw * ih
        return iw * ih / u if u > 0 else 0.0
    # every confident detection of either side has a partner (a candidate within 0.01 of the threshold may flip)
    for A, ca, B in ((rboxes, rconf, boxes), (boxes, conf, rboxes)):
        for b_, c_ in zip(A, ca):
            if c_ > 0.27:
                assert max(iou(b_, o_) for o_ in B) > 0.9, (b_, c_)
    inter = np.logical_and(mask > 127, rmask > 127).sum(); union = np.logical_or(mask > 127, rmask > 127).sum()
    assert union > 0 and inter / union > 0.97, inter / union
    y.close()


@pytest.mark.parametrize("yolo_dtype", [None, "f16"])
def test_fast_pose_predictor_with_the_builtin_detector(ysd, state_dict, tmp_path, yolo_dtype):
    """BASELINE configs[2] end to end: FastPosePredictor(device, yolo_path=<state_dict file>, posenet_path, intrin_path)
    on a 1080p frame -- detector, crops, PoseResNet, Procrustes, depth lift, all on the device.
    Default detector (r05): the exact-float32 one -- the `int16` boxes and the `uint8` mask that
    fast_pose_predictor.py:49-56 hands to the pose path EQUAL the float32 oracle's.  `yolo_dtype="f16"` is the opt-in fast detector:
    the same number of boxes except for candidates within 0.01 of the confidence threshold (listed in the failure message), every
    other box within 2 px of its partner, mask XOR < 2 % -- the count is asserted, the comparison can no longer be skipped."""
    import yaml
    from flope_amd.yolo_weights import synthetic_frame
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    H, W = 1080, 1920
    img = synthetic_frame(7, H, W)
    rng = np.random.default_rng(7)
    depth = (400 + rng.normal(0, 4, (H, W))).astype(np.uint16)
    yolo_f, ckpt, intr = tmp_path / "yolo11n_seg.pth", tmp_path / "posenet.pth", tmp_path / "intrinsics.yaml"
    torch.save({**ysd, "imgsz": torch.tensor(1280)}, yolo_f)
    torch.save(state_dict, ckpt)
    intr.write_text(yaml.safe_dump(dict(fx=1400.0, fy=1400.0, cx=W / 2, cy=H / 2, h=H, w=W)))
    from oracle import posenet_ref as O
    pred = FastPosePredictor("cuda", str(yolo_f), str(ckpt), str(intr), **({} if yolo_dtype is None else {"yolo_dtype": yolo_dtype}))
    assert pred.yolo.dtype == (yolo_dtype or "f32")
    bb, mask = pred.get_bbox_mask(img)
    assert bb.dtype == np.int16 and bb.shape[0] >= 5 and mask.shape == (H, W)
    Rt = pred.get_flower_poses(img, depth)
    K = np.array([[1400.0, 0, W / 2], [0, 1400.0, H / 2], [0, 0, 1]])
    ref = P.get_flower_poses(lambda b: O.forward(state_dict, b), O.procrustes_to_rotmat, img, depth, bb, mask, K)
    assert Rt is not None and Rt.shape == ref.shape and Rt.shape[0] >= 3
    assert np.abs(Rt[:, :3, :3] - ref[:, :3, :3]).max() <= 1e-3
    assert np.linalg.norm(Rt[:, :3, 3] - ref[:, :3, 3], axis=1).max() <= 1e-5
    # the detector half against the float32 oracle
    rb, rmask = Y.get_bbox_mask(ysd, img, 1280)
    if yolo_dtype is None:
        assert np.array_equal(bb, rb) and np.array_equal(mask, rmask)
        return
    _, rconf, _ = Y.detect(ysd, img, 1280)
    _, conf, _, _, _ = pred.yolo.detect(img)
    thr = 0.25
    marg_r = [i for i, c in enumerate(rconf) if c < thr + 0.01]          # kept candidates that a 16-bit evaluation may drop ...
    marg_d = [i for i, c in enumerate(conf) if c < thr + 0.01]           # ... or that only the 16-bit evaluation keeps
    assert len(rconf) == rb.shape[0] and len(conf) == bb.shape[0]
    assert abs(bb.shape[0] - rb.shape[0]) <= len(marg_r) + len(marg_d), (bb.shape, rb.shape, [float(rconf[i]) for i in marg_r], [float(conf[i]) for i in marg_d])
    for i, r in enumerate(rb.astype(int)):                                # every non-marginal box of either side has a partner within 2 px
        if i not in marg_r:
            assert np.abs(bb.astype(int) - r).max(axis=1).min() <= 2, (i, r, float(rconf[i]))
    for i, d in enumerate(bb.astype(int)):
        if i not in marg_d:
            assert np.abs(rb.astype(int) - d).max(axis=1).min() <= 2, (i, d, float(conf[i]))
    assert (np.logical_xor(mask > 127, rmask > 127)).mean() < 0.02


@pytest.mark.parametrize("widths,nc,seed,H,W,imgsz", [((16, 32, 64, 128, 256), 3, 1, 360, 640, 640), ((32, 64, 128, 256, 512), 1, 0, 300, 500, 320),
                                                       ((32, 64, 128, 256, 512), 2, 0, 1080, 1920, 640)])
def test_other_checkpoints_scale_s_and_several_classes(widths, nc, seed, H, W, imgsz):
    """The graph is built from the checkpoint: the `s` scale (twice the widths, four attention heads in C2PSA) and
    multi-class heads (class-aware NMS through the cls * 7680 box offset) need no code path of their own."""
    from flope_amd.yolo_weights import synthetic_frame, synthetic_yolo_state_dict
    sd = synthetic_yolo_state_dict(seed, nc=nc, widths=widths, cls_bias=-3.0)
    img = synthetic_frame(11, H, W)
    y = _engine(sd, H, W, imgsz)
    boxes, sc, cls, anchor, mask = y.detect(img, 0.05, 0.6)
    o = Y.forward_layers(sd, Y.preprocess(img, imgsz))
    for name in ("10", "16", "22"):
        assert _rel(y.read_tensor(name).cpu(), o[int(name)][0]) <= 1.5e-2, name
    assert _rel(y.read_tensor("proto").cpu(), o["proto"][0]) <= 3e-2
    _check_decode_and_nms(y, img, nc, 0.05, 0.6, 300, boxes, sc, cls, anchor)
    assert len(anchor) >= 3
    if nc > 1:
        assert len(set(cls.tolist())) >= 2
    y.close()


def test_pipelined_live_loop_equals_the_sequential_one(ysd, state_dict, tmp_path):
    """FastPosePredictor.iter_flower_poses (several frames in flight: uploads, one or two detector instances replaying
    captured hipGraphs, and the pose network on their own streams, per-slot frame / mask / box buffers) returns, frame by
    frame, exactly what get_flower_poses returns -- for streams shorter than, equal to and longer than the pipeline depth."""
    import yaml
    from flope_amd.harness import live_pose_loop
    from flope_amd.yolo_weights import synthetic_frame
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    H, W = 540, 960
    yolo_f, ckpt, intr = tmp_path / "yolo.pth", tmp_path / "posenet.pth", tmp_path / "intrinsics.yaml"
    torch.save({**ysd, "imgsz": torch.tensor(640)}, yolo_f)
    torch.save(state_dict, ckpt)
    intr.write_text(yaml.safe_dump(dict(fx=700.0, fy=700.0, cx=W / 2, cy=H / 2, h=H, w=W)))
    pred = FastPosePredictor("cuda", str(yolo_f), str(ckpt), str(intr))
    rng = np.random.default_rng(3)
    frames = []
    for i in range(8):
        img = synthetic_frame(20 + i, H, W)
        depth = (400 + rng.normal(0, 4, (H, W))).astype(np.uint16)
        if i == 2:
            img = np.zeros_like(img)                  # a frame with nothing to detect in the middle of the stream
        frames.append((img, depth))
    seq = live_pose_loop(pred, frames)
    assert any(r is not None for r in seq) and seq[2] is None
    for n, nd in ((8, 2), (8, 1), (1, 2), (2, 2), (3, 2), (4, 2), (0, 2), (3, 1)):
        pip = list(pred.iter_flower_poses(frames[:n], detectors=nd))
        assert len(pip) == n
        for a, b in zip(seq, pip):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(a, b)
    assert len(live_pose_loop(pred, frames[:5], pipelined=True)) == 5


def test_detector_on_a_cu_masked_stream(ysd):
    """flope_stream_create_cu_mask: a stream restricted to 64 of the 256 CUs runs the same launches (the multi-op grids and
    the persistent-free kernels do not depend on the CU count): identical detections; bad masks are rejected."""
    import ctypes as C
    from flope_amd import _lib
    from flope_amd.yolo_weights import synthetic_frame
    lib = _lib.load()
    img = synthetic_frame(13, 360, 640)
    y = _engine(ysd, 360, 640, 640)
    ref = y.detect(img, 0.05)
    mask = (C.c_uint32 * 8)(*([0xFFFFFFFF, 0xFFFFFFFF] + [0] * 6))
    h = C.c_void_p()
    assert lib.flope_stream_create_cu_mask(0, mask, 8, C.byref(h)) == 0 and h.value
    st = torch.cuda.ExternalStream(h.value)
    with torch.cuda.stream(st):
        got = y.detect(img, 0.05)
    st.synchronize()
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    assert len(ref[0]) >= 3
    assert lib.flope_stream_destroy(0, h) == 0
    zero = (C.c_uint32 * 8)()
    assert lib.flope_stream_create_cu_mask(0, zero, 8, C.byref(h)) != 0
    assert lib.flope_stream_create_cu_mask(0, None, 8, C.byref(h)) != 0
    y.close()


def test_yolo_error_paths(ysd):
    from flope_amd.yolo import YoloSeg
    with pytest.raises(RuntimeError, match="imgsz"):
        YoloSeg(480, 640, 333)
    y = YoloSeg(480, 640, 640)
    with pytest.raises(RuntimeError, match="before flope_yolo_load_weights"):
        y.forward(np.zeros((480, 640, 3), np.uint8))
    bad = {k: v for k, v in ysd.items() if not k.startswith("model.8.")}
    with pytest.raises(RuntimeError, match="missing"):
        y.load_state_dict(bad)
    y.close()
    y = YoloSeg(480, 640, 640)
    y.load_state_dict(ysd)
    with pytest.raises(ValueError, match="uint8 BGR frame"):
        y.forward(np.zeros((481, 640, 3), np.uint8))
    with pytest.raises(RuntimeError, match="max_det"):
        y.detect(np.zeros((480, 640, 3), np.uint8), max_det=301)
    with pytest.raises(RuntimeError, match="already loaded"):
        y.load_state_dict(ysd)
    for retired in ("chain", "xcd", "wlds", "splitk_max_m"):      # removed conv variants and launch knobs
        with pytest.raises(RuntimeError, match="unknown option " + retired):
            y.set_option(retired, 0)
    y.close()


# ---- strict float32 mode (FLOPE_DT_F32, yolo_f32.hip): the integer outputs of get_bbox_mask against the all-float32 oracle --------
def _oracle_detect(ysd, img, imgsz, conf=0.25, iou=0.7):
    """the oracle's whole detector with its intermediate values: -> dict(o, pred, det, idx, boxes float32 frame xyxy,
    bbox int16, mask_lb uint8 letterboxed, mask uint8 frame, mfloat = interpolated instance masks before `> 0`)"""
    H, W = img.shape[:2]
    x = Y.preprocess(img, imgsz)
    o = Y.forward_layers(ysd, x)
    nc = o["cls0"].shape[1]
    pred = Y.decode(o).numpy()
    det, idx = Y.non_max_suppression(pred, nc, conf, iou)
    shape = tuple(x.shape[2:])
    mfloat = Y.process_mask(o["proto"][0], det[:, 6:], det[:, :4], shape, return_float=True).numpy()
    masks = (mfloat > 0).astype(np.float32)
    boxes = Y.scale_boxes(shape, det[:, :4], img.shape)
    return dict(o=o, pred=pred, det=det, idx=idx, boxes=boxes, bbox=boxes.astype(np.int16), mfloat=mfloat,
                mask_lb=(np.clip(masks.sum(0), 0, 1) * 255).astype(np.uint8), mask=P.merge_masks(masks, (W, H)), shape=shape)


def _assert_integer_outputs_equal(y, img, ref, tag, conf=0.25):
    """bbox int16 and mask uint8 of the strict float32 device mode against the oracle's: EQUAL, except -- listed and
    bounded -- where the oracle's own float32 value sits within float32 round-off of the decision boundary (a box
    coordinate within 2e-3 px of an integer, an interpolated mask value within 1e-5 of zero)."""
    H, W = img.shape[:2]
    boxes, conf, cls, anchor, mask = y.detect(img, conf)
    assert anchor.tolist() == ref["idx"].tolist(), (tag, anchor.tolist(), ref["idx"].tolist())
    bb = boxes.astype(np.int16)                                  # fast_pose_predictor.py:55-56
    np.testing.assert_allclose(boxes, ref["boxes"], atol=5e-3)
    np.testing.assert_allclose(conf, ref["det"][:, 4], rtol=2e-5)
    flips = np.argwhere(bb != ref["bbox"])
    for i, c in flips:                                           # allowed only on a truncation boundary of the ORACLE's value
        v = float(ref["boxes"][i, c])
        assert abs(v - round(v)) < 2e-3 and abs(int(bb[i, c]) - int(ref["bbox"][i, c])) == 1, (tag, i, c, v, bb[i, c])
    assert len(flips) <= 1, (tag, flips.tolist())
    got_lb = y.read_tensor("mask_lb").cpu().numpy()[0].astype(np.uint8)
    diff_lb = np.argwhere(got_lb != ref["mask_lb"])
    for yy, xx in diff_lb:                                       # allowed only where an instance's interpolated value is ~0
        assert np.abs(ref["mfloat"][:, yy, xx]).min() < 1e-5, (tag, yy, xx, ref["mfloat"][:, yy, xx])
    assert len(diff_lb) <= 4, (tag, len(diff_lb))
    if len(diff_lb) == 0:
        assert np.array_equal(mask, ref["mask"]), tag            # uint8 frame mask: bit-exact
    else:                                                        # a flipped letterbox pixel reaches at most its bilinear footprint
        sy, sx = H / got_lb.shape[0], W / got_lb.shape[1]
        bad = np.argwhere(mask != ref["mask"])
        for yy, xx in bad:
            assert min(abs(yy - (a + 0.5) * sy) + abs(xx - (b + 0.5) * sx) for a, b in diff_lb) <= 2 * (sy + sx) + 2, (tag, yy, xx)
    return bb, mask, len(flips), len(diff_lb)


@pytest.mark.parametrize("H,W,imgsz,seed,conf", [(1080, 1920, 1280, 6, 0.25), (360, 640, 640, 4, 0.05), (300, 500, 320, 3, 0.03)])
def test_f32_strict_mode_integer_outputs_equal_the_fp32_oracle(ysd, H, W, imgsz, seed, conf):
    """VERDICT r2 item 1 / north_star bar (1): the reference runs ultralytics in float32 and hands INTEGER boxes and a uint8
    mask to the pose path (fast_pose_predictor.py:49-56).  In FLOPE_DT_F32 mode (float32 maps, plain float32 FMA convolutions,
    same graph) every graph output is within float32 round-off of the oracle, NMS keeps the same anchors in the same order,
    and `bbox.astype(int16)` / the uint8 mask are EQUAL to the oracle's."""
    from flope_amd.yolo_weights import synthetic_frame
    img = synthetic_frame(seed, H, W)
    y = _engine(ysd, H, W, imgsz, "f32")
    y.forward(img)
    x = Y.preprocess(img, imgsz)
    got_in = y.read_tensor("input").cpu()
    assert torch.equal(got_in[:3], x[0]) and not got_in[3:].any()          # letterbox + BGR->RGB + /255 in float32: exact
    ref = _oracle_detect(ysd, img, imgsz, conf)
    o = ref["o"]
    worst = 0.0
    for name in LAYERS:
        got = y.read_tensor(name).cpu()
        assert got.shape == o[int(name)][0].shape, name
        worst = max(worst, _rel(got, o[int(name)][0]))
        assert _rel(got, o[int(name)][0]) <= 2e-5, (name, _rel(got, o[int(name)][0]))
    for name in ["proto_up", "proto"] + [f"{k}{i}" for i in range(3) for k in ("box", "cls", "coef")]:
        assert _rel(y.read_tensor(name).cpu(), o[name][0]) <= 2e-5, (name, _rel(y.read_tensor(name).cpu(), o[name][0]))
    bb, mask, nflip, npix = _assert_integer_outputs_equal(y, img, ref, f"{H}x{W}", conf)
    assert bb.shape[0] >= 3 and bb.dtype == np.int16 and mask.dtype == np.uint8
    print(f"f32 strict {H}x{W}: worst graph rel-L2 {worst:.2e}, {bb.shape[0]} boxes, {nflip} boundary coordinates, {npix} threshold pixels")
    # the 16-bit modes cannot be told apart from this one by their schedule options: batch / bneck are ignored here
    y.set_option("batch", 1)
    b2 = y.detect(img, conf)[0].astype(np.int16)
    assert np.array_equal(b2, bb)
    # r04: everything above ran on the exact-fp32 MFMA convolutions (v_mfma_f32_16x16x4_f32, default).  The plain fused-multiply-add
    # kernels (f32mfma = 0) are their checker: another summation order, so float32 round-off apart, the same integers
    heads = {n: y.read_tensor(n).cpu() for n in ("22", "proto", "box0", "cls2", "coef1")}
    assert y.set_option("f32mfma", 0) == 1
    bx, cf, _, an, mk = y.detect(img, conf)
    assert np.array_equal(bx.astype(np.int16), bb) and an.tolist() == ref["idx"].tolist()
    assert np.count_nonzero(mk != mask) <= 8 * npix
    for n, t in heads.items():
        assert _rel(y.read_tensor(n).cpu(), t) <= 1e-5, n
    assert y.set_option("f32mfma", 1) == 0
    import ctypes as C
    from flope_amd import _lib
    h = C.c_void_p()
    assert _lib.load().flope_yolo_create(0, H, W, imgsz, 7, C.byref(h)) != 0 and b"dtype" in _lib.load().flope_yolo_last_error(None)
    y.close()


def test_f32_frame_to_poses_equals_the_all_oracle_pipeline(ysd, state_dict, tmp_path):
    """frame -> [N,4,4] through FastPosePredictor with the strict float32 detector, against a pipeline in which EVERYTHING is
    the oracle (oracle boxes, oracle mask, oracle crops / PoseResNet / Procrustes / depth lift): the same flowers in the same
    order, R within 1e-3, xyz within 1e-5 m.  (The 16-bit detector test above feeds the pose oracle the device's own boxes.)"""
    import yaml
    from flope_amd.yolo_weights import synthetic_frame
    from oracle import posenet_ref as O
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    H, W = 1080, 1920
    img = synthetic_frame(7, H, W)
    rng = np.random.default_rng(7)
    depth = (400 + rng.normal(0, 4, (H, W))).astype(np.uint16)
    yolo_f, ckpt, intr = tmp_path / "yolo11n_seg.pth", tmp_path / "posenet.pth", tmp_path / "intrinsics.yaml"
    torch.save({**ysd, "imgsz": torch.tensor(1280)}, yolo_f)
    torch.save(state_dict, ckpt)
    intr.write_text(yaml.safe_dump(dict(fx=1400.0, fy=1400.0, cx=W / 2, cy=H / 2, h=H, w=W)))
    pred = FastPosePredictor("cuda", str(yolo_f), str(ckpt), str(intr), yolo_dtype="f32")
    rb, rmask = Y.get_bbox_mask(ysd, img, 1280)
    bb, mask = pred.get_bbox_mask(img)
    assert np.array_equal(bb, rb) and np.array_equal(mask, rmask)           # integer outputs: equal (seed chosen off any boundary)
    Rt = pred.get_flower_poses(img, depth)
    K = np.array([[1400.0, 0, W / 2], [0, 1400.0, H / 2], [0, 0, 1]])
    ref = P.get_flower_poses(lambda b: O.forward(state_dict, b), O.procrustes_to_rotmat, img, depth, rb, rmask, K)
    assert Rt is not None and Rt.shape == ref.shape and Rt.shape[0] >= 3
    assert np.abs(Rt[:, :3, :3] - ref[:, :3, :3]).max() <= 1e-3
    assert np.linalg.norm(Rt[:, :3, 3] - ref[:, :3, 3], axis=1).max() <= 1e-5
    assert np.array_equal(Rt[:, 3], np.tile([0, 0, 0, 1.0], (Rt.shape[0], 1)))


def test_graph_cache_holds_one_entry_per_output_set(ysd):
    """"graph" option: repeated detects with the same (frame, thresholds, outputs) tuple replay ONE captured sequence -- the
    cache key is compared bytewise, so it must not depend on struct padding -- and more output sets than cache
    slots evict the oldest entry only after its last replay has finished."""
    from flope_amd.yolo_weights import synthetic_frame
    img = synthetic_frame(13, 360, 640)
    y = _engine(ysd, 360, 640, 640)
    y.set_option("graph", 1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ref = y.detect(img, 0.05)
        for _ in range(5):
            got = y.detect(img, 0.05)
            assert y.graph_cache_size() == 1
        outs = [y.new_outputs() for _ in range(11)]
        frame = torch.from_numpy(img).cuda()
        for k in range(3):
            for o in outs:
                y.detect_device(frame, 0.05, out=o, in_place=True)
            assert y.graph_cache_size() == 8
        st.synchronize()
        for o in outs:
            n = int(o[1].item())
            assert n == len(ref[0]) and np.array_equal(o[0][:n, :4].cpu().numpy(), ref[0]) and np.array_equal(o[2].cpu().numpy(), ref[4])
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
    y.close()
