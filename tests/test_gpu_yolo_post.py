"""The detector's post-processing kernels (ydecode_kernel, ynms_kernel and its box scaling, ymask_low_kernel / its float32 twin,
ymask_merge_kernel, the uint8 resize) on the hand-built head rows of tests/yolo_post_cases.py, through YoloSeg.postprocess: the
launch sequence of detect() itself, fed rows instead of a network forward.  The checker is the one the CPU half
(tests/test_yolo_post_cases.py) shows to fail on every broken copy of the algorithm.

Exact cases tolerate nothing: decoded boxes, kept anchors and their order, confidences, classes, scaled boxes, every pixel of the
merged mask and of the resized mask equal the oracle's.  Generic rows: rtol 3e-6 on confidences, atol 2e-3 on boxes (the suite's
own), NMS / scaling / masks bit-exact from the device's own candidates.

Measured on MI355X (run with -s for the figures of every case): no case differed on the device, in f16, bf16 or f32 engines, and no
kernel had to change.  Exact cases: every decoded box bit-equal, worst relative confidence error 1.6e-7 (rtol 3e-6).  Generic rows
(A = 21 / A = 84): worst relative confidence error 0 / 9.4e-8, worst box error 1.5e-5 / 3.1e-5 px (atol 2e-3).  Every over-capacity
case counted more than 4096 candidates on the device.  The whole file runs in about 3 s, no case runs a network forward.
"""
import numpy as np
import pytest
import torch

import yolo_post_cases as YC

pytestmark = pytest.mark.gpu

CASES = YC.all_cases()
_ENGINES, _SD = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for y in _ENGINES.values():
        y.close()
    _ENGINES.clear()


def _engine(g, dtype="f16"):
    """one engine per (size, checkpoint, dtype) for the whole module"""
    from flope_amd.yolo import YoloSeg
    from flope_amd.yolo_weights import synthetic_yolo_state_dict
    if (g.key, dtype) not in _ENGINES:
        if g.nc not in _SD:
            _SD[g.nc] = synthetic_yolo_state_dict(0) if g.nc == 1 else synthetic_yolo_state_dict(1, nc=g.nc, widths=(16, 32, 64, 128, 256), cls_bias=-3.0)
        y = YoloSeg(g.H, g.W, g.imgsz, dtype)
        y.load_state_dict(_SD[g.nc])
        assert y.input_hw == (g.h, g.w) and y.head_dims() == (g.A, 64 + g.nc + 32, g.nc, g.mh, g.mw)
        _ENGINES[(g.key, dtype)] = y
    return _ENGINES[(g.key, dtype)]


def _result(y, out):
    boxes, conf, cls, anchor, mask = out
    return YC.Result(y.read_tensor("cand_box").cpu().numpy()[:, 0].T.copy(), y.read_tensor("cand_conf").cpu().numpy()[0, 0],
                     y.read_tensor("cand_cls").cpu().numpy()[0, 0].astype(np.int64), boxes, conf, cls, anchor,
                     y.read_tensor("mask_lb").cpu().numpy()[0].astype(np.uint8), mask)


def _run(c, dtype="f16", conf=None):
    y = _engine(c.geom, dtype)
    if c.prelude is not None:
        p = c.prelude
        y.postprocess(p.rows, p.proto, p.conf, p.iou, p.max_det)
    return _result(y, y.postprocess(c.rows, c.proto, c.conf if conf is None else conf, c.iou, c.max_det))


@pytest.mark.parametrize("name", YC.NAMES)
def test_case(name):
    c = CASES[name]
    got = _run(c)
    log = []
    keep = YC.check(c, got, log)
    print(f"{name}: {len(keep)} kept, worst relative confidence error {log[0][1]:.2e}, worst box error {log[0][2]:.2e} px")
    if name in YC.OVER_NAMES:
        assert int((got.cand_conf > np.float32(c.conf)).sum()) > YC.CAP           # the over-capacity branch of ynms_kernel ran
    if name == "conf_empty":
        assert len(got.anchor) == 0 and not got.mask.any() and not got.mask_lb.any()
    if name == "stale_first":
        assert len(got.anchor) == 300


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("name", YC.MASK_NAMES)
def test_mask_case_in_every_map_type(name, dtype):
    """f16 / bf16: ymask_low_kernel<T>; f32: y32_mask_low_kernel"""
    c = CASES[name]
    got = _run(c, dtype)
    YC.check(c, got)
    if name != "generic_s64":
        assert got.mask_lb.any()


def test_confidence_at_the_threshold():
    """`conf` equal to the device's own confidence of an anchor: no candidate; one ulp lower: a candidate"""
    c = CASES["conf_zero"]
    got = _run(c)
    v = got.cand_conf[41]
    assert 0 < v < 1 and got.anchor.tolist() == [20, 41, 3, 12]
    assert _run(c, conf=float(v)).anchor.tolist() == [20]
    assert _run(c, conf=float(np.nextafter(v, np.float32(0)))).anchor.tolist() == [20, 41]
    half = got.cand_conf[3]
    assert half == np.float32(0.5) and got.cand_conf[20] == np.float32(1)
    assert _run(c, conf=0.5).anchor.tolist() == [20, 41]
    assert _run(c, conf=float(np.nextafter(np.float32(0.5), np.float32(0)))).anchor.tolist() == [20, 41, 3, 12]


def test_detect_equals_postprocess_of_its_own_rows():
    """the refactor: detect() = forward + the tail; the tail alone, fed detect()'s own head rows and proto map, returns the same"""
    from flope_amd.yolo_weights import synthetic_frame
    g = YC.S64
    img = synthetic_frame(4, g.H, g.W)
    for dtype in ("f16", "f32"):
        y = _engine(g, dtype)
        a = y.detect(img, 0.005, 0.6, 300)
        o = {f"{k}{i}": y.read_tensor(f"{k}{i}").cpu().numpy() for i in range(3) for k in ("box", "cls", "coef")}
        proto = y.read_tensor("proto").cpu()
        cand = [y.read_tensor(k).cpu() for k in ("cand_box", "cand_conf", "cand_cls", "mask_lb")]
        b = y.postprocess(YC.rows_of(g, o), proto, 0.005, 0.6, 300)
        assert len(a[3]) >= 3
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and np.array_equal(u, v)
        for k, t in zip(("cand_box", "cand_conf", "cand_cls", "mask_lb"), cand):
            assert torch.equal(y.read_tensor(k).cpu(), t)
        assert torch.equal(y.read_tensor("proto").cpu(), proto)
        y.set_option("graph", 1)                                    # eager whatever the option says: nothing is captured
        n = y.graph_cache_size()
        c = y.postprocess(YC.rows_of(g, o), proto, 0.005, 0.6, 300)
        assert y.graph_cache_size() == n and all(np.array_equal(u, v) for u, v in zip(a, c))
        y.set_option("graph", 0)


def test_postprocess_error_paths():
    from flope_amd.yolo import YoloSeg
    g = YC.S64
    c = CASES["iou_at"]
    y = YoloSeg(g.H, g.W, g.imgsz)
    lib = y.lib
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    assert lib.flope_yolo_postprocess(None, p, p, 0.25, 0.7, 300, p, p, p, None) != 0
    assert lib.flope_yolo_postprocess(y.handle, p, p, 0.25, 0.7, 300, p, p, p, None) != 0
    assert b"before flope_yolo_load_weights" in lib.flope_yolo_last_error(y.handle)
    y.close()
    y = _engine(g)
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert lib.flope_yolo_postprocess(y.handle, args[0], args[1], 0.25, 0.7, 300, args[2], args[3], args[4], None) != 0
        assert b"NULL argument" in lib.flope_yolo_last_error(y.handle)
    for md in (0, 301):
        with pytest.raises(RuntimeError, match="max_det"):
            y.postprocess(c.rows, c.proto, max_det=md)
    for conf, iou in ((-0.1, 0.7), (1.0, 0.7), (float("nan"), 0.7), (0.25, 0.0), (0.25, 1.5)):
        with pytest.raises(RuntimeError, match="bad thresholds"):
            y.postprocess(c.rows, c.proto, conf, iou)
    with pytest.raises(ValueError, match="expected rows"):
        y.postprocess(c.rows[:-1], c.proto)
    with pytest.raises(ValueError, match="expected rows"):
        y.postprocess(c.rows, c.proto[:, :-1])
    assert _run(c).anchor.tolist() == [27, 28, 35]                  # and the engine still works
