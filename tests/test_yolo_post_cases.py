"""CPU half of the post-processing cases (tests/yolo_post_cases.py): every promise a case makes, checked against the oracle alone, and
the checker itself -- a numpy emulation of the device algorithm passes it on every case, each deliberately broken copy fails it.
The GPU half (tests/test_gpu_yolo_post.py) runs the same cases through the kernels and the same checker."""
import numpy as np
import pytest
import torch

import yolo_post_cases as YC
from oracle import yolo_ref as Y

CASES = YC.all_cases()


def _oracle_keep(c):
    box, conf, cls, _ = YC.oracle_candidates(c)
    return YC.keep_from(c, box, conf, cls), box, conf, cls


def test_geometries():
    assert (YC.S32.h, YC.S32.w, YC.S32.A) == (32, 32, 21)
    assert (YC.S64.h, YC.S64.w, YC.S64.top, YC.S64.left, YC.S64.A, YC.S64.mh) == (64, 64, 9, 0, 84, 16)
    assert Y.letterbox_geometry(33, 47, 64)[2:4] == (9, 10)                                    # odd padding: 9 above, 10 below
    assert (YC.BIG.h, YC.BIG.w, YC.BIG.A, YC.BIG.seg) == (384, 640, 5040, 320) and YC.BIG.A > YC.CAP
    assert set(CASES) == set(YC.NAMES)


@pytest.mark.parametrize("name", YC.NAMES)
def test_boxes_are_exact_floats_where_promised(name):
    c = CASES[name]
    box = YC.oracle_candidates(c)[0]
    assert np.isfinite(box).all()
    if c.exact:                              # distances are multiples of half a cell of 8, 16 or 32 pixels
        assert (box % 4 == 0).all()
    assert c.exact == (not name.startswith("generic") and name != "mask_edges")


@pytest.mark.parametrize("name", YC.NAMES)
def test_confidences_are_equal_or_far_apart(name):
    """crafted cases: two confidences, and a confidence and `conf`, are bit-equal by construction (equal logits; 0.5 = sigmoid(0))
    or at least 4 x the suite's rtol apart, so no exp() of 3e-6 accuracy can reorder them.  Generic rows: only `conf` matters
    (their NMS is judged from the device's own candidates)."""
    c = CASES[name]
    g = c.geom
    conf = YC.oracle_candidates(c)[1]
    conf = conf[~np.isnan(conf)].astype(np.float64)
    near = np.abs(conf - c.conf) < YC.GAP * max(c.conf, 1e-30)
    if name == "conf_half":
        lg = c.rows[:, 64:64 + g.nc].max(1)
        assert near.sum() == 2 and (conf[near] == 0.5).all() and (lg[~np.isnan(lg)][near] == 0).all()
    elif c.conf == 0:
        assert (conf[near] == 0).all()                       # exp overflow: exactly 0 on any device
    else:
        assert not near.any()
    if c.exact:
        u = np.unique(conf[conf > 0])
        assert (np.diff(u) / u[1:] >= YC.GAP).all()
        rows_hi = c.rows[:, 64:64 + g.nc].max(1)
        assert ((rows_hi == YC.OFF) == (YC.oracle_candidates(c)[1] == 0))[~np.isnan(rows_hi)].all()


def test_iou_cases():
    b1, b2 = np.float32([12, 12, 44, 44]), np.float32([20, 12, 52, 44])
    inter = (min(b1[2], b2[2]) - max(b1[0], b2[0])) * (min(b1[3], b2[3]) - max(b1[1], b2[1]))
    ovr = np.float32(inter) / (np.float32(1024) + np.float32(1024) - np.float32(inter))
    assert inter == 768 and ovr == np.float32(YC.IOU_768_1280) == np.float32(CASES["iou_at"].iou) and np.float32(CASES["iou_below"].iou) < ovr
    assert _oracle_keep(CASES["iou_at"])[0].tolist() == [27, 28, 35]
    assert _oracle_keep(CASES["iou_below"])[0].tolist() == [27, 35]
    c = CASES["chain"]
    keep, box, _, _ = _oracle_keep(c)
    assert keep.tolist() == [27, 29]
    assert Y.nms_numpy(box[[28, 29]], [2, 1], c.iou).tolist() == [0]          # alone, B kills C


def test_conf_cases():
    assert _oracle_keep(CASES["conf_half"])[0].tolist() == [20, 41]
    assert _oracle_keep(CASES["conf_zero"])[0].tolist() == [20, 41, 3, 12]
    assert _oracle_keep(CASES["conf_none"])[0].tolist() == [20]
    assert YC.oracle_candidates(CASES["conf_none"])[1][20] == 1.0
    assert _oracle_keep(CASES["conf_empty"])[0].tolist() == []
    assert not YC.emulate(CASES["conf_empty"]).mask.any()


@pytest.mark.parametrize("n", YC.SORT_SIZES)
def test_sort_cases(n):
    c = CASES[f"sort{n}"]
    keep, box, conf, _ = _oracle_keep(c)
    cand = np.nonzero(conf > c.conf)[0]
    assert len(cand) == n
    order = cand[np.lexsort((cand, -conf[cand].astype(np.float64)))]
    assert keep.tolist() == order[:300].tolist()                                   # nothing suppressed: the output is the sort order
    if n >= 63:
        assert len(np.unique(conf[cand])) < n / 1.5                                # ties everywhere ...
        assert len(np.unique(cand // c.geom.seg)) == 16                            # ... from every wave segment of the gather
        k = conf[keep]
        assert (np.diff(keep)[np.diff(k) == 0] > 0).all() and (np.diff(k) == 0).sum() >= min(n, 300) // 3


def _cut(c):
    _, conf, _ = YC.oracle_candidates(c)[:3]
    cand = np.nonzero(conf > c.conf)[0]
    srt = np.sort(conf[cand])[::-1]
    cutv = srt[YC.CAP - 1]
    return cand, conf, cutv


@pytest.mark.parametrize("name", YC.OVER_NAMES)
def test_over_capacity_cases(name):
    c = CASES[name]
    cand, conf, cutv = _cut(c)
    assert len(cand) > YC.CAP
    above, eq = cand[conf[cand] > cutv], cand[conf[cand] == cutv]
    take = YC.CAP - len(above)
    taken, left = eq[:take], eq[take:]
    want = {"over_third": (1680, 3360, 2416, 3623), "over_straddle": (574, 4466, 3522, 3521), "over_distinct": (4095, 1, 1, None),
            "over_4097_tied": (0, 4097, 4096, 4095), "over_ones": (0, 4200, 4096, 4095)}[name]
    assert (len(above), len(eq), take) == want[:3] and (want[3] is None or taken[-1] == want[3])
    if name == "over_straddle":
        assert taken[-1] % c.geom.seg == 1                                         # the taken ties end one anchor into a wave segment
    if name == "over_ones":
        assert cutv == 1.0
    keep = _oracle_keep(c)[0]
    assert len(keep) < 100                                                         # every probe that entered the NMS shows
    small = np.nonzero((YC.oracle_candidates(c)[0][:, 2] - YC.oracle_candidates(c)[0][:, 0]) < 100)[0]      # the probes
    inside = set(above.tolist()) | set(taken.tolist())
    shown = set(keep.tolist()) & set(small.tolist())
    assert shown == set(small.tolist()) & inside
    assert len(shown & set(taken.tolist()) | shown & set(above.tolist())) >= 4 and len(set(small.tolist()) - inside) >= 1
    if len(left):
        assert set(small.tolist()) & set(left.tolist())                            # a tied probe past the cut exists, and stays out


def test_max_det_degenerate_class_and_scale_cases():
    full = _oracle_keep(CASES["maxdet_17"]._replace(max_det=300))[0]
    assert len(full) == 40
    assert _oracle_keep(CASES["maxdet_1"])[0].tolist() == full[:1].tolist()
    assert _oracle_keep(CASES["maxdet_17"])[0].tolist() == full[:17].tolist()
    assert len(_oracle_keep(CASES["maxdet_eq"])[0]) == 17 == CASES["maxdet_eq"].max_det
    assert len(_oracle_keep(CASES["stale_first"]._replace(max_det=300))[0]) == 300 and (YC.oracle_candidates(CASES["stale_first"])[1] > 0.01).sum() == 320
    keep, box, conf, cls = _oracle_keep(CASES["degenerate"])
    assert keep.tolist() == [36, 18, 19, 27] and np.isnan(conf[[50, 51]]).all()
    assert (box[36, 0] == box[36, 2]) and np.array_equal(box[18], box[19]) and box[18, 1] == box[18, 3]
    keep, box, conf, cls = _oracle_keep(CASES["classes"])
    assert keep.tolist() == [27, 28, 35, 0, 7] and cls[keep].tolist() == [0, 1, 2, 1, 0]
    assert all(np.array_equal(box[27], box[a]) for a in (28, 35, 36))
    c = CASES["scale"]
    keep, box, _, _ = _oracle_keep(c)
    g = c.geom
    assert len(keep) == 12
    raw = (box[keep] - np.float32([0, 9, 0, 9])) / np.float32(min(g.h / g.H, g.w / g.W))
    assert (raw[:, 0] < 0).any() and (raw[:, 1] < 0).any() and (raw[:, 2] > g.W).any() and (raw[:, 3] > g.H).any()
    assert (raw[:, 3] < 0).any() and (raw[:, 1] > g.H).any()                       # wholly inside the padding above / below
    sb = Y.scale_boxes((g.h, g.w), box[keep], (g.H, g.W, 3))
    assert sb.min() == 0 and sb[:, [0, 2]].max() == g.W and sb[:, [1, 3]].max() == g.H


@pytest.mark.parametrize("name", YC.NAMES)
def test_proto_and_coefficients_are_small_integers(name):
    c = CASES[name]
    coef = c.rows[:, 64 + c.geom.nc:]
    coef = coef[~np.isnan(coef).any(1)]
    for v in (c.proto, coef):
        assert (v == np.round(v)).all() and np.abs(v).max() <= 8
        t = torch.from_numpy(np.ascontiguousarray(v))
        assert torch.equal(t.to(torch.float16).float(), t) and torch.equal(t.to(torch.bfloat16).float(), t)


def test_mask_edge_case_reaches_every_edge():
    c = CASES["mask_edges"]
    keep, box, _, _ = _oracle_keep(c)
    assert sorted(keep.tolist()) == [0, 9, 12, 20, 21, 30, 41, 45, 50, 63]
    fr = lambda a: (box[a] / 4) % 1
    assert (fr(9) == 0).all() and np.abs(fr(12) - 0.5).max() < 1e-4 and np.abs(fr(41) - 0.125).max() < 1e-4
    assert box[0, 0] < 0 and box[0, 1] < 0 and box[63, 2] > c.geom.w and box[63, 3] > c.geom.h
    assert np.ceil(box[30, 0] / 4) >= box[30, 2] / 4                               # no proto column inside
    one = lambda a: Y.process_mask(c.proto, c.rows[[a], 64 + c.geom.nc:], box[[a]], (64, 64), return_float=True)[0].numpy()
    assert not (one(30) != 0).any()
    m = one(9)
    assert (m > 0)[4:20, 4:20].all() and (m > 0)[10, 2:22].all() and not (m > 0)[10, 22] and not (m > 0)[10, 1]       # the margin's border: 2 px
    m = one(41)
    assert (m > 0)[40, 25] and not (m > 0)[40, 26] and 25 > box[41, 2] + 4         # int + 0.125: 4.5 px past the box, beyond half the margin
    m = one(45)
    assert m[42, 44] == 0 and m[42, 43] > 0 and m[42, 45] < 0 and m[42, 52] == 0   # exactly 0 between a positive and a negative value
    both = one(20) + 0, one(21)
    assert ((both[0] > 0) & (both[1] < 0)).sum() > 50
    e = YC.emulate(c)
    assert e.mask_lb[42, 43] == 255 and e.mask_lb[42, 44] == 0 and e.mask_lb[20, 36] == 255
    d = YC.emulate(CASES["degenerate"])
    assert d.mask_lb[20, 20:29].max() == 255 and d.mask_lb[36, 36] == 255          # under the real box; the point and the lines add nothing
    only = YC.emulate(CASES["degenerate"]._replace(name="degenerate_alone", rows=np.where(np.arange(84)[:, None] == 27, YC.blank_rows(YC.S64), CASES["degenerate"].rows)))
    assert not only.mask_lb.any() and len(only.anchor) == 3


@pytest.mark.parametrize("name", YC.NAMES)
def test_unbroken_emulation_passes(name):
    c = CASES[name]
    YC.check(c, YC.emulate(c))


# the cases each break must be caught by (at least these)
NEEDS = {"iou_ge": ["iou_at", "chain"], "conf_ge": ["conf_half", "conf_zero"], "tie_desc": ["sort64", "sort1025", "degenerate"],
         "cut_from_end": ["over_third", "over_straddle", "over_4097_tied", "over_ones"], "no_cls_offset": ["classes"],
         "max_det_plus": ["maxdet_1", "maxdet_17"], "max_det_minus": ["maxdet_17", "maxdet_eq", "sort1023"], "crop_le": ["mask_edges"],
         "thr_ge": ["mask_edges", "conf_half"], "no_clip": ["scale"], "half_margin": ["mask_edges"], "low_to_max_det": ["stale_second"]}


def test_every_break_is_listed():
    assert set(NEEDS) == set(YC.BREAKS)


@pytest.mark.parametrize("brk", YC.BREAKS)
def test_broken_emulation_is_caught(brk):
    for name in NEEDS[brk]:
        c = CASES[name]
        with pytest.raises(AssertionError):
            YC.check(c, YC.emulate(c, brk))
