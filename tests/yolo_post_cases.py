"""Hand-built head rows for the detector's post-processing (flope_amd/csrc/yolo.hip: ydecode_kernel, ynms_kernel with its box
scaling, ymask_low_kernel / yolo_f32.hip's float32 twin, ymask_merge_kernel) and the checker both halves of their tests share:
tests/test_yolo_post_cases.py (CPU: each case's promises, a numpy emulation of the device algorithm and its broken copies) and
tests/test_gpu_yolo_post.py (the kernels, through YoloSeg.postprocess).

A case is a float32 row block [A][64 DFL logits + nc class logits + 32 coefficients], a proto map [32][mh][mw], thresholds, and
optionally a `prelude` case that runs first on the same engine (stale state).  Everything is built so that a result is decided,
not approximate:
  boxes    a DFL side is 0 at one bin or at two adjacent bins and -1e4 elsewhere: exp underflows to 0, the distance is that bin or
           bin + 0.5 exactly and the box an exact float (`exact`).  Other distances (d not a multiple of 0.5) mix two adjacent
           bins and are good to ~1e-6; cases that use them are judged from the device's own boxes only.
  ties     equal class logits give equal confidence bits on any exp(); confidences meant to differ are GAP apart or more.
  masks    proto values and coefficients are integers of magnitude <= 8: every 32-term sum and every bilinear value at scale 4
           (weights k / 8) is an exact float in any order and in f16 / bf16 storage.
The reference is oracle/yolo_ref.py throughout; nothing here restates it except `Emu`, the device algorithm in numpy, which exists
to show that the checker tells a subtly wrong kernel from a right one.
"""
import collections
import functools

import numpy as np
import torch

from oracle import pipeline_ref as P
from oracle import yolo_ref as Y

RTOL_CONF, ATOL_BOX = 3e-6, 2e-3        # the suite's own decode tolerances (test_gpu_yolo.py: _check_decode_and_nms)
GAP = 4 * RTOL_CONF                     # relative distance of confidences (and of `conf`) that are meant to differ
CAP = 4096                              # kNmsCap
OFF = -1e4                              # a logit that is exactly 0 after exp / sigmoid in float32
MAX_WH = 7680

Geom = collections.namedtuple("Geom", "key H W imgsz nc h w top left A levels mh mw seg")
Case = collections.namedtuple("Case", "name geom rows proto conf iou max_det exact prelude note")
Result = collections.namedtuple("Result", "cand_box cand_conf cand_cls boxes conf cls anchor mask_lb mask")


def geometry(key, H, W, imgsz, nc=1):
    nw, nh, top, bottom, left, right = Y.letterbox_geometry(H, W, imgsz)
    h, w = nh + top + bottom, nw + left + right
    levels, a0 = [], 0
    for s in (8, 16, 32):
        levels.append((a0, h // s, w // s, s))
        a0 += (h // s) * (w // s)
    return Geom(key, H, W, imgsz, nc, h, w, top, left, a0, tuple(levels), h // 4, w // 4, (a0 + 1023) // 1024 * 64)


# engines of the GPU file: (frame, imgsz, classes); "big" is only loaded, never run through the network
S32 = geometry("s32", 32, 32, 32)               # letterbox 32 x 32, A = 21
S64 = geometry("s64", 33, 47, 64)               # letterbox 64 x 64, 9 rows of padding above and 10 below, A = 84
C64 = geometry("c64", 33, 47, 64, nc=3)
BIG = geometry("big", 360, 640, 640)            # letterbox 384 x 640, A = 5040: more anchors than kNmsCap


def anchor_of(g, level, gy, gx):
    a0, gh, gw, _ = g.levels[level]
    assert 0 <= gy < gh and 0 <= gx < gw
    return a0 + gy * gw + gx


def anchor_centre(g, a):
    for a0, gh, gw, s in g.levels:
        if a < a0 + gh * gw:
            return ((a - a0) % gw + 0.5) * s, ((a - a0) // gw + 0.5) * s, s
    raise IndexError(a)


def blank_rows(g):
    """no anchor is a candidate (confidence exactly 0), every box is its anchor point, coefficients 0"""
    r = np.full((g.A, 64 + g.nc + 32), OFF, np.float32)
    r[:, 0:64:16] = 0
    r[:, 64 + g.nc:] = 0
    return r


def set_side(rows, a, side, d):
    """distance `d` (grid units, 0..15) on side 0..3 = left, top, right, bottom.  -> True when the decode is exact"""
    seg = rows[a, side * 16:(side + 1) * 16]
    seg[:] = OFF
    i = int(np.floor(d))
    f = d - i
    seg[i] = 0
    if f == 0.5:
        seg[i + 1] = 0
    elif f:
        seg[i + 1] = np.log(f / (1 - f))
    return f in (0, 0.5)


def set_box(rows, a, l, t, r, b):
    return all([set_side(rows, a, k, d) for k, d in enumerate((l, t, r, b))])


def set_xyxy(g, rows, a, x1, y1, x2, y2):
    cx, cy, s = anchor_centre(g, a)
    return set_box(rows, a, (cx - x1) / s, (cy - y1) / s, (x2 - cx) / s, (y2 - cy) / s)


def set_cls(g, rows, a, logits):
    rows[a, 64:64 + g.nc] = logits


def set_coef(g, rows, a, coef):
    rows[a, 64 + g.nc:] = coef


def unit(k, v=1):
    c = np.zeros(32, np.float32)
    c[k] = v
    return c


def std_proto(g, seed=0):
    """channel 0: +1 everywhere; channel 1: columns 5, -3, 5, -3 ... (3/8 * 5 + 5/8 * -3 = 0 at the pixels whose bilinear weights
    are 3/8, 5/8); channel 2: -1 everywhere; the others: seeded integers in [-8, 8]"""
    rng = np.random.default_rng(seed)
    p = rng.integers(-8, 9, (32, g.mh, g.mw)).astype(np.float32)
    p[0] = 1
    p[1] = np.where(np.arange(g.mw) % 2 == 0, 5, -3)[None, :]
    p[2] = -1
    return p


def case(name, g, rows, proto=None, conf=0.25, iou=0.7, max_det=300, exact=True, prelude=None, note=""):
    return Case(name, g, rows, std_proto(g) if proto is None else proto, float(np.float32(conf)), float(np.float32(iou)), max_det, exact,
                prelude, note)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
IOU_768_1280 = float(np.float32(768) / np.float32(1280))


def _iou_rows():
    g = S64
    r = blank_rows(g)
    for a, box, lg in ((27, (12, 12, 44, 44), 3), (28, (20, 12, 52, 44), 2), (35, (24, 32, 32, 40), 1)):
        assert set_xyxy(g, r, a, *box)
        set_cls(g, r, a, lg)
        set_coef(g, r, a, unit(0))
    return r


def _chain_rows():
    """A kills B (IoU 896/1152), B would have killed C, A and C meet at exactly 768/1280: C survives"""
    g = S64
    r = blank_rows(g)
    for a, box, lg in ((27, (12, 12, 44, 44), 3), (28, (16, 12, 48, 44), 2), (29, (20, 12, 52, 44), 1)):
        assert set_xyxy(g, r, a, *box)
        set_cls(g, r, a, lg)
        set_coef(g, r, a, unit(0))
    return r


def _grid_rows(g, anchors, logits, coef=None):
    """every listed anchor a box of half a cell right / below its point: boxes of one level are disjoint, a box of a coarser level
    holds at most one finer box at IoU <= 1/4"""
    r = blank_rows(g)
    for a, lg in zip(anchors, logits):
        assert set_box(r, a, 0, 0, 0.5, 0.5)
        set_cls(g, r, a, lg)
        if coef is not None:
            set_coef(g, r, a, coef)
    return r


SORT_SIZES = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096)
SORT_LOGITS = np.linspace(-1, 3, 40).astype(np.float32)


def _sort_case(n):
    rng = np.random.default_rng(1000 + n)
    anchors = np.sort(rng.choice(BIG.A, n, replace=False))
    return case(f"sort{n}", BIG, _grid_rows(BIG, anchors, rng.choice(SORT_LOGITS, n)), conf=0.01,
                note="n candidates with many equal confidences, scattered over the gather's wave segments; none suppresses another")


def _overcap_case(name, logits, probes, note):
    """every anchor a candidate.  Probes carry a small box of their own and survive if and only if they entered the NMS; every other
    anchor carries the largest box there is, which at iou = 0.05 leaves a handful of survivors."""
    g = BIG
    r = blank_rows(g)
    probes = set(int(p) for p in probes)
    for a in range(g.A):
        if a in probes:
            assert set_box(r, a, 0, 0, 0.5, 0.5)
        else:
            assert set_box(r, a, 15, 15, 15, 15)
        set_cls(g, r, a, logits[a])
    return case(name, g, r, conf=0.01, iou=0.05, note=note)


def _overcap_cases():
    A = BIG.A
    out = []
    a = np.arange(A)
    # every third anchor distinct and higher (1680), the other 3360 tied: 2416 tied ones enter, the last of them anchor 3623
    lg = np.full(A, -1.0, np.float32)
    hi = a[a % 3 == 0]
    lg[hi] = (0.5 + 1e-3 * np.random.default_rng(5).permutation(len(hi))).astype(np.float32)
    out.append(_overcap_case("over_third", lg, range(3600, 3648), "1680 distinct + the first 2416 of 3360 tied"))
    # 574 distinct higher ones at the end, 4466 tied: the last tied one taken is 3521, one past the wave-segment boundary 3520
    lg = np.full(A, -1.0, np.float32)
    lg[4466:] = (0.5 + 1e-3 * np.arange(574)).astype(np.float32)
    out.append(_overcap_case("over_straddle", lg, range(3500, 3540), "the taken ties end one anchor past a wave-segment boundary"))
    # all distinct: exactly 4096 above the cut, none tied at it
    perm = np.random.default_rng(6).permutation(A)
    lg = np.empty(A, np.float32)
    lg[perm] = (3 - 1e-3 * np.arange(A)).astype(np.float32)
    pr = [int(p) for p in perm[4080:4112] if p < 3840]
    out.append(_overcap_case("over_distinct", lg, pr, "4096 above the cut, no tie"))
    # 4097 tied candidates and nothing else
    lg = np.full(A, OFF, np.float32)
    lg[:4097] = 1
    out.append(_overcap_case("over_4097_tied", lg, range(4088, 4097), "4097 equal confidences: the last one stays out"))
    # 4200 confidences of exactly 1.0f
    lg = np.zeros(A, np.float32)
    lg[:4200] = 30
    out.append(_overcap_case("over_ones", lg, range(4088, 4104), "more than 4096 confidences of exactly 1.0f"))
    return out


def _conf_rows():
    """sigmoid(0) = 0.5 and sigmoid(30) = 1 exactly, on any exp()"""
    g = S64
    r = _grid_rows(g, [3, 12, 20, 41], [0, 0, 30, 1], unit(0))
    return r


def _maxdet_rows(n):
    g = S64
    return _grid_rows(g, np.arange(n), np.linspace(3, -1, n).astype(np.float32)[np.random.default_rng(n).permutation(n)], unit(0))


def _degenerate_rows():
    g = S64
    r = blank_rows(g)
    assert set_xyxy(g, r, 27, 12, 12, 44, 44); set_cls(g, r, 27, 1); set_coef(g, r, 27, unit(0))       # a real box
    set_cls(g, r, 36, 3); set_coef(g, r, 36, unit(0))                                                   # a point inside it, more confident
    assert set_xyxy(g, r, 18, 20, 20, 28, 20); set_cls(g, r, 18, 2); set_coef(g, r, 18, unit(0))        # a line, and the same line
    assert set_xyxy(g, r, 19, 20, 20, 28, 20); set_cls(g, r, 19, 2); set_coef(g, r, 19, unit(0))        # from the next anchor
    set_cls(g, r, 50, np.nan)                                                                           # never a candidate
    set_cls(g, r, 51, np.nan); r[51, 64 + g.nc:] = np.nan
    return r


def _class_rows():
    """the box [20, 20, 44, 44] from four anchors: classes 0, 1, 2 and class 0 again (suppressed); one row whose two best class
    logits are equal bits (argmax: the first)"""
    g = C64
    r = blank_rows(g)
    for a, lg in ((27, (3, OFF, OFF)), (28, (OFF, 2.5, OFF)), (35, (OFF, -1, 2)), (36, (1.5, OFF, OFF))):
        assert set_xyxy(g, r, a, 20, 20, 44, 44)
        set_cls(g, r, a, lg)
        set_coef(g, r, a, unit(0))
    assert set_box(r, 0, 0, 0, 0.5, 0.5)
    set_cls(g, r, 0, (OFF, 1, 1))
    assert set_box(r, 7, 0, 0, 0.5, 0.5)
    set_cls(g, r, 7, (1, 1, 1))
    return r


def _scale_rows():
    """boxes that leave the letterbox on every side, and boxes wholly inside the padding rows (9 above, 10 below)"""
    g = S64
    r = blank_rows(g)
    lg = iter(np.linspace(3, 0, 12).astype(np.float32))
    for a, d in ((0, (15, 15, 1, 1)), (7, (1, 15, 15, 1)), (56, (15, 1, 1, 15)), (63, (1, 1, 15, 15)), (27, (15, 15, 15, 15)),
                 (2, (0.5, 0.5, 0.5, 0.5)), (5, (0, 0.5, 1, 0)), (58, (0.5, 0, 0.5, 0.5)), (61, (1, 0, 0, 0.5)),
                 (anchor_of(g, 1, 1, 1), (0.5, 1, 1.5, 0.5)), (anchor_of(g, 2, 1, 0), (0, 15, 15, 0)), (34, (2.5, 0.5, 0, 3))):
        assert set_box(r, a, *d)
        set_cls(g, r, a, next(lg))
        set_coef(g, r, a, unit(0))
    return r


def _mask_edge_rows():
    g = S64
    r = blank_rows(g)
    ex = True
    lg = iter(np.linspace(3, 0, 16).astype(np.float32))

    def inst(a, box, coef):
        nonlocal ex
        ex = set_xyxy(g, r, a, *box) and ex
        set_cls(g, r, a, next(lg))
        set_coef(g, r, a, coef)
    inst(9, (4, 4, 20, 20), unit(0))                      # every edge / 4 an integer
    inst(12, (30, 6, 42, 18), unit(0))                    # edges / 4 at integer + 0.5
    inst(41, (8.5, 36.5, 20.5, 48.5), unit(0))            # edges / 4 at integer + 0.125 (two-bin mix: good to ~1e-6)
    inst(0, (-20, -12, 8, 8), unit(0))                    # below 0
    inst(63, (56, 52, 100, 72), unit(0))                  # beyond iw and ih
    inst(30, (50, 26, 52, 36), unit(0, 3))                # narrower than one proto pixel: [12.5, 13) holds no integer
    inst(45, (40, 40, 56, 48), unit(1))                   # columns 5, -3: the interpolated value is exactly 0 at x = 44, 52
    inst(20, (32, 16, 48, 24), unit(0))                   # a positive and a negative instance on the same pixels
    inst(21, (32, 16, 52, 24), unit(0, -1))
    inst(50, (16, 52, 32, 60), np.random.default_rng(3).integers(-8, 9, 32).astype(np.float32))
    return r, ex


def _stale_cases():
    g = BIG
    rng = np.random.default_rng(9)
    first = np.sort(rng.choice(3840, 320, replace=False))
    a = case("stale_first", g, _grid_rows(g, first, np.linspace(3, -1, 320).astype(np.float32), unit(0)), conf=0.01,
             note="300 all-positive instances kept, 20 more waiting")
    r = blank_rows(g)
    assert set_xyxy(g, r, anchor_of(g, 1, 10, 10), 120, 120, 200, 200); set_cls(g, r, anchor_of(g, 1, 10, 10), 2); set_coef(g, r, anchor_of(g, 1, 10, 10), unit(0))
    assert set_xyxy(g, r, anchor_of(g, 0, 40, 70), 540, 300, 580, 340); set_cls(g, r, anchor_of(g, 0, 40, 70), 1); set_coef(g, r, anchor_of(g, 0, 40, 70), unit(2))
    return a, case("stale_second", g, r, conf=0.01, prelude=a, note="2 instances after 300: no stale row of `low`, no stale box")


def _generic_case(g, seed):
    rng = np.random.default_rng(seed)
    r = np.empty((g.A, 64 + g.nc + 32), np.float32)
    r[:, :64] = rng.normal(0, 2, (g.A, 64))
    r[:, 64:64 + g.nc] = rng.normal(0, 2, (g.A, g.nc))
    r[:, 64 + g.nc:] = rng.integers(-8, 9, (g.A, 32))
    return case(f"generic_{g.key}", g, r, conf=0.25, iou=0.45, exact=False, note="random logits; integer coefficients")


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = [case("iou_at", S64, _iou_rows(), conf=0.05, iou=IOU_768_1280, note="IoU = threshold: both kept"),
          case("iou_below", S64, _iou_rows(), conf=0.05, iou=np.nextafter(np.float32(IOU_768_1280), np.float32(0)), note="one ulp lower: suppressed"),
          case("chain", S64, _chain_rows(), conf=0.05, iou=IOU_768_1280, note="A kills B, so B cannot kill C"),
          case("conf_half", S64, _conf_rows(), conf=0.5, note="conf = 0.5 = two confidences: not candidates"),
          case("conf_zero", S64, _conf_rows(), conf=0.0, note="conf = 0 is legal; confidences of exactly 0 stay out"),
          case("conf_none", S64, _conf_rows(), conf=0.9999, note="1.0 > 0.9999 only"),
          case("conf_empty", S64, _grid_rows(S64, [3, 12, 41], [0, 0, 1], unit(0)), conf=0.9999, note="no candidate: count 0, mask all zero"),
          case("maxdet_1", S64, _maxdet_rows(40), conf=0.05, max_det=1),
          case("maxdet_17", S64, _maxdet_rows(40), conf=0.05, max_det=17),
          case("maxdet_eq", S64, _maxdet_rows(17), conf=0.05, max_det=17, note="max_det = survivors"),
          case("degenerate", S64, _degenerate_rows(), conf=0.05, note="zero-area boxes (0/0 overlap), NaN class logits"),
          case("classes", C64, _class_rows(), conf=0.05, iou=0.5, note="class offset, argmax on equal logits"),
          case("scale", S64, _scale_rows(), conf=0.05, iou=0.9, note="clip on every side, odd padding"),
          _generic_case(S32, 21), _generic_case(S64, 84)]
    r, ex = _mask_edge_rows()
    cs.append(case("mask_edges", S64, r, conf=0.05, iou=0.99, exact=ex, note="crop and threshold at every kind of box edge"))
    cs += [_sort_case(n) for n in SORT_SIZES]
    cs += _overcap_cases()
    cs += list(_stale_cases())
    assert len({c.name for c in cs}) == len(cs)
    return {c.name: c for c in cs}


NAMES = ("iou_at", "iou_below", "chain", "conf_half", "conf_zero", "conf_none", "conf_empty", "maxdet_1", "maxdet_17", "maxdet_eq", "degenerate",
         "classes", "scale", "generic_s32", "generic_s64", "mask_edges") + tuple(f"sort{n}" for n in SORT_SIZES) + (
         "over_third", "over_straddle", "over_distinct", "over_4097_tied", "over_ones", "stale_first", "stale_second")
MASK_NAMES = ("mask_edges", "degenerate", "scale", "generic_s64", "stale_second")       # run in f16, bf16 and f32 engines
OVER_NAMES = ("over_third", "over_straddle", "over_distinct", "over_4097_tied", "over_ones")


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def head_dict(g, rows):
    """rows [A][no] -> the oracle's per-level dict (box / cls / coef [1, C, gh, gw])"""
    o = {}
    for i, (a0, gh, gw, _) in enumerate(g.levels):
        blk = torch.from_numpy(np.ascontiguousarray(rows[a0:a0 + gh * gw])).t().reshape(-1, gh, gw)
        o[f"box{i}"], o[f"cls{i}"], o[f"coef{i}"] = blk[None, :64], blk[None, 64:64 + g.nc], blk[None, 64 + g.nc:]
    return o


def rows_of(g, o):
    """the inverse: per-level [C, gh, gw] maps (read_tensor) -> rows [A][no]"""
    return np.concatenate([np.concatenate([np.asarray(o[f"{k}{i}"]).reshape(-1, gh * gw).T for k in ("box", "cls", "coef")], 1)
                           for i, (a0, gh, gw, _) in enumerate(g.levels)], 0).astype(np.float32)


_ORACLE = {}


def oracle_candidates(c):
    if c.name not in _ORACLE:
        with np.errstate(all="ignore"):
            pred = Y.decode(head_dict(c.geom, c.rows)).numpy()
            box, conf, cls = Y.candidates(pred, c.geom.nc)
        _ORACLE[c.name] = (box, conf, cls, pred)
    return _ORACLE[c.name]


def keep_from(c, box, conf, cls):
    with np.errstate(all="ignore"):
        return Y.nms_candidates(box, np.where(np.isnan(conf), np.float32(-1), conf), cls, np.float32(c.conf), np.float32(c.iou), c.max_det,
                                max_nms=CAP)


_MASKS = {}


def merged_from(c, lb_boxes, keep):
    """the merged letterbox mask of ops.process_mask (> 0, any instance) for the given kept boxes, and its resize to the frame"""
    g = c.geom
    key = (c.name, np.asarray(lb_boxes, np.float32).tobytes(), np.asarray(keep).tobytes())
    if key not in _MASKS:
        coef = c.rows[keep, 64 + g.nc:]
        lb = np.zeros((g.h, g.w), bool)
        for i in range(0, len(keep), 50):
            m = Y.process_mask(c.proto, np.nan_to_num(coef[i:i + 50]), lb_boxes[i:i + 50], (g.h, g.w)).numpy()
            lb |= m.any(0)
        lb = lb.astype(np.uint8) * 255
        _MASKS.clear()
        _MASKS[key] = (lb, P.resize_linear_u8(lb, (g.W, g.H)))
    return _MASKS[key]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check(c, got, log=None):
    """`got` (a Result, from the device or from Emu) against the oracle.  Exact cases tolerate nothing and leave nothing out."""
    g = c.geom
    rbox, rconf, rcls, pred = oracle_candidates(c)
    nan = np.isnan(rconf)
    ok = ~nan
    assert got.cand_conf.shape == rconf.shape and got.cand_box.shape == rbox.shape
    assert not (got.cand_conf[nan] > 0).any(), "a row with NaN class logits has a confidence"
    nz = ok & (rconf != 0)
    dconf = float(np.abs(got.cand_conf[nz].astype(np.float64) / rconf[nz] - 1).max()) if nz.any() else 0.0
    dbox = float(np.abs(got.cand_box.astype(np.float64) - rbox).max())
    if log is not None:
        log.append((c.name, float(dconf), dbox))
    np.testing.assert_allclose(got.cand_conf[ok], rconf[ok], rtol=RTOL_CONF, atol=0)
    if c.exact:
        assert np.array_equal(bits(got.cand_box), bits(rbox)), f"{c.name}: decoded boxes differ by up to {dbox}"
        assert np.array_equal(got.cand_cls[ok], rcls[ok])
    else:
        np.testing.assert_allclose(got.cand_box, rbox, atol=ATOL_BOX)
        sc = np.sort(pred[:, 4:4 + g.nc], 1)
        sure = ok & ((sc[:, -1] - sc[:, -2] > 1e-5) if g.nc > 1 else True)
        assert np.array_equal(got.cand_cls[sure], rcls[sure])
    # NMS, box scaling and masks from the candidates `got` itself decoded
    keep = keep_from(c, got.cand_box, got.cand_conf, got.cand_cls)
    assert got.anchor.tolist() == keep.tolist(), (c.name, len(got.anchor), len(keep), got.anchor.tolist()[:12], keep.tolist()[:12])
    if c.exact:                  # ... and, confidences being GAP apart or equal, from the oracle's own
        assert keep.tolist() == keep_from(c, rbox, rconf, rcls).tolist()
    assert np.array_equal(bits(got.conf), bits(got.cand_conf[keep])) and np.array_equal(got.cls, got.cand_cls[keep])
    ref_boxes = Y.scale_boxes((g.h, g.w), got.cand_box[keep], (g.H, g.W, 3)) if len(keep) else np.zeros((0, 4), np.float32)
    assert np.array_equal(bits(got.boxes), bits(ref_boxes)), (c.name, got.boxes, ref_boxes)
    ref_lb, ref_mask = merged_from(c, got.cand_box[keep], keep)
    assert got.mask_lb.shape == ref_lb.shape and got.mask_lb.dtype == np.uint8
    assert np.array_equal(got.mask_lb, ref_lb), (c.name, int((got.mask_lb != ref_lb).sum()), np.argwhere(got.mask_lb != ref_lb)[:8].tolist())
    assert np.array_equal(got.mask, ref_mask)
    return keep


# ---- the device algorithm in numpy, and its broken copies --------------------------------------------------------------------------
BREAKS = ("iou_ge", "conf_ge", "tie_desc", "cut_from_end", "no_cls_offset", "max_det_plus", "max_det_minus", "crop_le", "thr_ge", "no_clip",
          "half_margin", "low_to_max_det")
F = np.float32


class Emu:
    """One engine's post-processing state (`low`, `det_lb` survive a call, as on the device) and the algorithm of ynms_kernel,
    ymask_low_kernel and ymask_merge_kernel step by step.  brk: one of BREAKS, or None."""

    def __init__(self, g, brk=None):
        self.g, self.brk = g, brk
        self.low = np.zeros((300, g.mh, g.mw), np.float32)
        self.det_lb = np.zeros((300, 4), np.float32)

    def candidates(self, conf, thr):
        brk = self.brk
        ok = (conf >= thr) if brk == "conf_ge" else (conf > thr)
        idx = np.nonzero(ok)[0]
        if len(idx) <= CAP:
            return idx
        u = conf.view(np.uint32)[idx].astype(np.int64)
        lo, hi = 0, 0x3f800000
        while lo < hi:                                   # smallest cut with count(bits > cut) <= kNmsCap
            mid = lo + ((hi - lo) >> 1)
            if int((u > mid).sum()) <= CAP:
                hi = mid
            else:
                lo = mid + 1
        above, eq = idx[u > lo], idx[u == lo]
        take = CAP - len(above)
        return np.concatenate([above, eq[len(eq) - take:] if brk == "cut_from_end" else eq[:take]])

    def run(self, c):
        g, brk = self.g, self.brk
        with np.errstate(all="ignore"):
            box, conf, cls, _ = oracle_candidates(c)
            conf = np.where(np.isnan(conf), F(-1), conf).astype(np.float32)
            thr, iou = F(c.conf), F(c.iou)
            idx = self.candidates(conf, thr)
            order = np.lexsort((idx if brk != "tie_desc" else -idx, -conf[idx].astype(np.float64)))       # conf descending, anchor ascending
            idx = idx[order]
            off = (cls[idx].astype(np.float32) * F(0 if brk == "no_cls_offset" else MAX_WH))[:, None]
            b = (box[idx] + off).astype(np.float32)
            area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(np.float32)
            dead = np.zeros(len(idx), bool)
            limit = c.max_det + (1 if brk == "max_det_plus" else -1 if brk == "max_det_minus" else 0)
            kept = []
            for i in range(len(idx)):
                if dead[i]:
                    continue
                kept.append(i)
                if len(kept) >= limit:
                    break
                w = np.maximum(F(0), np.minimum(b[i, 2], b[i + 1:, 2]) - np.maximum(b[i, 0], b[i + 1:, 0]))
                h = np.maximum(F(0), np.minimum(b[i, 3], b[i + 1:, 3]) - np.maximum(b[i, 1], b[i + 1:, 1]))
                inter = (w * h).astype(np.float32)
                ovr = inter / ((area[i] + area[i + 1:]).astype(np.float32) - inter)
                dead[i + 1:] |= (ovr >= iou) if brk == "iou_ge" else (ovr > iou)
            kept = kept[:300]
            anchor = idx[kept]
            n = len(anchor)
            # box scaling (the values ynms_kernel holds: gain and pads of ops.scale_boxes)
            gain = F(min(g.h / g.H, g.w / g.W))
            pad = np.array([round((g.w - g.W * min(g.h / g.H, g.w / g.W)) / 2 - 0.1), round((g.h - g.H * min(g.h / g.H, g.w / g.W)) / 2 - 0.1)] * 2, np.float32)
            lb = box[anchor].astype(np.float32)
            fr = ((lb - pad) / gain).astype(np.float32)
            if brk != "no_clip":
                fr = np.minimum(np.maximum(fr, F(0)), np.array([g.W, g.H] * 2, np.float32))
            self.det_lb[:n] = lb
            # ymask_low_kernel
            m = min(n, c.max_det)
            xs, ys = np.arange(g.mw, dtype=np.float32)[None, :], np.arange(g.mh, dtype=np.float32)[:, None]
            wr, hr = F(g.mw / g.w), F(g.mh / g.h)
            proto = c.proto.reshape(32, -1)
            for i in range(m):
                x1, y1, x2, y2 = lb[i, 0] * wr, lb[i, 1] * hr, lb[i, 2] * wr, lb[i, 3] * hr
                inside = (xs >= x1) & ((xs <= x2) if brk == "crop_le" else (xs < x2)) & (ys >= y1) & (ys < y2)
                coef = c.rows[anchor[i], 64 + g.nc:]
                v = np.zeros(g.mh * g.mw, np.float32)
                if inside.any():
                    for k in range(32):
                        v = (v + coef[k] * proto[k]).astype(np.float32)
                self.low[i] = np.where(inside, v.reshape(g.mh, g.mw), F(0))
            # ymask_merge_kernel
            lbm = np.zeros((g.h, g.w), bool)
            margin = F(2) * F(g.w) / F(g.mw) * (F(0.5) if brk == "half_margin" else F(1))
            sch, scw = F(g.mh) / F(g.h), F(g.mw) / F(g.w)
            fy = np.maximum(sch * (np.arange(g.h, dtype=np.float32) + F(0.5)) - F(0.5), F(0))
            fx = np.maximum(scw * (np.arange(g.w, dtype=np.float32) + F(0.5)) - F(0.5), F(0))
            y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
            y1, x1 = np.minimum(y0 + 1, g.mh - 1), np.minimum(x0 + 1, g.mw - 1)
            ly1, lx1 = (fy - y0).astype(np.float32), (fx - x0).astype(np.float32)
            ly0, lx0 = F(1) - ly1, F(1) - lx1
            X, Yp = np.arange(g.w, dtype=np.float32), np.arange(g.h, dtype=np.float32)
            for i in range(c.max_det if brk == "low_to_max_det" else m):
                bx = self.det_lb[i]
                cx = np.nonzero(~((X < bx[0] - margin) | (X > bx[2] + margin)))[0]
                cy = np.nonzero(~((Yp < bx[1] - margin) | (Yp > bx[3] + margin)))[0]
                if not len(cx) or not len(cy):
                    continue
                L = self.low[i]
                yy0, yy1, xx0, xx1 = y0[cy][:, None], y1[cy][:, None], x0[cx][None, :], x1[cx][None, :]
                top = lx0[cx][None, :] * L[yy0, xx0] + lx1[cx][None, :] * L[yy0, xx1]
                bot = lx0[cx][None, :] * L[yy1, xx0] + lx1[cx][None, :] * L[yy1, xx1]
                v = ly0[cy][:, None] * top + ly1[cy][:, None] * bot
                lbm[np.ix_(cy, cx)] |= (v >= 0) if brk == "thr_ge" else (v > 0)
            mask_lb = lbm.astype(np.uint8) * 255
            return Result(box, conf, cls, fr, conf[anchor], cls[anchor], anchor, mask_lb, P.resize_linear_u8(mask_lb, (g.W, g.H)))


def emulate(c, brk=None):
    e = Emu(c.geom, brk)
    if c.prelude is not None:
        e.run(c.prelude)
    return e.run(c)
