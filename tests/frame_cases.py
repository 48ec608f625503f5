"""Cases of the frame handle (flope_amd/csrc/frame.hip: frame_select_kernel, flope_frame_select / enqueue / finish) and the checker
both halves of its tests share: tests/test_frame_cases.py (CPU: the arithmetic of flope_amd/csrc/frame_plan.h through
tests/host_harness/harness_frame.cpp, the builder's promises, an emulation of the kernel and its broken copies) and
tests/test_gpu_frame_cases.py (the handle itself: selection, capacity, slots, the host path, failed calls, call order).

Two kinds of case.

A selection case is (name, W, H, cap, max_det, det, count): `det` float32 [rows, 8] holds the detector table in its first max_det
rows and in-frame rows behind it (what a kernel that does not clamp the count would read: device memory the test owns), `count` is
what the detector reports.  The expected boxes are the two Python statements of the reference's loop
(sunflower.predictor.fast_pose_predictor.select_boxes, oracle.pipeline_ref.select_boxes) on det[:n, :4].astype(int16); the rows a
reader cannot do in their head carry their answer by hand in ROWS / WIDE_ROWS.

A frame is (name, rgb, mask, depth, det, count) at H, W = 96, 128 for a handle with crop 64, max_boxes 12 and an engine of batch
4.  Every frame has its own seeded rgb, mask background and uint16 depth (its own mean distance too), so that a buffer read from
another slot changes the answer.  mask is 255 in a blob 6 pixels larger than each box that is meant to have reliable depth
(the 10 x 10 erosion element reaches 5) and at most 100 elsewhere.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pipeline_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_COUNT = 50                # image_manipulation.py: reliable = at least 50 eroded-valid pixels
SENTINEL = -7777              # what the emulation's box memory holds where nothing was stored

SelCase = collections.namedtuple("SelCase", "name W H cap max_det det count")
Frame = collections.namedtuple("Frame", "name rgb mask depth det count")


# ---- the arithmetic, from the header the kernel includes ---------------------------------------------------------------------------------
def load_plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_frame.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_frame.so"])
    lib = C.CDLL(path)
    lib.frame_boxes.restype = None
    return lib


def plan_boxes(lib, rows, W, H):
    """frame_plan.h's frame_box over float32 rows [n, >= 4] -> (keep bool [n], good int32 [n, 4], sq int32 [n, 4]) of every row"""
    rows = np.asarray(rows, dtype=np.float32)
    n = len(rows)
    det = np.zeros((n, lib.frame_det_row()), np.float32)
    det[:, :4] = rows[:, :4]
    keep, good, sq = np.zeros(n, np.int32), np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
    lib.frame_boxes(det.ctypes.data_as(C.c_void_p), n, int(W), int(H), keep.ctypes.data_as(C.c_void_p), good.ctypes.data_as(C.c_void_p),
                    sq.ctypes.data_as(C.c_void_p))
    return keep.astype(bool), good, sq


# ---- selection rows ------------------------------------------------------------------------------------------------------------------------
SW, SH = 640, 480
# (x0, y0, x1, y1) as the detector leaves them; the square by hand; kept?
ROWS = [
    # the known answers of test_frame_box_selection_on_the_device_is_integer_exact
    ((10, 20, 50, 40), (10, 10, 50, 50), True),
    ((0, 0, 10, 5), (0, -3, 10, 7), False),
    ((SW - 40, 100, SW, 140), (SW - 40, 100, SW, 140), True),
    ((100, SH - 40, 140, SH), (100, SH - 40, 140, SH), True),
    ((3, 3, 4, 200), (-95, 3, 102, 200), False),
    ((SW - SH, 0, SW, SH), (SW - SH, 0, SW, SH), True),
    ((7, 9, 20, 22), (7, 9, 20, 22), True),
    ((7, 9, 21, 22), (7, 8, 21, 22), True),                     # w > h, d = 1: the min edge alone moves
    ((7, 9, 20, 24), (6, 9, 21, 24), True),                     # h > w, d = 2
    ((SW - 11, 10, SW - 1, 31), (SW - 17, 10, SW + 4, 31), False),
    # d odd and even on the other axis of each
    ((7, 9, 22, 22), (7, 8, 22, 23), True),                     # w > h, d = 2
    ((7, 9, 20, 25), (5, 9, 21, 25), True),                     # h > w, d = 3: lo = 2, hi = 1
    # inverted in x (w = -20, h = 10: h > w, d = 30, the x edges cross and form a 10 x 10 square), in y, in both (w = -20, h = -10:
    # d = 10, the square stays inverted), with x0 beyond the frame, and one whose min edge leaves the frame
    ((50, 40, 30, 50), (35, 40, 45, 50), True),
    ((40, 50, 50, 30), (40, 35, 50, 45), True),
    ((50, 60, 30, 50), (45, 60, 35, 50), True),
    ((660, 40, 600, 50), (625, 40, 635, 50), True),
    ((5, 40, -20, 50), (-13, 40, -3, 50), False),               # d = 35: lo = 18, hi = 17
    # zero area: inside, on the far edge, in the corner; zero width with a height
    ((100, 100, 100, 100), (100, 100, 100, 100), True),
    ((SW, 200, SW, 200), (SW, 200, SW, 200), True),
    ((SW, SH, SW, SH), (SW, SH, SW, SH), True),
    ((100, 100, 100, 120), (90, 100, 110, 120), True),
    # truncation toward zero: -0.5 and -0.999 are 0, -1.0 is -1; fractions that a rounding cast would move
    ((-0.5, -0.999, 20, 20), (0, 0, 20, 20), True),
    ((-1.0, 0, 19, 20), (-1, 0, 19, 20), False),
    ((0, -1.0, 20, 19), (0, -1, 20, 19), False),
    ((10.6, 20.7, 50.5, 40.9), (10, 10, 50, 50), True),
    # the square touches W, H and 0 exactly; one further it leaves
    ((SW - 21, 100, SW - 3, 124), (SW - 24, 100, SW, 124), True),
    ((SW - 21, 100, SW - 2, 125), (SW - 24, 100, SW + 1, 125), False),
    ((100, SH - 21, 124, SH - 3), (100, SH - 24, 124, SH), True),
    ((100, SH - 21, 125, SH - 2), (100, SH - 24, 125, SH + 1), False),
    ((3, 100, 21, 124), (0, 100, 24, 124), True),
    ((2, 100, 20, 124), (-1, 100, 23, 124), False),
    ((100, 3, 124, 21), (100, 0, 124, 24), True),
    ((100, 2, 124, 20), (100, -1, 124, 23), False),
    # one pixel
    ((0, 0, 1, 1), (0, 0, 1, 1), True),
    ((SW - 1, SH - 1, SW, SH), (SW - 1, SH - 1, SW, SH), True),
    ((300, 200, 301, 201), (300, 200, 301, 201), True),
]
# a frame at the handle's limit: 32767 x 16
WW, WH = 32767, 16
WIDE_ROWS = [
    ((32751, 0, 32767, 16), (32751, 0, 32767, 16), True),
    ((32757, 3, 32767, 13), (32757, 3, 32767, 13), True),
    ((32760, 0, 32767, 16), (32755, 0, 32771, 16), False),     # w = 7, h = 16, d = 9: lo = 5, hi = 4
    ((0, 0, 16, 16), (0, 0, 16, 16), True),
    ((32766.5, 15.5, 32767, 16), (32766, 15, 32767, 16), True),
    ((32000, 4, 32012, 8), (32000, 0, 32012, 12), True),
    ((32000, 4, 32014, 8), (32000, -1, 32014, 13), False),
    ((32767, 16, 32767, 16), (32767, 16, 32767, 16), True),
]
SEL_COUNTS = (0, 1, 63, 64, 65, 130)
SEL_ROWS = 130                # the table of the 640 x 480 cases
SEL_BEHIND = 10               # in-frame rows behind the table


def _random_rows(rng, n, W, H):
    """the generator of test_frame_box_selection_on_the_device_is_integer_exact: well-formed boxes with fractional coordinates"""
    det = np.zeros((n, 8), np.float32)
    x0, y0 = rng.uniform(0, W - 2, n), rng.uniform(0, H - 2, n)
    det[:, 0], det[:, 1] = x0, y0
    det[:, 2], det[:, 3] = np.minimum(x0 + rng.uniform(1, 220, n), W), np.minimum(y0 + rng.uniform(1, 220, n), H)
    det[:, 4] = rng.uniform(0.25, 1, n)
    return det


def _table(rows, n, W, H, seed):
    """`rows` first, random rows up to n, then SEL_BEHIND small squares that are in any frame"""
    det = _random_rows(np.random.default_rng(seed), n + SEL_BEHIND, W, H)
    det[:len(rows), :4] = np.array([r[0] for r in rows], np.float32)
    for k in range(SEL_BEHIND):
        det[n + k, :4] = (1 + k, 2, 9 + k, 10)
    return det


def selection_cases():
    det = _table(ROWS, SEL_ROWS, SW, SH, 41)
    out = [SelCase(f"rows_{c}", SW, SH, 300, SEL_ROWS, det, c) for c in SEL_COUNTS]
    out.append(SelCase("count_above_table", SW, SH, 300, SEL_ROWS, det, SEL_ROWS + 7))
    out.append(SelCase("count_negative", SW, SH, 300, SEL_ROWS, det, -3))
    out.append(SelCase("cap_12", SW, SH, 12, SEL_ROWS, det, 65))
    wide = _table(WIDE_ROWS, 16, WW, WH, 42)
    wide[len(WIDE_ROWS):16, :4] = 0
    wide[len(WIDE_ROWS):16, 2:4] = (8, 8)
    out.append(SelCase("wide", WW, WH, 16, 16, wide, 16))
    for c in out:
        c.det.setflags(write=False)
    return out


_SEL = {}


def selection_case(name):
    if not _SEL:
        _SEL.update({c.name: c for c in selection_cases()})
    return _SEL[name]


SEL_NAMES = tuple(f"rows_{c}" for c in SEL_COUNTS) + ("count_above_table", "count_negative", "cap_12", "wide")


def host_loop(bb16, H, W):
    """both Python statements of the reference's loop on int16 rows -> (good int32 [k, 4], sq int32 [k, 4]); they must agree"""
    from sunflower.predictor.fast_pose_predictor import select_boxes
    _, sq_m, good_m = select_boxes(bb16, (H, W, 3))
    with np.errstate(over="ignore"):                                  # (the oracle's box centre adds two int16: not read here)
        _, sq_o, good_o = P.select_boxes(bb16, (H, W, 3))
    good_m, sq_m = good_m.astype(np.int32).reshape(-1, 4), sq_m.astype(np.int32).reshape(-1, 4)
    good_o, sq_o = np.asarray(good_o, dtype=np.int32).reshape(-1, 4), np.asarray(sq_o, dtype=np.int32).reshape(-1, 4)
    assert np.array_equal(good_m, good_o) and np.array_equal(sq_m, sq_o), "the two Python statements of the loop disagree"
    return good_m, sq_m


_SEL_REF = {}


def selection_reference(c):
    """-> (in_frame, good [k, 4], sq [k, 4]) with k = min(in_frame, cap): what flope_frame_select must leave in the slot"""
    if c.name not in _SEL_REF:
        n = min(max(c.count, 0), c.max_det)
        good, sq = host_loop(c.det[:n, :4].astype(np.int16), c.H, c.W)
        _SEL_REF[c.name] = (len(good), good[:c.cap], sq[:c.cap])
    return _SEL_REF[c.name]


def check_selection(c, good, sq, in_frame=None):
    """boxes read back from one select of case c (the kept ones, `cap` at most) -> list of failures; integer for integer"""
    total, good_ref, sq_ref = selection_reference(c)
    good, sq = np.asarray(good).reshape(-1, 4), np.asarray(sq).reshape(-1, 4)
    fails = []
    if in_frame is not None and in_frame != total:
        fails.append(f"{c.name}: {in_frame} boxes in frame, expected {total}")
    if len(good) != len(good_ref) or len(sq) != len(sq_ref):
        return fails + [f"{c.name}: {len(good)} / {len(sq)} boxes kept, expected {len(good_ref)}"]
    for i in np.nonzero((good != good_ref).any(axis=1) | (sq != sq_ref).any(axis=1))[0]:
        fails.append(f"{c.name} box {i}: {good[i].tolist()} -> {sq[i].tolist()}, expected {good_ref[i].tolist()} -> {sq_ref[i].tolist()}")
    return fails


# ---- frames --------------------------------------------------------------------------------------------------------------------------------
FH, FW, CROP, ENGINE_BATCH, MAX_BOXES, SLOTS, MAX_DET = 96, 128, 64, 4, 12, 3, 16
K = np.array([[100.5, 0, FW / 2 + 0.25], [0, 99.25, FH / 2 - 0.25], [0, 0, 1.0]])      # exact in float32
DEPTH_DIV, NEAR, FAR = 1000.0, 0.1, 2.5

_F0 = [(8, 8, 40, 36), (50, 10, 70, 40), (80, 20, 120, 60), (10, 50, 40, 90), (60, 60, 78, 80)]
_F1 = [(100, 5, 126, 60),            # w 26, h 55: the square reaches x = 140
       (6, 6, 30, 30),
       (60, 10, 40, 20),             # inverted in x: squares to (45, 10, 55, 20)
       (36, 30, 66, 56),
       (90, 40, 90, 40),             # zero area
       (2, 70, 50, 90),              # w 48, h 20: the square reaches y = 104
       (70, 8, 98, 30),
       (76, 50, 116, 88),
       (8, 40, 30, 66)]
_F2 = [(100, 5, 126, 60), (2, 70, 50, 90), (0, 0, 10, 5)]
_F3 = [(10, 10, 40, 40), (60, 30, 100, 70)]
_F4 = [(4 + 18 * (i % 7), 4 + 26 * (i // 7), 20 + 18 * (i % 7), 20 + 26 * (i // 7)) for i in range(13)]
# name -> (detections, count, indices of the detections whose box gets a mask blob, rectangles zeroed in the mask afterwards)
_SPEC = dict(F0=(_F0, 5, (0, 1, 2, 3), [(54, 55, 84, 86)]), F1=(_F1, 9, (1, 3, 6, 7, 8), []), F2=(_F2, 3, (0, 1, 2), []),
             F3=(_F3, 2, (), []), F4=(_F4, 13, tuple(range(13)), []), F5=(_F0, 0, (0, 1, 2, 3), []), F6=(_F0, -3, (0, 1, 2, 3), []))
FRAME_NAMES = tuple(_SPEC)
# what the builder promises, per frame: boxes in frame, boxes with reliable depth among the first MAX_BOXES of them
PROMISED = dict(F0=(5, 4), F1=(7, 5), F2=(0, 0), F3=(2, 0), F4=(13, 12), F5=(0, 0), F6=(0, 0))


def _build_frame(name):
    boxes, count, blobs, holes = _SPEC[name]
    k = FRAME_NAMES.index(name)
    rng = np.random.default_rng(500 + k)
    rgb = rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8)
    mask = rng.integers(0, 101, (FH, FW)).astype(np.uint8)                  # background: never above 128
    yy, xx = np.mgrid[:FH, :FW]
    depth = (330 + 45 * k + xx // 4 + yy // 8 + rng.integers(0, 16, (FH, FW))).astype(np.uint16)
    for i in blobs:
        x0, y0, x1, y1 = boxes[i]
        mask[max(y0 - 6, 0):y1 + 6, max(x0 - 6, 0):x1 + 6] = 255
    for x0, y0, x1, y1 in holes:
        mask[y0:y1, x0:x1] = rng.integers(0, 101, (y1 - y0, x1 - x0)).astype(np.uint8)
    det = np.zeros((MAX_DET, 8), np.float32)
    det[:, :4] = (3, 3, 11, 11)                                              # rows behind the count: in frame, never to be read
    det[:len(boxes), :4] = np.array(boxes, np.float32) + np.float32(0.4)     # fractions: the int16 cast truncates
    det[:, 4] = rng.uniform(0.25, 1, MAX_DET)
    for a in (rgb, mask, depth, det):
        a.setflags(write=False)
    return Frame(name, rgb, mask, depth, det, count)


_FRAMES, _FRAME_REF = {}, {}


def frame(name):
    """built once per process; the arrays are read-only"""
    if name not in _FRAMES:
        _FRAMES[name] = _build_frame(name)
    return _FRAMES[name]


def frame_boxes_int16(fr):
    """the int16 boxes the host path receives (fast_pose_predictor.py:55-56) for the rows the detector reports"""
    n = min(max(fr.count, 0), MAX_DET)
    return fr.det[:n, :4].astype(np.int16)


def frame_reference(fr):
    """from the oracle alone -> (good [k, 4], sq [k, 4] of every in-frame box, eroded-valid pixel count [k], mean depth [k])"""
    if fr.name not in _FRAME_REF:
        good, sq = host_loop(frame_boxes_int16(fr), FH, FW)
        metres = fr.depth.astype(np.float32) / np.float32(DEPTH_DIV)
        cnt, mean = P.depth_stats64(good, metres, fr.mask, NEAR, FAR) if len(good) else (np.zeros(0, np.int64), np.zeros(0))
        _FRAME_REF[fr.name] = (good, sq, cnt, mean)
    return _FRAME_REF[fr.name]


def forwards(n, batch=ENGINE_BATCH):
    """sizes of the forwards a frame with n boxes runs on an engine of `batch` crops"""
    return [min(batch, n - off) for off in range(0, n, batch)]
