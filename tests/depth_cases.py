"""Edge cases of the depth statistics kernel (flope_amd/csrc/prep.hip: depth_box_kernel / depth_box_final_kernel, flope_depth_lift)
and the checker both halves of its tests share: tests/test_depth_cases.py (CPU: the builder's promises, an emulation of the kernel
and its broken copies) and tests/test_gpu_depth_lift.py (the kernel itself).

The kernel's count of eroded-valid pixels cannot be read from outside, only `reliable = count >= 50` and the mean.  So every frame
has a depth that varies per pixel (ramp + seeded noise: a dropped or doubled pixel moves the mean), and the holes that probe the
strip seams and the tile's halo are single pixels placed from the kernel's own strip plan (flope_amd/csrc/depth_plan.h through
tests/host_harness/harness_depth.cpp), never from a Python copy of it.

A case is (name, depth, mask, boxes, depth_div, near, far, K4) + the list of probing holes the builder placed.
  depth   uint16 raw [H, W] (metres = raw / depth_div) or float32 metres [H, W] (depth_div = 1)
  mask    uint8 [H, W], boxes int32 [N, 4] = x0, y0, x1, y1, K4 = fx, fy, cx, cy (exact in float32)
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pipeline_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U23 = 2.0 ** -23              # the bound of both outputs: twice the one float32 rounding each of them takes
MIN_COUNT = 50                # image_manipulation.py: reliable = at least 50 eroded-valid pixels

Case = collections.namedtuple("Case", "name depth mask boxes depth_div near far K4 holes")

# rows probed around every strip boundary ys + r0: -5 is the first row of the strip's tile, -6 the row above it; +3 is the last row
# of the previous strip's tile (its r1 is this r0), +4 and +5 lie below it
SEAM_ROWS = (-6, -5, -4, -1, 0, 3, 4, 5)
# columns probed, relative to xs (first four) and xe (last four): the tile spans xs - 5 .. xe + 3
SIDE_COLS = (("xs", -6), ("xs", -5), ("xs", -1), ("xs", 0), ("xe", -1), ("xe", 0), ("xe", 3), ("xe", 4))


# ---- the strip plan, from the header the kernel includes -----------------------------------------------------------------------------
def load_plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_depth.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_depth.so"])
    lib = C.CDLL(path)
    lib.depth_partials_begin.restype = C.c_long
    lib.depth_partials_begin.argtypes = [C.c_long]
    lib.depth_partials_end.restype = C.c_long
    lib.depth_partials_end.argtypes = [C.c_long, C.c_long]
    return lib


Plan = collections.namedtuple("Plan", "xs ys xe ye bw bh r0 r1 tiled tile")


def box_plan(lib, box, H, W):
    """the kernel's plan of one box: clamped extents, per strip rows [r0, r1) relative to ys, tiled flag, tile rectangle
    (first row, first column, rows, columns) in frame coordinates"""
    S = lib.depth_strips()
    b = (C.c_int * 4)(*[int(v) for v in box])
    ext = (C.c_int * 6)()
    lib.depth_extent(b, H, W, ext)
    r0, r1, tiled, tile = (C.c_int * S)(), (C.c_int * S)(), (C.c_int * S)(), (C.c_int * (4 * S))()
    lib.depth_plan(b, H, W, r0, r1, tiled, tile)
    return Plan(*list(ext), np.array(r0[:]), np.array(r1[:]), np.array(tiled[:]).astype(bool), np.array(tile[:]).reshape(S, 4))


def ellipse_rows(lib):
    lo, hi = (C.c_int * 10)(), (C.c_int * 10)()
    anchor = lib.depth_ellipse(lo, hi)
    return list(lo), list(hi), anchor


# ---- frames ------------------------------------------------------------------------------------------------------------------------------
def _ramp(H, W, base, ax, ay_num, ay_den, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    return (base + ax * xx + (ay_num * yy) // ay_den + rng.integers(0, 64, (H, W))).astype(np.uint16)


def _k4(H, W):
    return (600.5, 599.25, W / 2 + 0.25, H / 2 - 0.25)     # exact in float32; no box centre (multiples of 0.5) meets cx or cy


def _punch(depth, mask, holes, y, x, k, **rec):
    """one single-pixel hole in a frame whose mask is 255, by mask (128) when k is even, by depth (0) when odd; out-of-frame
    positions are skipped"""
    H, W = mask.shape
    if not (0 <= y < H and 0 <= x < W) or mask[y, x] != 255 or depth[y, x] == 0:      # a pixel is punched once, one way
        return
    how = "mask" if k % 2 == 0 else "depth"
    if how == "mask":
        mask[y, x] = 128
    else:
        depth[y, x] = 0
    holes.append(dict(rec, y=int(y), x=int(x), how=how))


def _seam_holes(lib, depth, mask, holes, bi, box, col0, stride, slots, which=None):
    """one hole in every frame row that lies at an offset of SEAM_ROWS from a strip boundary of the box; consecutive rows take
    columns `stride` apart, so that the pixel a hole should kill (or spare) is not killed by the holes of the rows around it"""
    H, W = mask.shape
    p = box_plan(lib, box, H, W)
    S = len(p.r0)
    rows = {}
    for s in range(S + 1) if which is None else which:
        boundary = p.ys + (p.r0[s] if s < S else p.r1[S - 1])
        for off in SEAM_ROWS:
            rows.setdefault(int(boundary + off), []).append((s, off))
    for k, y in enumerate(sorted(rows)):
        _punch(depth, mask, holes, y, p.xs + col0 + stride * (k % slots), k, box=bi, kind="row", at=rows[y])


def _side_holes(lib, depth, mask, holes, bi, box):
    """holes at the SIDE_COLS of the box, each pair of sides on its own row"""
    H, W = mask.shape
    p = box_plan(lib, box, H, W)
    for k, (edge, off) in enumerate(SIDE_COLS):
        y = p.ys + (p.bh * (2 * (k % 4) + 1)) // 8
        _punch(depth, mask, holes, y, (p.xs if edge == "xs" else p.xe) + off, k + k // 4, box=bi, kind="col", at=(edge, off))


def _seams(lib):
    """boxes of height 1, 5, 31, 32, 33, 64, 100 (110 wide, two columns), a one-pixel-wide box between the columns and a 10 x 10 box"""
    H, W = 208, 252
    depth, mask, holes = _ramp(H, W, 400, 3, 2, 1, 31), np.full((H, W), 255, np.uint8), []
    boxes = [[8, 8, 118, 108], [8, 122, 118, 155], [8, 170, 118, 171],                            # heights 100, 33, 1
             [134, 8, 244, 72], [134, 86, 244, 118], [134, 132, 244, 163], [134, 178, 244, 183],  # heights 64, 32, 31, 5
             [126, 20, 127, 90], [20, 192, 30, 202]]                                              # bw = 1; 10 x 10
    for bi, box in enumerate(boxes[:7]):
        _seam_holes(lib, depth, mask, holes, bi, box, 10, 10, 10)
        _side_holes(lib, depth, mask, holes, bi, box)
    _seam_holes(lib, depth, mask, holes, 7, boxes[7], 0, 0, 1, which=(0, 16, 32))
    _side_holes(lib, depth, mask, holes, 7, boxes[7])
    # the 10 x 10 box: one hole in the first tile row (kills exactly one pixel), one above it and two below the last tile row
    x0, y0, x1, y1 = boxes[8]
    for k, (y, x, at) in enumerate([(y0 - 5, x0 + 7, (0, -5)), (y0 - 6, x0 + 3, (0, -6)), (y1 + 4, x0 + 2, (32, 4)), (y1 + 5, x0 + 6, (32, 5))]):
        _punch(depth, mask, holes, y, x, k, box=8, kind="row", at=[at])
    return Case("seams", depth, mask, np.array(boxes, np.int32), 1000.0, 0.1, 2.5, _k4(H, W), holes)


def _seams_f32(lib):
    """the seam frame as float32 metres: the depth holes become NaN, +inf, -inf and 0 in turn"""
    c = _seams(lib)
    d = c.depth.astype(np.float32) / np.float32(1000)
    bad = [np.nan, np.inf, -np.inf, 0.0]
    k = 0
    for h in c.holes:
        if h["how"] == "depth":
            d[h["y"], h["x"]] = bad[k % 4]
            k += 1
    assert k >= 4
    return c._replace(name="seams_f32", depth=d, depth_div=1.0)


def _border(lib):
    """boxes flush with every edge and corner of the frame, holes 0..5 pixels from each edge, a box past the far corner (numpy
    slicing clamps it) and empty boxes"""
    H, W = 64, 80
    depth, mask, holes = _ramp(H, W, 500, 7, 5, 1, 32), np.full((H, W), 255, np.uint8), []
    for d in range(6):
        _punch(depth, mask, holes, d, 6 + 13 * d, d, kind="edge", at=("top", d))
        _punch(depth, mask, holes, H - 1 - d, 9 + 13 * d, d + 1, kind="edge", at=("bottom", d))
        _punch(depth, mask, holes, 12 + 9 * d, d, d, kind="edge", at=("left", d))
        _punch(depth, mask, holes, 8 + 9 * d, W - 1 - d, d + 1, kind="edge", at=("right", d))
    boxes = [[0, 0, 30, 24], [50, 0, W, 24], [0, 40, 30, H], [50, 40, W, H],            # the four corners
             [30, 0, 50, 20], [30, 44, 50, H], [0, 24, 20, 40], [60, 24, W, 40],        # the four edges
             [0, 0, W, H],                                                              # the whole frame
             [48, 34, W + 3, H + 2],                                                    # past the far corner: clamped
             [20, 10, 20, 30], [30, 10, 25, 30], [10, 30, 40, 30], [10, 30, 40, 22],    # empty: x1 == x0, x1 < x0, y1 == y0, y1 < y0
             [W, H, W + 5, H + 5]]                                                      # wholly outside
    return Case("border", depth, mask, np.array(boxes, np.int32), 1000.0, 0.1, 2.5, _k4(H, W), holes)


def _thresholds(lib):
    """valid rectangles on an invalid background whose eroded counts are exactly 0, 1, 49, 50, 51 ((w - 9) (h - 9) each); pixels
    exactly on the near and the far plane, and a mask of 129 with one 128 in it"""
    H, W = 96, 160
    depth, mask, holes = _ramp(H, W, 300, 5, 3, 1, 33), np.zeros((H, W), np.uint8), []
    boxes, x = [], 6
    for w, h in ((9, 14), (10, 10), (16, 16), (19, 14), (26, 12)):
        mask[6:6 + h, x:x + w] = 255
        boxes.append([x - 3, 3, x + w + 3, 6 + h + 3])
        x += w + 12
    # raw 100 and 2500 at div 1000: exactly near = 0.1 and far = 2.5, invalid; each punches a hole off the rectangle's centre
    mask[40:80, 8:56] = 255
    depth[50, 20], depth[66, 41] = 100, 2500
    holes += [dict(kind="plane", at="near", y=50, x=20, how="depth"), dict(kind="plane", at="far", y=66, x=41, how="depth")]
    boxes.append([4, 36, 60, 84])
    # 129 is valid, 128 is not
    mask[40:80, 70:118] = 129
    mask[52, 83] = 128
    holes.append(dict(kind="mask128", at="129|128", y=52, x=83, how="mask"))
    boxes.append([66, 36, 122, 84])
    # both planes at the threshold of `reliable`: 19 x 14 rectangles (50 pixels) with a pixel of the top row exactly on a plane; it
    # is the topmost tap of one survivor only -> 49
    for y0, raw, at in ((40, 2500, "far"), (64, 100, "near")):
        mask[y0:y0 + 14, 130:149] = 255
        depth[y0, 135] = raw
        holes.append(dict(kind="plane", at=at, y=y0, x=135, how="depth"))
        boxes.append([126, y0 - 4, 153, y0 + 18])
    return Case("thresholds", depth, mask, np.array(boxes, np.int32), 1000.0, 0.1, 2.5, _k4(H, W), holes)


def _high16(lib):
    """raw values 30000 .. 36000 at depth_div 20000 (1.5 .. 1.8 m): the upper half of uint16, negative if read as int16"""
    H, W = 48, 64
    depth, mask, holes = (_ramp(H, W, 30000, 70, 30, 1, 34)), np.full((H, W), 255, np.uint8), []
    assert depth.min() >= 30000 and depth.max() <= 36000 and (depth < 32768).any() and (depth >= 32768).any()
    for k, (y, x) in enumerate([(9, 12), (20, 41), (33, 27), (40, 55)]):
        _punch(depth, mask, holes, y, x, k, kind="plain", at=None)
    boxes = [[4, 4, 60, 44], [30, 10, 52, 34], [6, 8, 30, 40], [44, 6, 62, 42]]
    return Case("high16", depth, mask, np.array(boxes, np.int32), 20000.0, 0.1, 2.5, _k4(H, W), holes)


def _odd(lib):
    """a 37 x 53 frame (1961 pixels: the partials start at the rounded-up offset 1968) with 65 boxes, one more than a workgroup of
    the combining kernel takes; include/flope_amd.h's scratch formula H*W + 16 + 512 n leaves 9 bytes behind the last partial"""
    H, W = 37, 53
    rng = np.random.default_rng(35)
    depth, mask = _ramp(H, W, 300, 7, 5, 1, 35), np.full((H, W), 255, np.uint8)
    mask[rng.random((H, W)) < 1 / 80] = 128
    boxes = []
    for _ in range(63):
        x0, y0 = int(rng.integers(0, W - 1)), int(rng.integers(0, H - 1))
        boxes.append([x0, y0, x0 + int(rng.integers(1, W)), y0 + int(rng.integers(1, H))])
    boxes += [[3, 2, 50, 35], [0, 0, W, H]]
    return Case("odd", depth, mask, np.array(boxes, np.int32), 1000.0, 0.1, 2.5, _k4(H, W), [])


def _big(lib):
    """1000 x 1232: strips too wide for the LDS tile.  [0,0,1232,1000] is untiled throughout; [0,0,1200,1000] has its 31-row strips
    tiled and its 32-row strips untiled; the same box moved to the right edge; [16,8,1216,1008] clamps to 992 rows"""
    H, W = 1000, 1232
    rng = np.random.default_rng(36)
    yy, xx = np.mgrid[:H, :W]
    depth = (300 + xx + yy // 2 + rng.integers(0, 64, (H, W))).astype(np.uint16)
    mask, holes = np.full((H, W), 255, np.uint8), []
    boxes = [[0, 0, 1232, 1000], [0, 0, 1200, 1000], [16, 8, 1216, 1008], [32, 0, 1232, 1000]]
    _seam_holes(lib, depth, mask, holes, 0, boxes[0], 40, 37, 30)
    _seam_holes(lib, depth, mask, holes, 2, boxes[2], 50, 37, 30)
    for bi in (1, 2):
        _side_holes(lib, depth, mask, holes, bi, boxes[bi])
    ys, xs = rng.integers(0, H, 600), rng.integers(0, W, 600)
    for k in range(600):
        _punch(depth, mask, holes, int(ys[k]), int(xs[k]), k, kind="plain", at=None)
    return Case("big", depth, mask, np.array(boxes, np.int32), 1000.0, 0.1, 2.5, _k4(H, W), holes)


BUILDERS = dict(seams=_seams, seams_f32=_seams_f32, border=_border, thresholds=_thresholds, high16=_high16, odd=_odd, big=_big)
NAMES = tuple(BUILDERS)
_CASES, _REF = {}, {}


def case(lib, name):
    """built once per process; treat the arrays as read-only"""
    if name not in _CASES:
        c = BUILDERS[name](lib)
        for a in (c.depth, c.mask, c.boxes):
            a.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


# ---- the reference and the checker ---------------------------------------------------------------------------------------------------------
def metres(c):
    """float32 metres as the reference's caller forms them (fast_pose_predictor.py:90: depth.astype(float32) / div)"""
    return c.depth.astype(np.float32) / np.float32(c.depth_div)


def reference(c):
    """(count, mean64) of every box by oracle.pipeline_ref.depth_stats64, computed once per case"""
    if c.name not in _REF:
        _REF[c.name] = P.depth_stats64(c.boxes, metres(c), c.mask, c.near, c.far)
    return _REF[c.name]


def points_ref(c, mean64):
    """get_points3d in float64 from the fp64 means, intrinsics as the float32 values the C ABI carries"""
    fx, fy, cx, cy = [float(np.float32(v)) for v in c.K4]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    b = c.boxes.astype(np.float64)
    uv = np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2], 1)
    return P.get_points3d(uv, mean64, K)


def check(c, dv, rel, xyz):
    """outputs of one depth_lift call against the fp64 reference -> (list of failures, worst |err| / bound of depth_val, of xyz)
      reliable   == (count >= 50) on every row
      depth_val  |dv - mean64| <= 2^-23 mean64; exactly 0 where count == 0
      xyz        |xyz - get_points3d(mean64)| <= 2^-23 |component| on every row; exactly 0 where count == 0"""
    count, mean = reference(c)
    dv = np.asarray(dv).astype(np.float64)
    rel = np.asarray(rel).astype(bool)
    xyz = np.asarray(xyz).astype(np.float64)
    n = len(count)
    fails = []
    if dv.shape != (n,) or rel.shape != (n,) or xyz.shape != (n, 3):
        return [f"{c.name}: shapes {dv.shape} {rel.shape} {xyz.shape} for {n} boxes"], np.inf, np.inf
    want = count >= MIN_COUNT
    for i in np.nonzero(rel != want)[0]:
        fails.append(f"{c.name} box {i}: reliable {rel[i]} with count {count[i]}")
    pos = count > 0
    for i in np.nonzero(~pos)[0]:
        if dv[i] != 0 or (xyz[i] != 0).any():
            fails.append(f"{c.name} box {i}: count 0 but depth_val {dv[i]!r} xyz {xyz[i]}")
    pref = points_ref(c, mean)
    with np.errstate(invalid="ignore", divide="ignore"):
        r_dv = np.where(pos, np.abs(dv - mean) / (U23 * mean), 0.0)
        r_xyz = np.where(pos[:, None], np.abs(xyz - pref) / (U23 * np.abs(pref)), 0.0)
    r_dv[~np.isfinite(r_dv)] = np.inf
    r_xyz[~np.isfinite(r_xyz)] = np.inf
    for i in np.nonzero(r_dv > 1)[0]:
        fails.append(f"{c.name} box {i}: depth_val {dv[i]!r} vs {mean[i]!r} (count {count[i]}), |err| / bound = {r_dv[i]:.3g}")
    for i in np.nonzero((r_xyz > 1).any(axis=1))[0]:
        fails.append(f"{c.name} box {i}: xyz {xyz[i]} vs {pref[i]}, |err| / bound = {r_xyz[i].max():.3g}")
    return fails, float(r_dv.max(initial=0.0)), float(r_xyz.max(initial=0.0))
