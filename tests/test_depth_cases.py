"""The CPU half of the depth statistics tests (GPU half: tests/test_gpu_depth_lift.py; cases and checker: tests/depth_cases.py).

1.  The strip plan (flope_amd/csrc/depth_plan.h through tests/host_harness/harness_depth.cpp): partition, tile, LDS limit, element,
    scratch layout.
2.  The reference: oracle.pipeline_ref.erode against scipy's independent binary erosion on every case mask, depth_stats64 against
    get_depth_value.
3.  The builder's promises, each taken from the plan harness and depth_stats64: both paths occur and are mixed inside one box, empty
    strips occur, the counts 0, 1, 49, 50, 51 occur, every probing hole is inside or outside the halo as intended, every case has
    a box with pixels, dropping any one strip is seen.
4.  A numpy emulation of the kernel's algorithm (strip by strip, validity tile with halo or per-tap fallback, double sums combined
    in strip order) passes the checker on every case; copies of it broken the way this kernel could break each fail it on at least
    one case (the idiom of tests/test_conv_bound.py).  A break that no case catches means a case is missing.
"""
import numpy as np
import pytest

import depth_cases as DC
from oracle import pipeline_ref as P


@pytest.fixture(scope="module")
def plan():
    return DC.load_plan()


# ---- 1. the plan -------------------------------------------------------------------------------------------------------------------------
def test_plan_constants_and_element(plan):
    assert plan.depth_strips() == 32 and plan.depth_lds() == 48 * 1024 and plan.depth_min_count() == DC.MIN_COUNT
    lo, hi, anchor = DC.ellipse_rows(plan)
    k = P.ellipse_kernel(10)
    assert anchor == 5 and plan.depth_taps() == int(k.sum()) == 83
    for ey in range(10):
        assert np.nonzero(k[ey])[0].tolist() == list(range(lo[ey], hi[ey] + 1)), ey


@pytest.mark.parametrize("bh", [0, 1, 5, 10, 31, 32, 33, 64, 100, 992, 1000, 1080])
def test_strips_partition_the_box_rows(plan, bh):
    p = DC.box_plan(plan, [3, 2, 3 + 40, 2 + bh], 2000, 2000)
    assert p.bh == bh and p.r0[0] == 0 and p.r1[-1] == bh
    assert (p.r1[:-1] == p.r0[1:]).all() and (p.r1 >= p.r0).all()
    nr = p.r1 - p.r0
    assert nr.max() - nr.min() <= 1 and ((nr == 0).any() == (bh < 32))
    assert (p.tile[:, 0] == p.ys + p.r0 - 5).all() and (p.tile[:, 1] == p.xs - 5).all()
    assert (p.tile[:, 2] == nr + 9).all() and (p.tile[:, 3] == p.bw + 9).all()
    assert (p.tiled == (nr > 0)).all()                   # 49 columns: every non-empty strip fits


def test_tile_limit_and_clamping(plan):
    # at bh = 1000 the strips have 31 or 32 rows: 40- and 41-row tiles; 48 KiB holds 1228 and 1198 columns of them
    for bw, want31, want32 in ((1189, True, True), (1190, True, False), (1219, True, False), (1220, False, False)):
        p = DC.box_plan(plan, [0, 0, bw, 1000], 1000, 1232)
        nr = p.r1 - p.r0
        assert set(nr) == {31, 32}
        assert (p.tiled[nr == 31] == want31).all() and (p.tiled[nr == 32] == want32).all(), bw
        assert (p.tiled == ((bw + 9) * (nr + 9) <= 48 * 1024)).all()
    # numpy slicing: far edges clamp, empty and inverted ranges select nothing
    H, W = 64, 80
    for box, want in (([48, 34, 83, 66], (48, 34, 80, 64, 32, 30)), ([20, 10, 20, 30], (20, 10, 20, 30, 0, 20)),
                      ([30, 10, 25, 30], (30, 10, 25, 30, 0, 20)), ([10, 30, 40, 22], (10, 30, 40, 22, 30, 0)),
                      ([80, 64, 85, 69], (80, 64, 80, 64, 0, 0))):
        p = DC.box_plan(plan, box, H, W)
        assert (p.xs, p.ys, p.xe, p.ye, p.bw, p.bh) == want
        a = np.zeros((H, W))[box[1]:box[3], box[0]:box[2]]
        assert a.shape == (p.bh, p.bw) or a.size == 0 == p.bw * p.bh
        assert not p.tiled.any() or p.bw * p.bh > 0


def test_scratch_layout(plan):
    """the partials begin 16-byte aligned behind H*W bytes and end inside the H*W + 16 + 512 n bytes include/flope_amd.h asks for"""
    for npix, n in ((37 * 53, 65), (16, 1), (17, 3), (1000 * 1232, 4), (1, 0)):
        b, e = plan.depth_partials_begin(npix), plan.depth_partials_end(npix, n)
        assert b % 16 == 0 and npix <= b < npix + 16 and e == b + 512 * n and e <= npix + 16 + 512 * n
    c = DC.case(plan, "odd")
    npix = c.mask.size
    assert c.mask.shape == (37, 53) and len(c.boxes) == 65 > 64                    # a second, ragged workgroup of the combine
    assert plan.depth_partials_begin(npix) == 1968 != npix                          # the rounded-up offset is in use
    assert npix + 16 + 512 * 65 - plan.depth_partials_end(npix, 65) == 9            # the partials sit at the end of the buffer


# ---- 2. the reference ----------------------------------------------------------------------------------------------------------------------
def _valid(c):
    d = DC.metres(c)
    return (d > np.float32(c.near)) & (d < np.float32(c.far)) & (c.mask > 128)


@pytest.mark.parametrize("name", DC.NAMES)
def test_oracle_erosion_equals_scipy(plan, name):
    from scipy.ndimage import binary_erosion
    m = _valid(DC.case(plan, name))
    ref = binary_erosion(m, structure=P.ellipse_kernel(10).astype(bool), border_value=1, origin=0)
    assert m.any() and not m.all() and np.array_equal(P.erode(m, 10), ref)


@pytest.mark.parametrize("name", DC.NAMES)
def test_depth_stats64_is_get_depth_value_made_visible(plan, name):
    c = DC.case(plan, name)
    count, mean = DC.reference(c)
    dv, rel = P.get_depth_value(c.boxes.tolist(), DC.metres(c), c.mask, near_plane=c.near, far_plane=c.far)
    assert rel.tolist() == (count >= DC.MIN_COUNT).tolist()
    assert (dv[count == 0] == 0).all() and (mean[count == 0] == 0).all()
    # the reference's own float32 mean (pairwise, <= ~log2(n) roundings) against fp64: for the record, and a loose sanity bound
    err = np.abs(dv - mean)[count > 0] / mean[count > 0]
    print(f"{name}: reference float32 np.mean vs fp64, worst relative difference {err.max():.3g} = {err.max() / DC.U23:.2f} x 2^-23")
    assert err.max() <= 32 * DC.U23


# ---- 3. the builder's promises -----------------------------------------------------------------------------------------------------------
def _plans(plan, c):
    H, W = c.mask.shape
    return [DC.box_plan(plan, b, H, W) for b in c.boxes.tolist()]


def test_both_paths_occur_and_mix_inside_one_box(plan):
    ps = _plans(plan, DC.case(plan, "big"))
    assert not ps[0].tiled.any()                                                  # [0,0,1232,1000]: untiled throughout
    for i in (1, 3):                                                                 # 1200 wide, 1000 high: mixed
        nr = ps[i].r1 - ps[i].r0
        assert ps[i].tiled[nr == 31].all() and not ps[i].tiled[nr == 32].any() and (nr == 31).any() and (nr == 32).any()
    assert ps[2].bh == 992 and ps[2].tiled.all()                                     # clamped to 31-row strips: tiled throughout
    for name in DC.NAMES[:-1]:                                                       # every small case is tiled wherever it has rows
        for p in _plans(plan, DC.case(plan, name)):
            assert (p.tiled == ((p.r1 - p.r0 > 0) & (p.bw > 0))).all()


def test_empty_strips_and_odd_heights_occur(plan):
    ps = _plans(plan, DC.case(plan, "seams"))
    assert sorted(p.bh for p in ps[:7]) == [1, 5, 31, 32, 33, 64, 100]
    assert [(p.bw, p.bh) for p in ps[7:]] == [(1, 70), (10, 10)]
    for p in ps:
        assert ((p.r1 - p.r0 == 0).any()) == (p.bh < 32)
    assert any(len(set(p.r1 - p.r0)) == 2 and p.bh > 32 for p in ps)                 # heights that are no multiple of 32


def test_threshold_counts_occur_exactly(plan):
    c = DC.case(plan, "thresholds")
    count, _ = DC.reference(c)
    assert count[:5].tolist() == [0, 1, 49, 50, 51]                                  # (w - 9) (h - 9) of the five rectangles
    assert count[7:].tolist() == [49, 49]                                            # 50 less the one survivor under a plane pixel
    d = DC.metres(c)
    for h in c.holes:
        y, x = h["y"], h["x"]
        if h["kind"] == "plane":
            assert d[y, x] == np.float32(c.near if h["at"] == "near" else c.far) and c.mask[y, x] > 128
        else:
            assert c.mask[y, x] == 128 and c.mask[y, x + 1] == 129 and c.near < d[y, x] < c.far
    # each of them changes the count of its box: without it the box would hold more pixels
    m = _valid(c)
    for h in c.holes:
        m2 = m.copy()
        m2[h["y"], h["x"]] = True
        assert P.erode(m2, 10).sum() > P.erode(m, 10).sum(), h


@pytest.mark.parametrize("name", ["seams", "seams_f32", "big"])
def test_probing_holes_lie_where_intended(plan, name):
    """row holes: offset >= -5 from boundary s <=> inside the tile of strip s; offset <= +3 <=> inside the tile of strip s - 1.
    column holes: xs - 5 .. xe + 3 inside, xs - 6 and xe + 4 outside."""
    c = DC.case(plan, name)
    ps = _plans(plan, c)
    d = DC.metres(c)
    seen_rows, seen_cols, kinds = set(), set(), set()
    for h in c.holes:
        y, x = h["y"], h["x"]
        bad = not (d[y, x] > np.float32(c.near) and d[y, x] < np.float32(c.far))
        assert (c.mask[y, x] == 128 and not bad) if h["how"] == "mask" else (bad and c.mask[y, x] == 255), h
        kinds.add((h["how"], "nan" if np.isnan(d[y, x]) else float(d[y, x]) if h["how"] == "depth" else 0))
        if h["kind"] == "row":
            p = ps[h["box"]]
            assert p.tile[0, 1] <= x < p.tile[0, 1] + p.tile[0, 3]
            for s, off in h["at"]:
                if s < 32:
                    assert y == p.ys + p.r0[s] + off
                    assert (p.tile[s, 0] <= y < p.tile[s, 0] + p.tile[s, 2]) == (off >= -5 and off < p.r1[s] - p.r0[s] + 4), h
                if s > 0:
                    assert y == p.ys + p.r1[s - 1] + off
                    t = p.tile[s - 1]
                    assert (t[0] <= y < t[0] + t[2]) == (off <= 3 and off >= -(p.r1[s - 1] - p.r0[s - 1]) - 5), h
                seen_rows.add(off)
        elif h["kind"] == "col":
            p = ps[h["box"]]
            edge, off = h["at"]
            assert x == (p.xs if edge == "xs" else p.xe) + off and p.ys <= y < p.ye
            assert (p.tile[0, 1] <= x < p.tile[0, 1] + p.tile[0, 3]) == ((edge, off) not in (("xs", -6), ("xe", 4))), h
            seen_cols.add((edge, off))
    assert seen_rows == set(DC.SEAM_ROWS) and seen_cols == set(DC.SIDE_COLS)
    assert {k[0] for k in kinds} == {"mask", "depth"}
    if name == "seams_f32":
        vals = {k[1] for k in kinds if k[0] == "depth"}
        assert {"nan", float("inf"), float("-inf"), 0.0} <= vals
    if name != "big":
        # every boundary of every seam box carries every offset that lies in the frame
        H = c.mask.shape[0]
        for bi in range(7):
            have = {(s, off) for h in c.holes if h["kind"] == "row" and h["box"] == bi for s, off in h["at"]}
            p = ps[bi]
            want = {(s, off) for s in range(33) for off in DC.SEAM_ROWS
                    if 0 <= p.ys + (p.r0[s] if s < 32 else p.r1[31]) + off < H}
            assert have == want and len(want) == 33 * 8


def test_outermost_tile_rows_and_columns_matter_alone(plan):
    """the holes in the first and last tile row / column of a whole box (ys - 5, ye + 3, xs - 5, xe + 3) are shadowed by no other
    hole: filling one alone raises the box's count; the holes one step further out (ys - 6, ye + 4, xs - 6, xe + 4) change nothing"""
    c = DC.case(plan, "seams")
    m = _valid(c)
    base = P.erode(m, 10)
    tried = set()
    for h in c.holes:
        if h["kind"] == "row":
            keys = [("row", s, off) for s, off in h["at"] if (s, off) in ((0, -5), (0, -6), (32, 3), (32, 4))]
        elif h["kind"] == "col":
            keys = [("col",) + h["at"]] if h["at"] in (("xs", -5), ("xs", -6), ("xe", 3), ("xe", 4)) else []
        else:
            keys = []
        x0, y0, x1, y1 = c.boxes[h["box"]].tolist()
        if not keys or h["box"] == 7 or (h["kind"] == "col" and y1 - y0 < 31):
            continue                             # the one-pixel-wide box and the side holes of low boxes share their victims
        m2 = m.copy()
        m2[h["y"], h["x"]] = True
        gain = int(P.erode(m2, 10)[y0:y1, x0:x1].sum()) - int(base[y0:y1, x0:x1].sum())
        inside = keys[0][2] in (-5, 3)
        assert (gain >= 1) == inside, (h, gain)
        tried.add((h["box"], keys[0]))
    for bi in range(7):
        keys = [("row", 0, -5), ("row", 0, -6), ("row", 32, 3), ("row", 32, 4)]
        if c.boxes[bi, 3] - c.boxes[bi, 1] >= 31:
            keys += [("col", "xs", -5), ("col", "xs", -6), ("col", "xe", 3), ("col", "xe", 4)]
        for key in keys:
            assert (bi, key) in tried, (bi, key)


def test_border_case_reaches_every_edge(plan):
    c = DC.case(plan, "border")
    H, W = c.mask.shape
    b = c.boxes
    assert (b[:, 0] == 0).any() and (b[:, 1] == 0).any() and (b[:, 2] == W).any() and (b[:, 3] == H).any()
    for corner in ((0, 0), (W, 0), (0, H), (W, H)):
        assert any((bx[0] == corner[0] or bx[2] == corner[0]) and (bx[1] == corner[1] or bx[3] == corner[1]) for bx in b.tolist())
    assert ((b[:, 2] > W) & (b[:, 3] > H) & (b[:, 0] < W) & (b[:, 1] < H)).any()
    assert (b[:, 2] == b[:, 0]).any() and (b[:, 2] < b[:, 0]).any()
    assert {h["at"] for h in c.holes} == {(e, d) for e in ("top", "bottom", "left", "right") for d in range(6)}
    for h in c.holes:
        e, d = h["at"]
        assert {"top": h["y"], "bottom": H - 1 - h["y"], "left": h["x"], "right": W - 1 - h["x"]}[e] == d
    count, _ = DC.reference(c)
    ps = _plans(plan, c)
    assert all((cnt == 0) for cnt, p in zip(count, ps) if p.bw * p.bh == 0) and sum(p.bw * p.bh == 0 for p in ps) >= 5


def test_high_half_case(plan):
    c = DC.case(plan, "high16")
    assert c.depth.dtype == np.uint16 and c.depth_div == 20000.0
    d = DC.metres(c)
    assert d[c.depth > 0].min() >= 1.5 and d.max() <= 1.8 and (c.depth == 0).sum() == 2
    for x0, y0, x1, y1 in c.boxes.tolist():
        sub = c.depth[y0:y1, x0:x1]
        assert (sub >= 32768).any()
    assert any((c.depth[y0:y1, x0:x1] < 32768).any() for x0, y0, x1, y1 in c.boxes.tolist())


@pytest.mark.parametrize("name", DC.NAMES)
def test_every_case_has_pixels_and_depth_varies(plan, name):
    c = DC.case(plan, name)
    count, mean = DC.reference(c)
    assert (count > 0).any() and np.isfinite(mean).all()
    assert len(np.unique(c.depth[np.isfinite(c.depth.astype(np.float64))])) > 200
    assert c.mask.size <= 1_300_000


# ---- 4. the emulation and its broken copies ------------------------------------------------------------------------------------------------
class Emu:
    """The kernel's algorithm in numpy.  `brk` names one deliberate defect; None is the kernel as written."""

    def __init__(self, lib, brk=None):
        self.lib, self.brk = lib, brk
        lo, hi, self.anchor = DC.ellipse_rows(lib)
        self.taps = [(ey, ex) for ey in range(10) for ex in range(lo[ey], hi[ey] + 1)]
        self.taps_untiled = list(self.taps)
        if brk == "untiled_table_row":                      # the __constant__ tables disagree with the unrolled ones in one row
            self.taps_untiled = [(ey, ex) for ey, ex in self.taps if not (ey == 8 and ex in (1, 9))]
        if brk == "tiled_table_row":
            self.taps = [(ey, ex) for ey, ex in self.taps if not (ey == 1 and ex in (2, 8))]

    def metres(self, c):
        raw = c.depth
        if raw.dtype == np.uint16 and self.brk == "sign_extend":
            raw = raw.view(np.int16)
        return raw.astype(np.float32) / np.float32(c.depth_div)

    def valid_map(self, c):
        d = self.metres(c)
        near, far = np.float32(c.near), np.float32(c.far)
        a = (d >= near) if self.brk == "near_ge" else (d > near)
        b = (d <= far) if self.brk == "far_le" else (d < far)
        m = (c.mask >= 128) if self.brk == "mask_ge" else (c.mask > 128)
        return a & b & m

    def fetch(self, v, y0, x0, h, w):
        """validity of the frame rectangle rows y0 .. y0+h-1, columns x0 .. x0+w-1; out-of-frame reads as valid"""
        H, W = v.shape
        out = np.full((h, w), self.brk != "border_invalid", bool)
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
        if ya < yb and xa < xb:
            out[ya - y0:yb - y0, xa - x0:xb - x0] = v[ya:yb, xa:xb]
        return out

    def partials(self, c):
        """-> (double sums [n, 32], counts [n, 32])"""
        H, W = c.mask.shape
        v = self.valid_map(c)
        mm = self.metres(c) * np.float32(1000)
        n = len(c.boxes)
        sums, cnts = np.zeros((n, 32)), np.zeros((n, 32), np.int64)
        A = self.anchor
        for b, box in enumerate(c.boxes.tolist()):
            p = DC.box_plan(self.lib, box, H, W)
            for s in range(32):
                r0, r1 = int(p.r0[s]), int(p.r1[s])
                if self.brk == "r1_plus" and r1 < p.bh:
                    r1 += 1
                if self.brk == "r1_minus" and r1 > r0:
                    r1 -= 1
                nr, bw = r1 - r0, p.bw
                if nr <= 0 or bw <= 0:
                    continue
                ok = np.ones((nr, bw), bool)
                if p.tiled[s]:
                    hl = 4 if self.brk == "halo4" else A                  # halo4: one row / column less on every side
                    hh = 3 if self.brk == "halo4" else 9 - A
                    tile = np.ones((nr + 9, bw + 9), bool)                # what the taps index; outside the built part: "valid"
                    built = self.fetch(v, p.ys + r0 - hl, p.xs - hl, nr + hl + hh, bw + hl + hh)
                    tile[A - hl:A - hl + built.shape[0], A - hl:A - hl + built.shape[1]] = built
                    for ey, ex in self.taps:
                        ok &= tile[ey:ey + nr, ex:ex + bw]
                else:
                    for ey, ex in self.taps_untiled:
                        ok &= self.fetch(v, p.ys + r0 + ey - A, p.xs + ex - A, nr, bw)
                g = mm[p.ys + r0:p.ys + r1, p.xs:p.xs + bw][ok]
                sums[b, s], cnts[b, s] = g.astype(np.float64).sum(), g.size
        return sums, cnts

    def finish(self, c, sums, cnts, drop=None):
        n = len(c.boxes)
        dv, xyz, rel = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, bool)
        fx, fy, cx, cy = [float(np.float32(k)) for k in c.K4]
        last = 31 if self.brk == "last_strip" else 32
        for b in range(n):
            s, cnt = 0.0, 0
            for k in range(last):
                if k != drop:
                    s += float(sums[b, k])
                    cnt += int(cnts[b, k])
            den = cnt + 1 if self.brk == "count_plus_1" else cnt
            d = (s / den) / 1000.0 if cnt > 0 else 0.0
            dv[b] = np.float32(d)
            rel[b] = {"rel_gt": cnt > 50, "rel_49": cnt >= 49}.get(self.brk, cnt >= 50)
            x0, y0, x1, y1 = c.boxes[b].tolist()
            xn, yn = ((x0 + x1) * 0.5 - cx) / fx, ((y0 + y1) * 0.5 - cy) / fy
            z = d / np.sqrt(xn * xn + yn * yn + 1.0)
            xyz[b] = np.float32(xn * z), np.float32(yn * z), np.float32(z)
        return dv, rel, xyz

    def run(self, c):
        return self.finish(c, *self.partials(c))


_PARTIALS = {}


def _good_partials(plan, name):
    if name not in _PARTIALS:
        _PARTIALS[name] = Emu(plan).partials(DC.case(plan, name))
    return _PARTIALS[name]


@pytest.mark.parametrize("name", DC.NAMES)
def test_unbroken_emulation_passes(plan, name):
    c = DC.case(plan, name)
    e = Emu(plan)
    sums, cnts = _good_partials(plan, name)
    count, _ = DC.reference(c)
    assert cnts.sum(axis=1).tolist() == count.tolist()                    # the strips add up to the reference's count
    fails, r_dv, r_xyz = DC.check(c, *e.finish(c, sums, cnts))
    print(f"{name}: emulation worst |err| / bound: depth_val {r_dv:.3f}, xyz {r_xyz:.3f}")
    assert not fails, fails[:5]


BREAKS = ["halo4", "r1_plus", "r1_minus", "border_invalid", "near_ge", "far_le", "mask_ge", "rel_gt", "rel_49", "sign_extend",
          "last_strip", "untiled_table_row", "tiled_table_row", "count_plus_1"]


@pytest.mark.parametrize("brk", BREAKS)
def test_broken_emulation_is_caught(plan, brk):
    caught = {}
    for name in DC.NAMES:
        c = DC.case(plan, name)
        fails, _, _ = DC.check(c, *Emu(plan, brk).run(c))
        if fails:
            caught[name] = len(fails)
        if caught and name in ("odd", "high16"):                          # the large frame only where the small ones saw nothing
            break
    print(f"{brk}: caught by {caught}")
    assert caught, f"no case notices the break {brk!r}: a case is missing"


@pytest.mark.parametrize("name", ["seams", "border", "big"])
def test_dropping_any_one_strip_is_seen(plan, name):
    """every strip index carries, in some box of the case, enough of the mean to move it past the bound"""
    c = DC.case(plan, name)
    e = Emu(plan)
    sums, cnts = _good_partials(plan, name)
    for s in range(32):
        fails, _, _ = DC.check(c, *e.finish(c, sums, cnts, drop=s))
        assert fails, (name, s)


def test_what_each_break_needs(plan):
    """the cases are not interchangeable: the breaks that live on one path or one format are caught by the case built for them"""
    for brk, name in (("untiled_table_row", "big"), ("sign_extend", "high16"), ("border_invalid", "border"), ("halo4", "seams"),
                      ("halo4", "seams_f32"), ("rel_gt", "thresholds"), ("rel_49", "thresholds"), ("near_ge", "thresholds"),
                      ("far_le", "thresholds"), ("mask_ge", "thresholds"), ("last_strip", "odd")):
        c = DC.case(plan, name)
        fails, _, _ = DC.check(c, *Emu(plan, brk).run(c))
        assert fails, (brk, name)
    # and the reliable flag itself flips under each comparison break, not only the mean
    c = DC.case(plan, "thresholds")
    for brk in ("near_ge", "far_le", "rel_gt", "rel_49"):
        fails, _, _ = DC.check(c, *Emu(plan, brk).run(c))
        assert any("reliable" in f for f in fails), brk
