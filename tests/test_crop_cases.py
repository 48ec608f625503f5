"""The CPU half of the crop + Lanczos-4 resize tests (GPU half: tests/test_gpu_crop_cases.py; cases and checker: tests/crop_cases.py).

1.  The tile plan (flope_amd/csrc/crop_plan.h through tests/host_harness/harness_crop.cpp) and the first-tap formula the path model
    is fed with.
2.  The builder's promises, each taken from the plan harness and the oracle: windows of exactly 64 and 65 rows occur, one crop has
    tiles on both paths, a ragged last tile takes another path than its existing rows alone would give it, every border box
    touches what it claims, every narrow axis clamps every tap, the identity frame holds all 65 536 (img, m) pairs, the
    accumulator case reaches 0.95 * 2^31 and no fraction t = k / 65536 can pass 2^31.
3.  A numpy emulation of the kernel's algorithm (tile by tile; an int32 window of kCropRows rows on the separable path, the direct
    8 x 8 sum otherwise; int32 throughout, then fin and masked_unit, then the store into the flat buffer of each format) passes the
    checker on every case; copies of it broken the way this kernel could break are each noticed on at least one case (the idiom
    of tests/test_conv_bound.py).  A break that no case notices means a case is missing.

    Two of the breaks move no output bit, BECAUSE the two paths add the same integers: the limit tested as R < 64, and R taken from
    the last existing row of a ragged tile.  They only move tiles from one path to the other.  The emulation therefore also
    reports the path of every tile, and a run is noticed when its bits OR its path map differ from crop_plan.h's; for those two
    that states that tiles of exactly 64 rows and a ragged tile flipped by its phantom row are among the cases.

    "r0 from the tile's first live row": the first output row of every tile exists (there are ceil(S / 16) tile rows), so the break
    is read as the window starting at the first source row that exists in the crop (max(r0, 0)) while rb still counts from the
    unclamped r0.
"""
import numpy as np
import pytest

import crop_cases as CC
from oracle import pipeline_ref as P


@pytest.fixture(scope="module")
def plan():
    return CC.load_plan()


# ---- 1. the plan -------------------------------------------------------------------------------------------------------------------------
def test_plan_constants_and_rule(plan):
    assert plan.crop_tile() == 16 and plan.crop_rows_limit() == 64 and plan.crop_taps() == 8 and plan.crop_taps_back() == 3
    assert [plan.crop_tile_count(S) for S in (1, 15, 16, 17, 100, 256)] == [1, 1, 1, 2, 7, 16]
    for s0, s15 in ((-1, 2), (0, 56), (0, 57), (10, 10), (300, 357)):
        assert plan.crop_first_row(s0) == s0 - 3
        assert plan.crop_rows(s0, s15) == (s15 + 4) - (s0 - 3) + 1              # taps s0 - 3 .. s15 + 4, both ends included
    assert [plan.crop_separable(R) for R in (1, 63, 64, 65, 66, 400)] == [1, 1, 1, 0, 0, 0]


@pytest.mark.parametrize("n_src,S", [(60, 16), (91, 24), (7, 78), (301, 100), (1, 40), (40, 40)])
def test_first_taps_are_the_oracles_and_phantoms_continue_them(plan, n_src, S):
    """for d < S the positions and weights are _axis_table_raw's; for d >= S the same formula goes on (monotone, same scale)"""
    count = plan.crop_tile_count(S) * plan.crop_tile()
    s, wt, raw = CC.axis(n_src, S, count)
    _, wt_o, s_o = P._axis_table_raw(n_src, S)
    assert np.array_equal(s[:S], s_o) and np.array_equal(wt[:S], wt_o)
    assert (np.diff(s) >= 0).all()
    scale = n_src / S
    assert (np.abs(s - np.floor((np.arange(count) + 0.5) * scale - 0.5)) <= 1).all()


def test_issue_row_counts(plan):
    """the tile row counts the cases were chosen by"""
    assert CC.tile_rows(plan, 60, 16) == [64] and CC.tile_rows(plan, 61, 16) == [65]
    assert CC.tile_rows(plan, 90, 24) == [64, 64] and CC.tile_rows(plan, 91, 24) == [65, 64] and CC.tile_rows(plan, 92, 24) == [65, 66]
    assert CC.tile_rows(plan, 148, 40) == [63, 64, 64]
    assert set(CC.tile_rows(plan, 370, 100)) == {63, 64} and set(CC.tile_rows(plan, 380, 100)) == {65}


# ---- 2. the builder's promises -----------------------------------------------------------------------------------------------------------
def _all_rows(plan):
    rows = {}
    for name in CC.NAMES:
        c = CC.case(plan, name)
        for b, p in enumerate(CC.tile_paths(plan, c)):
            if p is not None:
                rows[(name, b)] = [R for R, _ in p]
    return rows


def test_both_sides_of_the_limit_and_mixed_paths_occur(plan):
    rows = _all_rows(plan)
    flat = [R for v in rows.values() for R in v]
    assert 64 in flat and 65 in flat and 63 in flat and 66 in flat
    mixed = [k for k, v in rows.items() if min(v) <= 64 < max(v)]
    # 91 -> 24 is [65, 64]; 151 -> 40 is [65, 65, 64]; 377 -> 100 is [64, 65, 64, 64, 65, 65, 64]: both paths between full tiles
    assert {k[0] for k in mixed} >= {"path_edge_s24", "path_edge_s40", "path_edge_s100"}, mixed
    assert CC.tile_rows(plan, 377, 100) == [64, 65, 64, 64, 65, 65, 64]
    for S, name in ((16, "path_edge_s16"), (24, "path_edge_s24"), (40, "path_edge_s40"), (100, "path_edge_s100")):
        c = CC.case(plan, name)
        hs = (c.boxes[:, 3] - c.boxes[:, 1]).tolist()
        ws = (c.boxes[:, 2] - c.boxes[:, 0]).tolist()
        for h in c.notes["heights"]:
            w_of_h = {w for w, hh in zip(ws, hs) if hh == h}
            assert h in w_of_h and 8 in w_of_h and any(w > h for w in w_of_h), (name, h)
    assert {tuple(CC.case(plan, n).notes["heights"]) for n in CC.NAMES if n.startswith("path_edge")} == \
        {(59, 60, 61, 62), (90, 91, 92), (147, 148, 150, 151), (366, 370, 377, 380)}


def test_a_phantom_row_flips_the_path_of_a_ragged_tile(plan):
    """92 rows -> 24: the last tile has 8 existing rows that touch 35 source rows, but its sixteenth, phantom row stretches the
    window to 66 rows: direct path, where its real rows alone would be separable"""
    assert CC.tile_rows(plan, 92, 24) == [65, 66] and CC.tile_rows_live(plan, 92, 24) == [65, 35]
    flipped = []
    for name in CC.NAMES:
        c = CC.case(plan, name)
        for b, box in enumerate(c.boxes.tolist()):
            if CC.is_live(box):
                full, real = CC.tile_rows(plan, box[3] - box[1], c.S), CC.tile_rows_live(plan, box[3] - box[1], c.S)
                assert full[:-1] == real[:-1] and (c.S % 16 != 0 or full == real)
                if bool(plan.crop_separable(full[-1])) != bool(plan.crop_separable(real[-1])):
                    flipped.append((name, b))
    assert any(n == "path_edge_s24" for n, _ in flipped), flipped
    print("crops whose ragged last tile is moved to the direct path by its phantom row:", flipped)


def test_every_tile_starts_on_an_existing_row(plan):
    for S in (1, 16, 17, 24, 31, 33, 40, 78, 100, 128, 256):
        assert (plan.crop_tile_count(S) - 1) * plan.crop_tile() < S


def test_border_boxes_touch_what_they_claim(plan):
    for name in ("borders", "borders_u8"):
        c = CC.case(plan, name)
        H, W = c.mask.shape
        assert H % 2 == 1 and W % 2 == 1 and len(c.boxes) == len(c.notes["claims"])
        for (x0, y0, x1, y1), claim in zip(c.boxes.tolist(), c.notes["claims"]):
            touched = {k for k, v in (("left", x0 == 0), ("top", y0 == 0), ("right", x1 == W), ("bottom", y1 == H)) if v}
            assert touched == claim
        claims = [frozenset(k) for k in c.notes["claims"]]
        for want in ({"left"}, {"top"}, {"right"}, {"bottom"}, {"left", "top"}, {"right", "top"}, {"left", "bottom"}, {"right", "bottom"}):
            assert frozenset(want) in claims
        assert c.boxes[8].tolist() == [0, 0, W, H] and c.boxes[9].tolist() == [W - 1, H - 1, W, H]
    assert (CC.case(plan, "borders_u8").mask == 255).all() and len(np.unique(CC.case(plan, "borders").mask)) > 200


@pytest.mark.parametrize("S", [40, 48])
def test_narrow_axes_clamp_every_tap(plan, S):
    """each of the eight taps leaves the crop at some output index; below 8 pixels some tap does at every index; at 1 pixel all do"""
    c = CC.case(plan, f"narrow_s{S}")
    pairs = {(int(b[2] - b[0]), int(b[3] - b[1])) for b in c.boxes}
    assert {(w, h) for w in CC.NARROW for h in CC.NARROW} <= pairs and {(1, 40), (40, 1)} <= pairs
    assert (S % 16 == 0) == (S == 48)
    for n in CC.NARROW:
        s, _, _ = CC.axis(n, S, S)
        taps = s[:, None] - 3 + np.arange(8)
        out = (taps < 0) | (taps > n - 1)
        assert out.any(axis=0).all(), n
        assert n >= 8 or out.any(axis=1).all()
        assert n > 1 or out.sum() == 7 * S               # one pixel: the seven taps off it clamp onto it at every index
        assert n <= S                                     # up-scaled


def test_identity_covers_every_pair(plan):
    c = CC.case(plan, "identity_all_pairs")
    pairs = c.rgb[:, :, 0].astype(np.int64) * 256 + c.mask
    assert len(np.unique(pairs)) == 65536 and (c.rgb[:, :, 1] == c.rgb[:, :, 0]).all() and (c.rgb[:, :, 2] == c.rgb[:, :, 0]).all()
    assert c.S == 256 and c.boxes.tolist() == [[0, 0, 256, 256]]
    ref = CC.reference_f32(c)
    want = (c.rgb[:, :, 0].astype(np.float64) * (c.mask / 255.0) / 255.0).astype(np.float32)
    assert np.array_equal(ref[0, 0], want)
    f32 = (c.rgb[:, :, 0].astype(np.float32) * (c.mask.astype(np.float32) / np.float32(255)) / np.float32(255))
    assert (f32 != want).any()                            # float32 arithmetic is told apart


def test_one_axis_identity_and_degenerate_cases(plan):
    c = CC.case(plan, "one_axis_identity")
    wh = [(int(b[2] - b[0]), int(b[3] - b[1])) for b in c.boxes]
    assert any(w == c.S != h for w, h in wh) and any(h == c.S != w for w, h in wh) and (c.S, c.S) in wh
    _, wt, _ = CC.axis(c.S, c.S, c.S)
    assert (wt == np.array([0, 0, 0, 2048, 0, 0, 0, 0])).all()
    c = CC.case(plan, "degenerate")
    d = [(int(b[2] - b[0]), int(b[3] - b[1])) for b in c.boxes]
    kinds = {(np.sign(w), np.sign(h)) for w, h in d}
    assert {(0, 1), (1, 0), (0, 0), (-1, 1), (1, -1), (-1, -1), (1, 1)} <= kinds
    live = [CC.is_live(b) for b in c.boxes.tolist()]
    assert live[0] and live[-1] and live.count(False) == 6                           # the empty boxes sit between live ones
    assert any(not live[i] and live[i + 1] for i in range(9)) and any(live[i] and not live[i + 1] for i in range(9))
    ref = CC.reference_f32(c)
    assert all((ref[i] == 0).all() != live[i] for i in range(len(live)))


def test_weight_tie_axes_round_differently(plan):
    c = CC.case(plan, "weight_tie")
    for n in c.notes["tie_axes"]:
        _, wt, raw = CC.axis(n, c.S, c.S)
        up = np.floor(raw + np.float32(0.5)).astype(np.int64)
        assert (up != wt).any() and np.abs(up - wt).max() == 1, n
    used = {int(v) for b in c.boxes for v in (b[2] - b[0], b[3] - b[1])}
    assert set(c.notes["tie_axes"]) <= used


def _sums64(img, S):
    """vertical sums of resize_lanczos4_u8 before rounding, int64 [S, S]"""
    h, w = img.shape
    xi, xw = P._axis_table(w, S)
    yi, yw = P._axis_table(h, S)
    src = img.astype(np.int64)
    hor = np.einsum("hdk,dk->hd", src[:, xi], xw)
    return np.einsum("dkw,dk->dw", hor[yi, :], yw)


def test_worst_accumulator_case_reaches_its_margin(plan):
    c = CC.case(plan, "worst_acc")
    n, S, d1 = CC.WORST_AXIS
    d2, pat = c.notes["d2"], c.notes["pattern"]
    _, wt, _ = CC.axis(n, S, S)
    Pp, N = CC.axis_pn(wt[d1])
    ver = _sums64(pat, S)
    assert ver[d1, d1] == 255 * (Pp * Pp + N * N) == ver.max() == 2107377120
    P2, N2 = CC.axis_pn(wt[d2])
    assert ver[d2, d2] == -255 * 2 * P2 * N2 == ver.min()
    print(f"worst_acc: largest vertical sum {int(ver.max())} = {ver.max() / 2**31:.4f} x 2^31 (P {Pp}, N {N}); most negative {int(ver.min())}")
    assert np.abs(ver).max() >= 0.95 * 2**31 and np.abs(ver).max() + 2**21 < 2**31
    for b, (x0, y0, x1, y1) in enumerate(c.boxes.tolist()):           # both boxes hold the pattern: in rgb, and in the mask
        for img in ([c.rgb[y0:y1, x0:x1, k] for k in range(3)] if b == 0 else [c.mask[y0:y1, x0:x1]]):
            assert np.array_equal(img, pat)
    ref = CC.reference_f32(c)
    assert (ref[:, :, d1, d1] == 1).all() and (ref[:, :, d2, d2] == 0).all()      # 255 and 0 after saturation
    # noise never comes near: a flat 255 image gives 255 * 2048^2 = 0.498 x 2^31, these stay below 0.75 x 2^31
    for name in ("borders", "ragged_s33"):
        o = CC.case(plan, name)
        x0, y0, x1, y1 = o.boxes[0].tolist()
        assert np.abs(_sums64(o.rgb[y0:y1, x0:x1, 0], o.S)).max() < 0.75 * 2**31


def test_accumulator_bound_for_every_fraction():
    """over every t = k / 65536: with P, N the positive and negative sums of the quantised weights of one axis, no image can drive
    the vertical sum past 255 (Px Py + Nx Ny) <= 255 max(P^2 + N^2) (Cauchy-Schwarz); that and the rounding term stay below 2^31"""
    best = (0, None)
    for k in range(65536):
        q = np.rint(P._lanczos4_coeffs(np.float32(k / 65536)).astype(np.float32) * np.float32(2048)).astype(np.int64)
        Pp, N = CC.axis_pn(q)
        best = max(best, (255 * (Pp * Pp + N * N), k, Pp, N))
    print(f"largest reachable |acc| over t = k / 65536: {best[0]} = {best[0] / 2**31:.4f} x 2^31 at k = {best[1]} (P {best[2]}, N {best[3]})")
    assert best[0] == 2107377120 and best[0] + 2**21 < 2**31
    n, S, d = CC.WORST_AXIS
    assert CC.axis_pn(CC.axis(n, S, S)[1][d]) == (best[2], best[3])


def test_frames_are_small_and_odd_sizes_occur(plan):
    shapes = [CC.case(plan, n).mask.shape for n in CC.NAMES]
    assert all(h <= 400 and w <= 400 for h, w in shapes)
    assert any(w % 2 for _, w in shapes) and any(h % 2 for h, _ in shapes)
    for n in CC.NAMES:
        c = CC.case(plan, n)
        if n not in ("identity_all_pairs",) and not n.endswith("_u8"):
            assert len(np.unique(c.mask)) > 200, n                      # the mask takes the values between, not only 0 and 255
    assert {CC.case(plan, n).S for n in CC.NAMES if n.startswith("ragged")} == {17, 24, 31, 33, 100}


# ---- 3. the emulation and its broken copies ------------------------------------------------------------------------------------------------
class Emu:
    """The kernel's algorithm in numpy.  `brk` names one deliberate defect; None is the kernel as written."""

    def __init__(self, lib, brk=None):
        self.lib, self.brk = lib, brk
        self.T, self.LIM = lib.crop_tile(), lib.crop_rows_limit()

    def axis(self, n, S):
        s, wt, raw = CC.axis(n, S, self.lib.crop_tile_count(S) * self.T)
        if self.brk == "half_up":
            wt = np.clip(np.floor(raw + np.float32(0.5)).astype(np.int64), -32768, 32767)
        return s.astype(np.int32), wt.astype(np.int32)

    def between(self, hor):
        if self.brk == "round_between":
            return (hor + np.int32(1 << 10)) >> 11
        if self.brk == "hor_int16":
            return hor.astype(np.int16).astype(np.int32)
        return hor

    def fin(self, v):
        if self.brk == "round_between":
            v = (v + np.int32(1 << 10)) >> 11
        elif self.brk == "truncate":
            v = v >> 22
        else:
            v = (v + np.int32(1 << 21)) >> 22
        return np.clip(v, 0, 255)

    def unit(self, img, m):
        if self.brk == "unit_f32":
            return img.astype(np.float32) * (m.astype(np.float32) / np.float32(255)) / np.float32(255)
        return (img.astype(np.float64) * (m.astype(np.float64) / 255.0) / 255.0).astype(np.float32)

    def crop(self, c, src, box):
        """-> (float32 [S, S, 3], [(rows, separable) per tile row]) of a live box"""
        H, W = c.mask.shape
        S, T, LIM = c.S, self.T, self.LIM
        x0, y0, x1, y1 = box
        cw, ch = x1 - x0, y1 - y0
        nt = self.lib.crop_tile_count(S)
        sx, wx = self.axis(cw, S)
        sy, wy = self.axis(ch, S)
        k8 = np.arange(8, dtype=np.int32)

        def rows(yy):
            if self.brk == "clamp_frame":
                return np.clip(y0 + yy, 0, H - 1)
            return np.minimum(y0 + np.clip(yy, 0, (cw if self.brk == "cw_row_clamp" else ch) - 1), H - 1)

        xx = sx[:, None] - 3 + k8
        xcols = np.clip(x0 + xx, 0, W - 1) if self.brk == "clamp_frame" else x0 + np.clip(xx, 0, cw - 1)       # [nt * T, 8]
        out = np.zeros((nt * T, nt * T, 3), np.float32)
        paths = []
        for ty in range(nt):
            sy_t, wy_t = sy[ty * T:(ty + 1) * T], wy[ty * T:(ty + 1) * T]
            r0 = self.lib.crop_first_row(int(sy_t[0]))
            last = min(T - 1, S - 1 - ty * T) if self.brk == "rows_from_last_live" else T - 1
            R = self.lib.crop_rows(int(sy_t[0]), int(sy_t[last]))
            sep = bool(self.lib.crop_separable(R))
            if self.brk == "limit_lt":
                sep = R < LIM
            if self.brk == "limit_wrap":
                sep = R <= LIM + 1
            paths.append((R, sep))
            if sep:
                start = max(r0, 0) if self.brk == "r0_live" else r0
                g = src[rows(start + np.arange(R, dtype=np.int32))][:, xcols]                      # [R, cols, 8, 4]
                hor = self.between((g * wx[None, :, :, None]).sum(2, dtype=np.int32))              # [R, cols, 4]
                win = np.zeros((LIM,) + hor.shape[1:], np.int32)                                   # hor[kCropRows][16][4]
                win[:min(R, LIM)] = hor[:LIM]
                if R > LIM:
                    win[:R - LIM] = hor[LIM:R]                                                     # a longer window wraps onto its start
                rb = sy_t - 3 - r0
                idx = (rb[:, None] + k8) % LIM                                                     # [T, 8]
                acc = (win[idx] * wy_t[:, :, None, None]).sum(1, dtype=np.int32)                   # [T, cols, 4]
            else:
                g = src[rows(sy_t[:, None] - 3 + k8)][:, :, xcols]                                 # [T, 8, cols, 8, 4]
                hor = self.between((g * wx[None, None, :, :, None]).sum(3, dtype=np.int32))        # [T, 8, cols, 4]
                acc = (hor * wy_t[:, :, None, None]).sum(1, dtype=np.int32)
            v = self.fin(acc)
            m = np.full_like(v[:, :, 3:], 255) if self.brk == "premultiply" else v[:, :, 3:]
            out[ty * T:(ty + 1) * T] = self.unit(v[:, :, :3], m)
        return out[:S, :S], paths

    def run(self, c, fmt="f32"):
        """-> (the output buffer as element bits, per box its tile-row paths or None)"""
        S, T = c.S, self.T
        rgb = c.rgb.astype(np.int32)
        if self.brk == "premultiply":
            rgb = (rgb * c.mask[:, :, None].astype(np.int32) + 127) // 255
        src = np.concatenate([rgb, c.mask[:, :, None].astype(np.int32)], axis=2)                  # [H, W, 4] int32
        n = CC.n_elements(c)
        total = n + 3 * S * S
        buf = np.full(2 * total + 64 * S * len(c.boxes) * 3, CC.SENTINEL[fmt], CC.BITS_DTYPE[fmt])    # room for a wrong stride
        Sp = (S + T - 1) // T * T if self.brk == "stride16" else S
        dy, dx = np.mgrid[:S, :S]
        paths = []
        for b, box in enumerate(c.boxes.tolist()):
            if not CC.is_live(box):
                paths.append(None)
                if self.brk == "degenerate_unwritten":
                    continue
                val = np.zeros((S, S, 3), np.float32)
            else:
                val, p = self.crop(c, src, box)
                paths.append(p)
            for ch in range(3):
                if fmt == "f32":
                    at = (b * 3 * S + dy) * Sp + dx + ch * S * S
                    bits = val[:, :, ch].view(np.uint32)
                else:
                    at = ((b * S + dy) * Sp + dx) * 3 + ch
                    if fmt == "f16":
                        bits = val[:, :, ch].astype(np.float16).view(np.uint16)
                    else:                                                       # round to nearest even on the upper 16 bits
                        u = np.ascontiguousarray(val[:, :, ch]).view(np.uint32)
                        bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
                buf[at.ravel()] = np.ascontiguousarray(bits).ravel()
        return buf[:total].copy(), paths


def _noticed(plan, c, fmt, buf, paths):
    fails = CC.check(plan, c, fmt, buf)
    if paths != CC.tile_paths(plan, c):
        fails.append(f"{c.name}: the path map differs from crop_plan.h's")
    return fails


@pytest.mark.parametrize("name", CC.NAMES)
def test_unbroken_emulation_passes(plan, name):
    c = CC.case(plan, name)
    buf, paths = Emu(plan).run(c)
    fails = _noticed(plan, c, "f32", buf, paths)
    sep, direct, mixed = CC.path_counts(plan, c)
    print(f"{name}: {len(c.boxes)} boxes at S = {c.S}: {sep} tiles separable, {direct} direct, {mixed} crops with both")
    assert not fails, fails[:5]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["degenerate", "ragged_s17", "path_edge_s24", "identity_all_pairs"])
def test_unbroken_emulation_passes_in_16_bit(plan, name, fmt):
    c = CC.case(plan, name)
    buf, _ = Emu(plan).run(c, fmt)
    fails = CC.check(plan, c, fmt, buf)
    assert not fails, fails[:5]


BREAKS = ["clamp_frame", "limit_lt", "limit_wrap", "r0_live", "rows_from_last_live", "cw_row_clamp", "premultiply", "round_between",
          "truncate", "half_up", "unit_f32", "hor_int16", "degenerate_unwritten", "stride16"]


@pytest.mark.parametrize("brk", BREAKS)
def test_broken_emulation_is_noticed(plan, brk):
    caught = {}
    for name in CC.NAMES:
        c = CC.case(plan, name)
        fails = _noticed(plan, c, "f32", *Emu(plan, brk).run(c))
        if fails:
            caught[name] = len(fails)
            break
    print(f"{brk}: first noticed by {caught}")
    assert caught, f"no case notices the break {brk!r}: a case is missing"


def test_what_each_break_needs(plan):
    """the cases are not interchangeable: each break is noticed by the case built for it, in output bits unless stated otherwise"""
    for brk, name, fmt in (("limit_wrap", "path_edge_s16", "f32"), ("limit_wrap", "path_edge_s24", "f32"), ("half_up", "weight_tie", "f32"),
                           ("unit_f32", "identity_all_pairs", "f32"), ("degenerate_unwritten", "degenerate", "f32"),
                           ("stride16", "ragged_s17", "f32"), ("stride16", "ragged_s17", "bf16"), ("stride16", "ragged_s33", "f16"),
                           ("cw_row_clamp", "narrow_s40", "f32"), ("cw_row_clamp", "one_axis_identity", "f32"),
                           ("clamp_frame", "narrow_s48", "f32"), ("hor_int16", "worst_acc", "f32"), ("r0_live", "borders", "f32"),
                           ("premultiply", "borders", "f32"), ("round_between", "ragged_s24", "f32"), ("truncate", "ragged_s31", "f32")):
        c = CC.case(plan, name)
        buf, _ = Emu(plan, brk).run(c, fmt)
        assert CC.check(plan, c, fmt, buf), (brk, name, fmt)
    # the two breaks that move tiles between bit-identical paths: no bit differs, the path map does
    for brk, name in (("limit_lt", "path_edge_s16"), ("limit_lt", "path_edge_s40"), ("rows_from_last_live", "path_edge_s24")):
        c = CC.case(plan, name)
        buf, paths = Emu(plan, brk).run(c)
        assert not CC.check(plan, c, "f32", buf) and paths != CC.tile_paths(plan, c), (brk, name)
    # stride16 and an S that is a multiple of 16: nothing to see, which is why the ragged S are there
    c = CC.case(plan, "narrow_s48")
    assert not CC.check(plan, c, "f32", Emu(plan, "stride16").run(c)[0])


def test_checker_sees_the_tail_and_names_tile_and_path(plan):
    c = CC.case(plan, "path_edge_s24")
    buf, _ = Emu(plan).run(c)
    n = CC.n_elements(c)
    bad = buf.copy()
    bad[n + 5] = 0
    assert any("behind the last crop" in f for f in CC.check(plan, c, "f32", bad))
    b = next(i for i, box in enumerate(c.boxes.tolist()) if box[3] - box[1] == 91)          # tiles of 65 and 64 rows
    bad = buf.copy()
    bad[(b * 3 * 24 + 20) * 24 + 3] ^= 1                                                     # channel 0, dy 20, dx 3
    fails = CC.check(plan, c, "f32", bad)
    assert len(fails) == 1 and f"crop {b} " in fails[0] and "1 mismatching elements" in fails[0], fails
    assert "dy 20 dx 3" in fails[0] and "tile (1, 0) of 64 rows on the separable path" in fails[0], fails
    bad[(b * 3 * 24 + 2) * 24 + 17] ^= 1
    assert "tile (0, 1) of 65 rows on the direct path; 1 mismatches on the separable path, 1 on the direct path" in CC.check(plan, c, "f32", bad)[0]
