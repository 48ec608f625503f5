"""Edge cases of the crop + Lanczos-4 resize + mask kernel (flope_amd/csrc/prep.hip: crop_resize_mask_tiled_kernel,
flope_crop_resize_mask) and the checker both halves of its tests share: tests/test_crop_cases.py (CPU: the builder's promises, an
emulation of the kernel and its broken copies) and tests/test_gpu_crop_cases.py (the kernel itself).

The claim under test is bit-exactness against oracle.pipeline_ref.crop_batch, so the checker knows no tolerance: every element of
the output buffer is compared as bits.

A case is (name, rgb uint8 [H, W, 3], mask uint8 [H, W], boxes int32 [N, 4] = x0, y0, x1, y1, S) + notes of the builder.  Every
box lies inside its frame (0 <= x0, x1 <= W, 0 <= y0, y1 <= H; the builder asserts it: the kernel trusts its boxes).  rgb and mask
are seeded noise over 0 .. 255 unless the case says otherwise.

The tile edge, the LDS window and the rule that picks a tile's path come from the header the kernel includes
(flope_amd/csrc/crop_plan.h through tests/host_harness/harness_crop.cpp), never from a Python copy.  The first-tap positions the
rule is fed with come from the formula of oracle.pipeline_ref._axis_table_raw, here evaluated for d >= S too: the sixteenth row
of a ragged last tile is such a phantom index.  tests/test_gpu_parity.py::test_lanczos_tables_bit_exact_vs_oracle pins that
formula against the device for d < S only; THE PATH MODEL FOR PHANTOM INDICES RESTS ON THE SAME FORMULA AND IS NOT READ BACK FROM
THE DEVICE.  It decides which path a mismatch is reported under and what the builder promises, not what the output must be: the
two paths are claimed bit-identical, and the expected bits come from the oracle alone.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import pipeline_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("f32", "bf16", "f16")                   # float32 NCHW, bfloat16 NHWC, float16 NHWC
FMT_CODE = {"f32": 0, "bf16": 1, "f16": 2}         # flope_amd._lib.IN_F32_NCHW, IN_BF16_NHWC, IN_F16_NHWC
BITS_DTYPE = {"f32": np.uint32, "bf16": np.uint16, "f16": np.uint16}
SENTINEL_BYTE = 0xA5                               # 0xA5A5A5A5 / 0xA5A5 are negative numbers: no output in [0, 1] has these bits
SENTINEL = {"f32": 0xA5A5A5A5, "bf16": 0xA5A5, "f16": 0xA5A5}

Case = collections.namedtuple("Case", "name rgb mask boxes S notes")


# ---- the tile plan, from the header the kernel includes -----------------------------------------------------------------------------
def load_plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_crop.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_crop.so"])
    return C.CDLL(path)


_AXIS = {}


def axis(n_src, S, count):
    """one axis resized n_src -> S, destination indices 0 .. count - 1 (count may exceed S: phantom indices) ->
    (first-tap position s int64 [count], int16-range weights int64 [count, 8], the float32 products co * 2048 they are rounded from)"""
    key = (int(n_src), int(S), int(count))
    if key not in _AXIS:
        scale = P._resize_scale(n_src, S)
        s_all, wt, raw = np.zeros(count, np.int64), np.zeros((count, 8), np.int64), np.zeros((count, 8), np.float32)
        for d in range(count):
            f = np.float32((d + 0.5) * scale - 0.5)
            s = int(np.floor(f))
            f = np.float32(f - np.float32(s))
            raw[d] = P._lanczos4_coeffs(f).astype(np.float32) * np.float32(2048)
            wt[d] = np.clip(np.rint(raw[d]).astype(np.int64), -32768, 32767)
            s_all[d] = s
        _AXIS[key] = (s_all, wt, raw)
    return _AXIS[key]


def tile_rows(lib, n_src, S):
    """source rows each tile row of an axis n_src -> S touches, by crop_plan.h's rule fed with the oracle's first-tap positions"""
    T, nt = lib.crop_tile(), lib.crop_tile_count(S)
    s, _, _ = axis(n_src, S, nt * T)
    return [lib.crop_rows(int(s[t * T]), int(s[t * T + T - 1])) for t in range(nt)]


def tile_rows_live(lib, n_src, S):
    """the same from each tile's last EXISTING output row: what the window would be without phantom rows"""
    T, nt = lib.crop_tile(), lib.crop_tile_count(S)
    s, _, _ = axis(n_src, S, nt * T)
    return [lib.crop_rows(int(s[t * T]), int(s[min(t * T + T - 1, S - 1)])) for t in range(nt)]


def is_live(box):
    return box[2] - box[0] > 0 and box[3] - box[1] > 0


def tile_paths(lib, c):
    """per box: None for a degenerate box, else one (rows, separable) per tile row; every tile of a tile row takes the same path"""
    out = []
    for box in c.boxes.tolist():
        out.append([(R, bool(lib.crop_separable(R))) for R in tile_rows(lib, box[3] - box[1], c.S)] if is_live(box) else None)
    return out


def path_counts(lib, c):
    """-> (tiles on the separable path, tiles on the direct path, crops whose tiles take both)"""
    nt = lib.crop_tile_count(c.S)
    sep = direct = mixed = 0
    for p in tile_paths(lib, c):
        if p is None:
            continue
        a = sum(1 for _, s in p if s)
        sep += a * nt
        direct += (len(p) - a) * nt
        mixed += 0 < a < len(p)
    return sep, direct, mixed


# ---- frames and boxes --------------------------------------------------------------------------------------------------------------------
def _noise(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


def _place(sizes, H, W, seed):
    """boxes of the given (w, h) at seeded positions inside an H x W frame"""
    rng = np.random.default_rng(seed)
    boxes = []
    for w, h in sizes:
        x0, y0 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        boxes.append([x0, y0, x0 + w, y0 + h])
    return boxes


def _case(name, rgb, mask, boxes, S, **notes):
    H, W = mask.shape
    b = np.array(boxes, np.int32).reshape(-1, 4)
    assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8 and mask.dtype == np.uint8 and H <= 400 and W <= 400
    assert (b[:, [0, 2]] >= 0).all() and (b[:, [0, 2]] <= W).all() and (b[:, [1, 3]] >= 0).all() and (b[:, [1, 3]] <= H).all(), name
    return Case(name, rgb, mask, b, S, notes)


def _path_edge(S, heights, H, W, wider, seed):
    """crops whose row counts sit on both sides of the kCropRows limit, each as wide as high, 8 wide and wider than high"""
    def build(lib):
        rgb, mask = _noise(H, W, seed)
        sizes = [(w, h) for h in heights for w in (h, 8, h + wider)]
        return _case(f"path_edge_s{S}", rgb, mask, _place(sizes, H, W, seed + 1), S, heights=heights)
    return build


BORDER_CLAIMS = ({"left"}, {"top"}, {"right"}, {"bottom"}, {"left", "top"}, {"right", "top"}, {"left", "bottom"},
                 {"right", "bottom"}, {"left", "top", "right", "bottom"}, {"right", "bottom"})


def _border_boxes(H, W):
    return [[0, 10, 20, 30], [15, 0, 40, 22], [40, 12, W, 33], [18, 30, 44, H],                       # the four borders
            [0, 0, 17, 19], [W - 21, 0, W, 16], [0, H - 18, 23, H], [W - 19, H - 22, W, H],           # the four corners
            [0, 0, W, H], [W - 1, H - 1, W, H]]                                                       # the whole frame; its last pixel


def _borders(u8):
    def build(lib):
        H, W = 53, 61
        rgb, mask = _noise(H, W, 41)
        if u8:
            mask = np.full((H, W), 255, np.uint8)
        return _case("borders_u8" if u8 else "borders", rgb, mask, _border_boxes(H, W), 40, claims=BORDER_CLAIMS)
    return build


NARROW = (1, 2, 3, 7, 8, 9)


def _narrow(S, u8):
    def build(lib):
        H, W = 45, 47
        rgb, mask = _noise(H, W, 42 + S)
        if u8:
            mask = np.full((H, W), 255, np.uint8)
        sizes = [(w, h) for w in NARROW for h in NARROW] + [(1, 40), (40, 1), (3, 40), (40, 7), (9, 40), (40, 2)]
        return _case(f"narrow_s{S}" + ("_u8" if u8 else ""), rgb, mask, _place(sizes, H, W, 43 + S), S)
    return build


def _identity_all_pairs(lib):
    """rgb = column index, mask = row index, the whole 256 x 256 frame at S = 256: every (img, m) pair meets masked_unit once"""
    col = np.tile(np.arange(256, dtype=np.uint8), (256, 1))
    rgb = np.ascontiguousarray(np.stack([col, col, col], axis=2))
    mask = np.ascontiguousarray(col.T)
    return _case("identity_all_pairs", rgb, mask, [[0, 0, 256, 256]], 256)


def _one_axis_identity(lib):
    """one axis at scale 1 (its weights are 0, 0, 0, 2048, 0, 0, 0, 0), the other resized; cv2 copies only when both match"""
    H, W = 97, 101
    rgb, mask = _noise(H, W, 44)
    sizes = [(40, 29), (40, 93), (29, 40), (93, 40), (40, 40), (40, 41), (39, 40)]
    return _case("one_axis_identity", rgb, mask, _place(sizes, H, W, 45), 40)


def _degenerate(lib):
    """empty and inverted boxes between live ones: the device writes zeros for them (the reference has no answer: its slice is
    empty and cv2.resize rejects it)"""
    H, W = 41, 45
    rgb, mask = _noise(H, W, 46)
    boxes = [[3, 4, 30, 29], [10, 5, 10, 30], [5, 6, 25, 20], [8, 12, 33, 12], [20, 20, 20, 20], [1, 1, 9, 40],
             [30, 8, 12, 33], [6, 35, 31, 10], [25, 30, 12, 5], [0, 0, W, H]]
    return _case("degenerate", rgb, mask, boxes, 24)


# (n_src, S, d): at destination index d of an axis resized 79 -> 128 the fraction is t = 0.48828125 and the quantised weights have
# P = 2780, N = 732, the pair at which 255 (P^2 + N^2) is largest over every t = k / 65536 (tests/test_crop_cases.py searches again)
WORST_AXIS = (79, 128, 121)


def axis_pn(wt):
    wt = np.asarray(wt, np.int64)
    return int(wt[wt > 0].sum()), int(-wt[wt < 0].sum())


def _worst_acc(lib):
    """the image that drives the int32 accumulators furthest: 255 where the outer product of the two weight vectors of output
    pixel (d1, d1) is positive, 0 elsewhere (all 64 products add: 255 (P^2 + N^2)), and at a second pixel (d2, d2) whose taps share
    nothing with the first the complement (255 where negative: -255 * 2 P N).  Box 0 carries the pattern in rgb under a mask of
    255, box 1 carries it in the mask under rgb of 255: the mask runs through the same accumulators."""
    n, S, d1 = WORST_AXIS
    s, wt, _ = axis(n, S, S)
    inner = lambda d: s[d] - 3 >= 0 and s[d] + 4 <= n - 1
    assert inner(d1)
    cand = [d for d in range(S) if inner(d) and abs(int(s[d]) - int(s[d1])) >= 8]
    d2 = max(cand, key=lambda d: (np.prod(axis_pn(wt[d])), -d))
    rng = np.random.default_rng(47)
    pat = rng.integers(0, 256, (n, n), dtype=np.uint8)
    a, b = int(s[d1]) - 3, int(s[d2]) - 3
    pat[a:a + 8, a:a + 8] = np.where(np.outer(wt[d1], wt[d1]) > 0, 255, 0)
    pat[b:b + 8, b:b + 8] = np.where(np.outer(wt[d2], wt[d2]) < 0, 255, 0)
    H, W = n + 2, 2 * n + 3
    rgb, mask = _noise(H, W, 48)
    rgb[1:1 + n, 1:1 + n] = pat[:, :, None]
    mask[1:1 + n, 1:1 + n] = 255
    rgb[1:1 + n, n + 2:2 * n + 2] = 255
    mask[1:1 + n, n + 2:2 * n + 2] = pat
    return _case("worst_acc", rgb, mask, [[1, 1, 1 + n, 1 + n], [n + 2, 1, 2 * n + 2, 1 + n]], S, d1=d1, d2=int(d2), pattern=pat)


def _weight_tie(lib):
    """axes on which some float32 product co * 2048 is exactly 316.5: cvRound (half to even) gives 316, rounding half up 317.  Over
    every fraction j / 2S with S < 420 only eleven have such a tie with an even floor; 5, 7, 11 and 59 -> 78 reach one"""
    H, W = 63, 67
    rgb, mask = _noise(H, W, 49)
    sizes = [(7, 7), (7, 59), (59, 7), (11, 5), (5, 11)]
    return _case("weight_tie", rgb, mask, _place(sizes, H, W, 50), 78, tie_axes=(5, 7, 11, 59))


def _ragged(S, seed):
    """S that is no multiple of the tile, up-scaled about 3x, about 1x, and down-scaled about 3x, square and mixed"""
    def build(lib):
        up, down = S // 3 + 1, 3 * S + 1
        H, W = down + 4, down + 10
        rgb, mask = _noise(H, W, seed)
        sizes = [(up, up), (S + 1, S - 1), (down, down), (up, down), (down, S + 1)]
        return _case(f"ragged_s{S}", rgb, mask, _place(sizes, H, W, seed + 1), S)
    return build


BUILDERS = collections.OrderedDict([
    ("degenerate", _degenerate), ("borders", _borders(False)), ("borders_u8", _borders(True)),
    ("narrow_s40", _narrow(40, False)), ("narrow_s48", _narrow(48, False)), ("narrow_s40_u8", _narrow(40, True)),
    ("narrow_s48_u8", _narrow(48, True)), ("one_axis_identity", _one_axis_identity),
    ("path_edge_s16", _path_edge(16, (59, 60, 61, 62), 67, 75, 9, 51)), ("path_edge_s24", _path_edge(24, (90, 91, 92), 97, 107, 11, 53)),
    ("ragged_s17", _ragged(17, 61)), ("ragged_s24", _ragged(24, 63)), ("ragged_s31", _ragged(31, 65)), ("ragged_s33", _ragged(33, 67)),
    ("weight_tie", _weight_tie), ("worst_acc", _worst_acc), ("path_edge_s40", _path_edge(40, (147, 148, 150, 151), 155, 167, 13, 55)),
    ("identity_all_pairs", _identity_all_pairs), ("ragged_s100", _ragged(100, 69)),
    ("path_edge_s100", _path_edge(100, (366, 370, 377, 380), 383, 397, 15, 57)),
])
NAMES = tuple(BUILDERS)
_CASES, _REF = {}, {}


def case(lib, name):
    """built once per process; treat the arrays as read-only"""
    if name not in _CASES:
        c = BUILDERS[name](lib)
        assert c.name == name
        for a in (c.rgb, c.mask, c.boxes):
            a.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


# ---- the reference and the checker ---------------------------------------------------------------------------------------------------------
def n_elements(c):
    return len(c.boxes) * 3 * c.S * c.S


def new_buffer(c, fmt):
    """the output buffer as element bits: the crops and one more crop's worth behind them, all sentinel"""
    return np.full(n_elements(c) + 3 * c.S * c.S, SENTINEL[fmt], BITS_DTYPE[fmt])


def reference_f32(c):
    """float32 [N, 3, S, S]: oracle.pipeline_ref.crop_batch cast as the reference casts it; zeros for a degenerate box"""
    key = (c.name, "f32")
    if key not in _REF:
        out = np.zeros((len(c.boxes), 3, c.S, c.S), np.float32)
        for b, box in enumerate(c.boxes.tolist()):
            if is_live(box):
                out[b] = P.crop_batch(c.rgb, c.mask, [box], c.S)[0].transpose(2, 0, 1).astype(np.float32)
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def reference_bits(c, fmt):
    """the bits every element of the N crops must have, flat in the layout of the format"""
    key = (c.name, fmt, "bits")
    if key not in _REF:
        f = reference_f32(c)
        if fmt == "f32":
            bits = f.view(np.uint32).reshape(-1).copy()
        else:
            import torch
            t = torch.from_numpy(np.ascontiguousarray(f.transpose(0, 2, 3, 1))).to(torch.bfloat16 if fmt == "bf16" else torch.float16)
            bits = t.view(torch.int16).numpy().view(np.uint16).reshape(-1).copy()
        bits.setflags(write=False)
        _REF[key] = bits
    return _REF[key]


def reference_u8(c):
    """uint8 [N, 3, S, S] by oracle.pipeline_ref.resize_lanczos4_u8: what an all-255 mask lets through"""
    key = (c.name, "u8")
    if key not in _REF:
        out = np.zeros((len(c.boxes), 3, c.S, c.S), np.uint8)
        for b, (x0, y0, x1, y1) in enumerate(c.boxes.tolist()):
            if is_live((x0, y0, x1, y1)):
                out[b] = P.resize_lanczos4_u8(c.rgb[y0:y1, x0:x1], c.S).transpose(2, 0, 1)
        _REF[key] = out
    return _REF[key]


def _where(c, fmt, i):
    """flat element index -> (crop, channel, dy, dx)"""
    S = c.S
    if fmt == "f32":
        b, ch, dy, dx = np.unravel_index(i, (len(c.boxes), 3, S, S))
    else:
        b, dy, dx, ch = np.unravel_index(i, (len(c.boxes), S, S, 3))
    return b, ch, dy, dx


def check(lib, c, fmt, buf):
    """an output buffer of new_buffer's shape after one call -> list of failures (empty: every bit as expected)
      live crops        every element has the bits of the reference (float32, or its one further rounding to the 16-bit format)
      degenerate crops  every element is zero
      the tail          still the sentinel
      all-255 mask      in float32 also rint(out * 255) == resize_lanczos4_u8
    A failure names the crop, the count and first position of its mismatches, the tile and the path that tile takes."""
    buf = np.asarray(buf)
    n = n_elements(c)
    if buf.dtype != BITS_DTYPE[fmt] or buf.shape != (n + 3 * c.S * c.S,):
        return [f"{c.name} {fmt}: buffer {buf.dtype} {buf.shape}"]
    fails = []
    tail = np.nonzero(buf[n:] != SENTINEL[fmt])[0]
    if tail.size:
        fails.append(f"{c.name} {fmt}: {tail.size} elements behind the last crop overwritten, first at offset {int(tail[0])}")
    bad = np.nonzero(buf[:n] != reference_bits(c, fmt))[0]
    if bad.size:
        T = lib.crop_tile()
        paths = tile_paths(lib, c)
        b, ch, dy, dx = _where(c, fmt, bad)
        for k in np.unique(b):
            sel = np.nonzero(b == k)[0]
            j = sel[0]
            box = c.boxes[k].tolist()
            if paths[k] is None:
                what = "degenerate box, zeros expected"
            else:
                sep = np.array([s for _, s in paths[k]])[dy[sel] // T]
                R, s0 = paths[k][dy[j] // T]
                what = (f"tile ({dy[j] // T}, {dx[j] // T}) of {R} rows on the {'separable' if s0 else 'direct'} path; "
                        f"{int(sep.sum())} mismatches on the separable path, {int((~sep).sum())} on the direct path")
            fails.append(f"{c.name} {fmt}: crop {k} {box}: {sel.size} mismatching elements, first at channel {ch[j]} dy {dy[j]} dx {dx[j]}: "
                         f"{int(buf[bad[j]]):#x} for {int(reference_bits(c, fmt)[bad[j]]):#x}; {what}")
    if fmt == "f32" and (c.mask == 255).all():
        got = np.rint(buf[:n].view(np.float32).reshape(-1, 3, c.S, c.S).astype(np.float64) * 255)
        d = np.nonzero(got != reference_u8(c))
        if d[0].size:
            fails.append(f"{c.name} f32: {d[0].size} elements differ from resize_lanczos4_u8 under an all-255 mask, first at {[int(v[0]) for v in d]}")
    return fails
