// The strip plan of the depth statistics kernel (prep.hip: depth_box_kernel / depth_box_final_kernel, flope_depth_lift), in ONE
// place and without HIP: how a box is clamped to the frame, which rows each of its strips owns, which rectangle of validity bits a
// strip needs around them, whether that rectangle is kept as an LDS tile, where the strip partials lie in the scratch buffer, and
// the rows of the erosion element.  The kernel takes all of it from here; tests/host_harness/harness_depth.cpp exports the same
// functions to the CPU tests (tests/test_depth_cases.py), which build their edge cases from the plan instead of from a copy of it.
//
// The operation (image_manipulation.py:39-96): valid = (near < d < far) & (mask > 128), eroded by cv2's 10 x 10 MORPH_ELLIPSE with
// anchor (5, 5) -- a pixel survives when every tap (y + ey - 5, x + ex - 5), ex in [lo(ey), hi(ey)], is valid or outside the frame
// (erode's default border is +inf) -- then the mean of the surviving depths inside the box.
#pragma once

#include <stddef.h>

#ifndef DEPTH_HD
#if defined(__HIPCC__)
#define DEPTH_HD __host__ __device__
#else
#define DEPTH_HD
#endif
#endif

constexpr int kDepthStrips = 32;           // horizontal strips per box, one workgroup each; partials are combined in strip order
constexpr int kDepthLds = 48 * 1024;       // bytes of LDS for one strip's validity tile; a larger tile is not built (untiled path)
constexpr int kDepthMinCount = 50;         // reliable = count >= kDepthMinCount

// Element rows (OpenCV getStructuringElement: dx = round(c * sqrt(1 - dy^2/r^2)), r = c = 5):
//   ey: 0 -> col 5 | 1,9 -> 2..8 | 2,8 -> 1..9 | 3..7 -> 0..9        1 + 7 + 9 + 5 * 10 + 9 + 7 = 83 taps
constexpr int kDepthElem = 10;             // the element is kDepthElem x kDepthElem
constexpr int kDepthAnchor = 5;            // taps reach kDepthAnchor rows / columns back and kDepthElem - 1 - kDepthAnchor forward
#define DEPTH_ELLIPSE_LO {5, 2, 1, 0, 0, 0, 0, 0, 1, 2}
#define DEPTH_ELLIPSE_HI {5, 8, 9, 9, 9, 9, 9, 9, 9, 8}
constexpr int kDepthEllipseLo[kDepthElem] = DEPTH_ELLIPSE_LO;
constexpr int kDepthEllipseHi[kDepthElem] = DEPTH_ELLIPSE_HI;

constexpr int depth_ellipse_taps() {
  int n = 0;
  for (int ey = 0; ey < kDepthElem; ++ey) n += kDepthEllipseHi[ey] - kDepthEllipseLo[ey] + 1;
  return n;
}
static_assert(depth_ellipse_taps() == 83, "cv2.getStructuringElement(MORPH_ELLIPSE, (10, 10)) has 83 taps");

// numpy slicing semantics of depth[y0:y1, x0:x1] for non-negative boxes: the far edges clamp to the frame, an empty or inverted
// range selects nothing
struct DepthExtent { int xs, ys, xe, ye, bw, bh; };
DEPTH_HD inline DepthExtent depth_box_extent(int x0, int y0, int x1, int y1, int FH, int FW) {
  DepthExtent e;
  e.xs = x0 > 0 ? x0 : 0; e.ys = y0 > 0 ? y0 : 0;
  e.xe = x1 < FW ? x1 : FW; e.ye = y1 < FH ? y1 : FH;
  e.bw = e.xe - e.xs > 0 ? e.xe - e.xs : 0; e.bh = e.ye - e.ys > 0 ? e.ye - e.ys : 0;
  return e;
}

// strip s owns the box rows r0 <= r < r1 (relative to ys); r1 of a strip is r0 of the next, a box lower than kDepthStrips rows
// has empty strips
struct DepthRows { int r0, r1; };
DEPTH_HD inline DepthRows depth_strip_rows(int bh, int s) {
  DepthRows r;
  r.r0 = (int)((long)bh * s / kDepthStrips);
  r.r1 = (int)((long)bh * (s + 1) / kDepthStrips);
  return r;
}

// validity of a strip and of everything its taps reach: frame rows ys + r0 - 5 .. ys + r1 + 3, columns xs - 5 .. xe + 3
DEPTH_HD inline int depth_tile_w(int bw) { return bw + kDepthElem - 1; }
DEPTH_HD inline int depth_tile_h(int nr) { return nr + kDepthElem - 1; }

// the tile is built (one byte per pixel) when the strip is not empty and the tile fits; otherwise each tap is re-derived from the
// inputs
DEPTH_HD inline bool depth_strip_is_tiled(int bw, int nr) {
  return nr > 0 && bw > 0 && (long)depth_tile_w(bw) * depth_tile_h(nr) <= kDepthLds;
}

// scratch of flope_depth_lift: [H*W bytes, unused since the validity map became an LDS tile][16-byte aligned partials, 16 bytes per
// strip]; include/flope_amd.h asks the caller for H*W + 16 + 512*n bytes
constexpr int kDepthPartialBytes = 16;
DEPTH_HD inline size_t depth_partials_offset(size_t npix) { return (npix + 15) & ~(size_t)15; }
DEPTH_HD inline size_t depth_scratch_needed(size_t npix, size_t n) {
  return depth_partials_offset(npix) + n * kDepthStrips * kDepthPartialBytes;
}
