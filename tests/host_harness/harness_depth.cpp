// CPU-only test harness of the depth statistics kernel's strip plan (flope_amd/csrc/depth_plan.h, the header prep.hip's
// depth_box_kernel takes its geometry from): tests/depth_cases.py builds its edge cases from these answers and
// tests/test_depth_cases.py checks them.  Not part of the product.
#include "depth_plan.h"

extern "C" {

int depth_strips() { return kDepthStrips; }
int depth_lds() { return kDepthLds; }
int depth_min_count() { return kDepthMinCount; }
int depth_taps() { return depth_ellipse_taps(); }

// the element: first and last column of each of its 10 rows, and the anchor
int depth_ellipse(int* lo, int* hi) {
  for (int ey = 0; ey < kDepthElem; ++ey) { lo[ey] = kDepthEllipseLo[ey]; hi[ey] = kDepthEllipseHi[ey]; }
  return kDepthAnchor;
}

// box = {x0, y0, x1, y1} in a frame of FH x FW -> out = {xs, ys, xe, ye, bw, bh}
void depth_extent(const int* box, int FH, int FW, int* out) {
  const DepthExtent e = depth_box_extent(box[0], box[1], box[2], box[3], FH, FW);
  out[0] = e.xs; out[1] = e.ys; out[2] = e.xe; out[3] = e.ye; out[4] = e.bw; out[5] = e.bh;
}

// per strip of the box: its rows [r0, r1) relative to ys, whether its validity tile is built, and the tile's frame rectangle
// tile[s] = {first row, first column, rows, columns} (stated for untiled strips too: it is what their taps reach)
void depth_plan(const int* box, int FH, int FW, int* r0, int* r1, int* tiled, int* tile) {
  const DepthExtent e = depth_box_extent(box[0], box[1], box[2], box[3], FH, FW);
  for (int s = 0; s < kDepthStrips; ++s) {
    const DepthRows r = depth_strip_rows(e.bh, s);
    r0[s] = r.r0; r1[s] = r.r1;
    tiled[s] = depth_strip_is_tiled(e.bw, r.r1 - r.r0) ? 1 : 0;
    tile[s * 4] = e.ys + r.r0 - kDepthAnchor; tile[s * 4 + 1] = e.xs - kDepthAnchor;
    tile[s * 4 + 2] = depth_tile_h(r.r1 - r.r0); tile[s * 4 + 3] = depth_tile_w(e.bw);
  }
}

// where the strip partials start in the scratch buffer and where they end, for a frame of npix pixels and n boxes
long depth_partials_begin(long npix) { return (long)depth_partials_offset((size_t)npix); }
long depth_partials_end(long npix, long n) { return (long)depth_scratch_needed((size_t)npix, (size_t)n); }

}  // extern "C"
