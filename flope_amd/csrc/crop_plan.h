// The tile plan of the crop + Lanczos-4 resize kernel (prep.hip: crop_resize_mask_tiled_kernel, flope_crop_resize_mask), in ONE
// place and without HIP: the edge of an output tile, how many source rows a tile touches, and which of the kernel's two paths the
// tile takes.  The kernel takes all of it from here; tests/host_harness/harness_crop.cpp exports the same functions to the CPU
// tests (tests/crop_cases.py, tests/test_crop_cases.py), which place their edge cases from the rule instead of from a copy of it.
//
// One workgroup computes one kCropTile x kCropTile output tile of one crop.  Output row dy of an axis resized n_src -> S has its
// eight taps at the source rows s(dy) - 3 .. s(dy) + 4 (s = the first-tap position lanczos4_axis returns; clamped to the crop when
// read).  The tile's source window runs from the first tap of its first output row to the last tap of its SIXTEENTH output row,
// whether or not that row exists: in the ragged last tile of an S that is no multiple of kCropTile the sixteenth row is a phantom
// (dy >= S) whose s is still evaluated, so the window -- and with it the path -- of such a tile is decided by a row that is never
// written.  A window of at most kCropRows rows is filtered horizontally into LDS once and then vertically (separable path); a
// larger one (down-scaling by more than about 3.5x) is summed directly, 8 x 8 taps per output pixel.  Both paths add the same
// integers, so the choice moves no bit of the result.
#pragma once

#ifndef CROP_HD
#if defined(__HIPCC__)
#define CROP_HD __host__ __device__
#else
#define CROP_HD
#endif
#endif

constexpr int kCropTile = 16;              // output tile edge; a workgroup has kCropTile * kCropTile threads
constexpr int kCropRows = 64;              // source rows of the LDS window of the separable path
constexpr int kCropTaps = 8;               // Lanczos-4: taps s - kCropTapsBack .. s + kCropTaps - 1 - kCropTapsBack
constexpr int kCropTapsBack = 3;

CROP_HD inline int crop_tiles(int S) { return (S + kCropTile - 1) / kCropTile; }

// first (unclamped, possibly negative) source row of a tile whose first output row has first-tap position s_first
CROP_HD inline int crop_tile_first_row(int s_first) { return s_first - kCropTapsBack; }

// source rows a tile touches, given the first-tap positions of its first and of its sixteenth output row
CROP_HD inline int crop_tile_rows(int s_first, int s_sixteenth) {
  return s_sixteenth + (kCropTaps - 1 - kCropTapsBack) - crop_tile_first_row(s_first) + 1;
}

// the separable LDS path when the window fits, the direct 8 x 8 sum otherwise
CROP_HD inline bool crop_tile_is_separable(int rows) { return rows <= kCropRows; }
