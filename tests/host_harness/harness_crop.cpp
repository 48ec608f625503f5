// CPU-only test harness of the crop + Lanczos-4 resize kernel's tile plan (flope_amd/csrc/crop_plan.h, the header prep.hip's
// crop_resize_mask_tiled_kernel takes its tile edge, its LDS window and its path rule from): tests/crop_cases.py places its edge
// cases from these answers and tests/test_crop_cases.py checks them.  Not part of the product.
#include "crop_plan.h"

extern "C" {

int crop_tile() { return kCropTile; }
int crop_rows_limit() { return kCropRows; }
int crop_taps() { return kCropTaps; }
int crop_taps_back() { return kCropTapsBack; }
int crop_tile_count(int S) { return crop_tiles(S); }

// first (unclamped) source row of a tile from the first-tap position of its first output row
int crop_first_row(int s_first) { return crop_tile_first_row(s_first); }

// source rows a tile touches from the first-tap positions of its first and sixteenth output row
int crop_rows(int s_first, int s_sixteenth) { return crop_tile_rows(s_first, s_sixteenth); }

// 1: separable LDS path, 0: direct 8 x 8 sum
int crop_separable(int rows) { return crop_tile_is_separable(rows) ? 1 : 0; }

}  // extern "C"
