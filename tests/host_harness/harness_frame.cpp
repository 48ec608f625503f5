// CPU-only test harness of the box selection's arithmetic (flope_amd/csrc/frame_plan.h, the header frame.hip's
// frame_select_kernel takes its count clamp and its per-row decision from): tests/frame_cases.py and tests/test_frame_cases.py
// compare these answers with the two Python statements of the reference's loop.  Not part of the product.
#include "frame_plan.h"

extern "C" {

int frame_det_row() { return kFrameDetRow; }

// rows the kernel reads for a detector count of `count` and a table of max_det rows
int frame_count_rows(int count, int max_det) { return frame_count(count, max_det); }

// frame_box over n detector rows of kFrameDetRow floats each: keep[i] (0 / 1), good[i][4], sq[i][4] of every row, kept or not
void frame_boxes(const float* det, int n, int W, int H, int* keep, int* good, int* sq) {
  for (int i = 0; i < n; ++i) keep[i] = frame_box(det + (long)i * kFrameDetRow, W, H, good + (long)i * 4, sq + (long)i * 4) ? 1 : 0;
}

}  // extern "C"
