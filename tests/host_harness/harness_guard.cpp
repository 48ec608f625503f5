// CPU-only test harness of the guarded mode (flope_amd/csrc/guard.hip): the conditioning figure and the flag predicate of
// pose_math.h, the code the select kernel runs per crop (tests/test_guard_host.py).  Not part of the product.
#include "pose_math.h"

extern "C" {

// gap(M) of n row-major 3x3 matrices
void guard_gap(const float* M, int n, float* out) {
  for (int i = 0; i < n; ++i) out[i] = procrustes_gap3x3(M + (long)i * 9);
}

// 1: the crop would be repaired
int guard_flagged(float gap, float gap_min) { return procrustes_gap_flagged(gap, gap_min) ? 1 : 0; }

}  // extern "C"
