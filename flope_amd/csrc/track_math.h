// The arithmetic of the device tracker (track.hip: track_assoc_kernel, track_apply_kernel), in ONE place and without HIP: a pose
// to a measurement, the distance to an anchor, the order of two (distance, index) candidates, one filter update.  The kernels take
// all four from here and keep only their lanes, strides and prefix counts; tests/host_harness/harness_track.cpp compiles the same
// definitions for the CPU tests (tests/track_cases.py, tests/test_track_host.py).  DESIGN.md 45.
//
// The operation is FlowerModel.assign_meas_to_state (sunflower/predictor/flower_model.py): world pose = camera pose x flower pose,
// measurement = [translation | scalar-last quaternion], nearest ANCHOR (a track's first measurement) under a gate, and per track
// the 7-state identity-model Kalman filter, which is one scalar recursion for all seven components because F = H = I and P, Q, R
// are multiples of I (oracle/fusion_ref.py):   p += q;  k = p / (p + r);  x += k (z - x);  p = (1 - k)^2 p + k^2 r.
//
// Everything is float64 and every operation below is ONE rounding, in the order written: contraction into fused multiply-adds is
// switched off inside each function, so that the device code, the host compile and the count of roundings in tests/track_bound.py
// speak of the same thing.
#pragma once
#include <math.h>

#ifndef TRACK_HD
#if defined(__HIPCC__)
#define TRACK_HD __host__ __device__
#else
#define TRACK_HD
#endif
#endif

#if defined(__clang__)
#define TRACK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TRACK_NO_CONTRACT            /* g++ for x86-64 without -mfma has no fused multiply-add to contract into */
#endif

constexpr int kTrackDim = 7;         // [x y z | qx qy qz qw]

// the quaternion (not yet normalised) of the rotation in W's 3x3 when diagonal entry I is the largest of (R00, R11, R22, trace);
// I is a template argument so that every index is a constant (registers, not scratch memory, in the kernel)
template <int I>
TRACK_HD inline void track_quat_diagonal(const double W[12], double tr, double q[4]) {
  TRACK_NO_CONTRACT
  constexpr int i = I, j = (i + 1) % 3, k = (j + 1) % 3;
  q[i] = (1.0 - tr) + 2.0 * W[i * 4 + i];
  q[j] = W[j * 4 + i] + W[i * 4 + j];
  q[k] = W[k * 4 + i] + W[i * 4 + k];
  q[3] = W[k * 4 + j] - W[j * 4 + k];
}

// row-major 4x4 pose (P) in the camera frame and the camera pose C -> z[7].  W = C P by a fixed k = 0..3 chain per element (four
// products, three sums), top three rows only; translation = W[:3,3]; quaternion of W[:3,:3] by the largest of (R00, R11, R22,
// trace), the first maximum in that order, then divided by its norm.  The rule only normalises: a matrix that is not orthogonal is
// not moved onto a rotation first.
TRACK_HD inline void track_measure(const double P[16], const double C[16], double z[kTrackDim]) {
  TRACK_NO_CONTRACT
  double W[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double acc = C[i * 4] * P[j];
      for (int k = 1; k < 4; ++k) acc = acc + C[i * 4 + k] * P[k * 4 + j];
      W[i * 4 + j] = acc;
    }
  z[0] = W[3]; z[1] = W[7]; z[2] = W[11];
  const double tr = (W[0] + W[5]) + W[10];
  const double dec[4] = {W[0], W[5], W[10], tr};
  int c = 0;
  for (int m = 1; m < 4; ++m) if (dec[m] > dec[c]) c = m;
  double q[4];
  if (c == 0) {
    track_quat_diagonal<0>(W, tr, q);
  } else if (c == 1) {
    track_quat_diagonal<1>(W, tr, q);
  } else if (c == 2) {
    track_quat_diagonal<2>(W, tr, q);
  } else {
    q[0] = W[9] - W[6];
    q[1] = W[2] - W[8];
    q[2] = W[4] - W[1];
    q[3] = 1.0 + tr;
  }
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int m = 0; m < 4; ++m) z[3 + m] = q[m] / n;
}

// distance of a measurement's translation to an anchor's
TRACK_HD inline double track_dist(const double* z, const double* a) {
  TRACK_NO_CONTRACT
  const double dx = z[0] - a[0], dy = z[1] - a[1], dz = z[2] - a[2];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// does candidate (d, i) come before (bd, bi)?  The nearer one, and among equal distances the lower index (np.argmin), whatever
// order the candidates are met in.  A NaN distance never comes first.
TRACK_HD inline bool track_better(double d, int i, double bd, int bi) { return d < bd || (d == bd && i < bi); }

// the match test on the winner of track_better over all anchors (bi < 0: there was no anchor)
TRACK_HD inline bool track_match(double bd, int bi, double th) { return bi >= 0 && bd < th; }

// one predict + update of a track on measurement z, then the quaternion part divided by its norm
TRACK_HD inline void track_filter_update(double x[kTrackDim], double* p, const double z[kTrackDim], double q, double r) {
  TRACK_NO_CONTRACT
  const double pp = *p + q;
  const double k = pp / (pp + r);
  for (int c = 0; c < kTrackDim; ++c) x[c] = x[c] + k * (z[c] - x[c]);
  const double a = 1.0 - k;
  *p = (a * a) * pp + (k * k) * r;
  const double n = sqrt(((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) + x[6] * x[6]);
  for (int c = 3; c < kTrackDim; ++c) x[c] = x[c] / n;
}

// association entries (flope_track_read_assoc): >= 0 matched track, -1 - t opened track t, kTrackSkipped unreliable row
constexpr int kTrackSkipped = -2147483647 - 1;
constexpr int kTrackUnmatched = -1;          // between the two kernels only: "opens a track", before the index is known
