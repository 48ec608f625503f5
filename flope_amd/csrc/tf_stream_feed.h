// The feed rule of a device-positioned stream state (flope_tf_stream_open_device, flope_tf_stream_step_assoc / _step_tracker; DESIGN.md
// 46), in ONE place and without HIP: which rows of a frame's association (the device tracker's encoding, track_math.h) feed their
// track one token, the table entry and the position each writes, and the float32 token row.  tf_stream_feed_kernel (tf_encoder.hip)
// calls these per thread; tests/host_harness/harness_tf_feed.cpp compiles the same definitions for the CPU tests
// (tests/track_stream_cases.py, tests/test_tf_feed_host.py).  Plain integer code, in the way track_math.h is.
//
// Row m of a frame has association a: a >= 0 names the matched track a, a < 0 the opened track -1 - a, INT32_MIN a row the tracker
// skipped.  Row m FEEDS its track iff the tracker's overflow flag is clear, the row was not skipped, the track is one of the
// stream's, no row e < m names the same track (the first measurement in measurement order is the frame's token) and the track's
// position is below INT_MAX.  A feeding row writes (track, pos[track]) into the table and pos[track] + 1 back; every other row writes
// (code, 0) and moves nothing.  No two feeding rows name one track and a row reads pos[] only for a track it feeds, so the rows may
// run in any order, or all at once: one thread per row, no atomics.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/flope_amd.h"

#ifndef TF_FEED_HD
#if defined(__HIPCC__)
#define TF_FEED_HD __host__ __device__
#else
#define TF_FEED_HD
#endif
#endif

namespace flope_tf_plan {

constexpr int kTfFeedSkippedAssoc = INT_MIN;        // track_math.h: kTrackSkipped
constexpr int kTfFeedDim = 7;                       // track_math.h: kTrackDim, [x y z | qx qy qz qw]

// the track an association entry names (not for the skipped value); -1 - a cannot overflow: a >= INT_MIN + 1 there
TF_FEED_HD inline int tf_feed_track(int a) { return a >= 0 ? a : -1 - a; }

// does row e of the frame name `track`?
TF_FEED_HD inline bool tf_feed_names(const int* assoc, int e, int track) {
  return assoc[e] != kTfFeedSkippedAssoc && tf_feed_track(assoc[e]) == track;
}

// The track row m feeds (>= 0), or the FLOPE_TF_FEED_* code (< 0) of the first test it fails, in this order: overflow, skipped, range,
// duplicate, full.  Under the overflow flag the association is what an earlier frame left and is not read at all; pos[] is read
// only for the track of a row that passed every other test.
TF_FEED_HD inline int tf_feed_decide(const int* assoc, int m, int overflow, int tracks, const int* pos) {
  if (overflow) return FLOPE_TF_FEED_OVERFLOW;
  const int a = assoc[m];
  if (a == kTfFeedSkippedAssoc) return FLOPE_TF_FEED_SKIPPED;
  const int track = tf_feed_track(a);
  if (track >= tracks) return FLOPE_TF_FEED_RANGE;
  for (int e = 0; e < m; ++e)
    if (tf_feed_names(assoc, e, track)) return FLOPE_TF_FEED_DUPLICATE;
  if (pos[track] == INT_MAX) return FLOPE_TF_FEED_FULL;
  return track;
}

// ... and what it writes: the table entry tab[2 m], tab[2 m + 1] and, where it feeds, the track's position.  -> the decision
TF_FEED_HD inline int tf_feed_row(const int* assoc, int m, int overflow, int tracks, int* pos, int* tab) {
  const int t = tf_feed_decide(assoc, m, overflow, tracks, pos);
  if (t >= 0) {
    const int p = pos[t];
    tab[2 * m] = t;
    tab[2 * m + 1] = p;
    pos[t] = p + 1;
  } else {
    tab[2 * m] = t;
    tab[2 * m + 1] = 0;
  }
  return t;
}

// The token row of a row that feeds from a tracker's 7-vector z (a measurement or a filtered mean): each component rounded once to
// float32, zeros behind them up to input_dim (>= kTfFeedDim).  z == nullptr: a row that feeds nothing, all zero.
TF_FEED_HD inline void tf_feed_token(const double* z, int input_dim, float* row) {
  for (int c = 0; c < input_dim; ++c) row[c] = z && c < kTfFeedDim ? (float)z[c] : 0.f;
}

}  // namespace flope_tf_plan
