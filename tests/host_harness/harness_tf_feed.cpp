// CPU-only test harness of the feed rule of a device-positioned stream state (flope_amd/csrc/tf_stream_feed.h, which
// tf_stream_feed_kernel calls per thread): the rule over host arrays in ascending or descending row order (it needs no
// order), the token row, and track_measure of flope_amd/csrc/track_math.h, so that the GPU tests have the expected token bits.
// `broken` selects copies that are wrong the way the kernel can be wrong; tests/test_tf_feed_host.py shows that the cases of
// tests/track_stream_cases.py notice each.  Not part of the product.
// With -DTF_FEED_MAIN the file is a program of its own (built under -fsanitize=address,undefined by the test and run as a child
// process): random associations in arrays of exactly n, tracks and 2 n elements, both row orders against each other.
#include <stdint.h>
#include <vector>
#include "tf_stream_feed.h"
#include "track_math.h"

using namespace flope_tf_plan;

enum { BROKEN_LAST_WINS = 1, BROKEN_DUP_ADVANCES = 2, BROKEN_OPENED_NEG = 4, BROKEN_FULL_FED = 8 };

namespace {
// the rule restated with its faults; broken = 0 is never routed here
int broken_row(const int* assoc, int m, int n, int overflow, int tracks, int* pos, int* tab, int broken) {
  int t;
  if (overflow) t = FLOPE_TF_FEED_OVERFLOW;
  else if (assoc[m] == kTfFeedSkippedAssoc) t = FLOPE_TF_FEED_SKIPPED;
  else {
    const auto track_of = [&](int a) { return (broken & BROKEN_OPENED_NEG) ? (a >= 0 ? a : -a) : tf_feed_track(a); };
    t = track_of(assoc[m]);
    if (t >= tracks) t = FLOPE_TF_FEED_RANGE;
    else {
      bool dup = false;
      const int e0 = (broken & BROKEN_LAST_WINS) ? m + 1 : 0, e1 = (broken & BROKEN_LAST_WINS) ? n : m;
      for (int e = e0; e < e1 && !dup; ++e) dup = assoc[e] != kTfFeedSkippedAssoc && track_of(assoc[e]) == t;
      if (dup) {
        if ((broken & BROKEN_DUP_ADVANCES) && pos[t] != INT_MAX) ++pos[t];
        t = FLOPE_TF_FEED_DUPLICATE;
      } else if (pos[t] == INT_MAX && !(broken & BROKEN_FULL_FED)) t = FLOPE_TF_FEED_FULL;
    }
  }
  if (t >= 0) {
    const int p = pos[t];
    tab[2 * m] = t; tab[2 * m + 1] = p;
    pos[t] = p == INT_MAX ? INT_MAX : p + 1;              // (the faulty copy must not itself overflow an int)
  } else {
    tab[2 * m] = t; tab[2 * m + 1] = 0;
  }
  return t;
}
}  // namespace

extern "C" {

int tf_feed_codes(int* out5) {
  out5[0] = FLOPE_TF_FEED_SKIPPED; out5[1] = FLOPE_TF_FEED_OVERFLOW; out5[2] = FLOPE_TF_FEED_RANGE; out5[3] = FLOPE_TF_FEED_DUPLICATE;
  out5[4] = FLOPE_TF_FEED_FULL;
  return kTfFeedSkippedAssoc == kTrackSkipped && kTfFeedDim == kTrackDim ? 0 : -1;
}
int tf_feed_h_track(int a) { return tf_feed_track(a); }
int tf_feed_h_decide(const int* assoc, int m, int overflow, int tracks, const int* pos) { return tf_feed_decide(assoc, m, overflow, tracks, pos); }

// One frame over host arrays: assoc [n], pos [tracks] (updated), tab [2 n].  descending != 0: the rows from the last one down.  Returns
// the number of rows that fed.
int tf_feed_walk(const int* assoc, int n, int overflow, int tracks, int* pos, int* tab, int descending, int broken) {
  int fed = 0;
  for (int i = 0; i < n; ++i) {
    const int m = descending ? n - 1 - i : i;
    fed += (broken ? broken_row(assoc, m, n, overflow, tracks, pos, tab, broken) : tf_feed_row(assoc, m, overflow, tracks, pos, tab)) >= 0;
  }
  return fed;
}

// z: float64 [7], or NULL for a row that feeds nothing -> row float32 [input_dim]
void tf_feed_h_token(const double* z, int input_dim, float* row) { tf_feed_token(z, input_dim, row); }

// track_measure: pose row-major 4x4, float32 (f64 = 0, widened exactly) or float64; cam16 row-major 4x4 -> z float64 [7]
void tf_feed_h_measure(const void* pose, int f64, const double* cam16, double* z) {
  double P[16];
  for (int e = 0; e < 16; ++e) P[e] = f64 ? ((const double*)pose)[e] : (double)((const float*)pose)[e];
  track_measure(P, cam16, z);
}

}  // extern "C"

#ifdef TF_FEED_MAIN
#include <stdio.h>
namespace {
uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t next() {                                          // xorshift64*
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545f4914f6cdd1dull) >> 32);
}
}  // namespace

int main() {
  int frames = 0, failures = 0;
  for (int round = 0; round < 400; ++round) {
    const int tracks = 1 + (int)(next() % 40), n = (int)(next() % 70);
    // exactly tracks, n and 2 n elements: the sanitizer sees an access behind the last one
    std::vector<int> pos(tracks), assoc(n), ta(2 * (size_t)n), tb(2 * (size_t)n);
    for (int t = 0; t < tracks; ++t) pos[t] = next() % 5 == 0 ? INT_MAX - (int)(next() % 2) : (int)(next() % 1000);
    for (int m = 0; m < n; ++m) {
      const int t = (int)(next() % (tracks + 3));
      const uint32_t k = next() % 8;
      assoc[m] = k == 0 ? kTfFeedSkippedAssoc : k < 4 ? -1 - t : t;
    }
    const int overflow = next() % 9 == 0;
    std::vector<int> pa = pos, pb = pos;
    const int fa = tf_feed_walk(assoc.data(), n, overflow, tracks, pa.data(), ta.data(), 0, 0);
    const int fb = tf_feed_walk(assoc.data(), n, overflow, tracks, pb.data(), tb.data(), 1, 0);
    ++frames;
    if (fa != fb || pa != pb || ta != tb) ++failures;
    long moved = 0;
    for (int t = 0; t < tracks; ++t) { moved += (long)pa[t] - pos[t]; if (pa[t] - pos[t] < 0 || pa[t] - pos[t] > 1) ++failures; }
    if (moved != fa || (overflow && fa)) ++failures;
    float row[12];
    const double z[7] = {0.1, -0.2, 0.3, 0.5, 0.5, -0.5, 0.5};
    tf_feed_h_token(n % 2 ? z : nullptr, 7 + n % 6, row);
  }
  printf("%d frames, %d failures\n", frames, failures);
  return failures ? 1 : 0;
}
#endif
