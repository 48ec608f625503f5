// CPU-only test harness of the device tracker (flope_amd/csrc/track.hip): the functions of flope_amd/csrc/track_math.h, which
// the kernels call, and a scalar walk of a whole update -- association against the anchors of the start of the frame (the lanes'
// strided argmin and the pair reduction restated with a `lanes` parameter), the overflow rule, the appends in measurement order,
// the ordered updates of each track -- over host arrays, every index checked.  `broken` selects copies that are wrong the way the
// kernels can be wrong; tests/test_track_host.py shows that the cases notice each.  Not part of the product.
// With -DTRACK_MAIN the file is a program of its own (built under -fsanitize=address,undefined by the test and run as a child
// process): random frames through the walk at 1 and 64 lanes, overflow, and the sentinel words behind every array.
#include <stdint.h>
#include <vector>
#include "track_math.h"

enum { BROKEN_REVERSE = 1, BROKEN_MEANS = 2, BROKEN_VISIBLE = 4, BROKEN_TIE_HIGH = 8 };

extern "C" {

int track_dim() { return kTrackDim; }
int track_skipped() { return kTrackSkipped; }

// pose: row-major 4x4, float32 (f64 = 0, widened exactly) or float64
void track_h_measure(const void* pose, int f64, const double* cam16, double* z) {
  double P[16];
  for (int e = 0; e < 16; ++e) P[e] = f64 ? ((const double*)pose)[e] : (double)((const float*)pose)[e];
  track_measure(P, cam16, z);
}

double track_h_dist(const double* z, const double* a) { return track_dist(z, a); }
int track_h_better(double d, int i, double bd, int bi) { return track_better(d, i, bd, bi) ? 1 : 0; }
int track_h_match(double bd, int bi, double th) { return track_match(bd, bi, th) ? 1 : 0; }
void track_h_update(double* x, double* p, const double* z, double q, double r) { track_filter_update(x, p, z, q, r); }

// One update over host arrays: anchors / means [max_tracks][7], p / hits [max_tracks], count[2] = {tracks, overflow flag},
// assoc [max_meas].  Returns 0, or -(line) of the index check that failed (nothing may be read or written outside the arrays).
#define TRACK_CHECK(i, limit) do { if ((long)(i) < 0 || (long)(i) >= (long)(limit)) return -__LINE__; } while (0)
int track_walk(const void* Rt, int rt_f64, const int32_t* rel, int n, const double* cam16, double* anchors, double* means, double* p,
               int32_t* hits, int32_t* count, int32_t* assoc, int max_tracks, int max_meas, double th, double q, double r, double p0,
               int lanes, int broken) {
  if (n < 0 || n > max_meas || lanes < 1) return -__LINE__;
  if (n == 0) return 0;
  const int T0 = count[0];
  TRACK_CHECK(T0, max_tracks + 1);
  std::vector<double> meas((size_t)n * kTrackDim);
  std::vector<int> cand(n);
  int visible = T0;                                    // BROKEN_VISIBLE only: anchors a measurement sees, tracks of its own frame included
  for (int m = 0; m < n; ++m) {
    if (rel && rel[m] == 0) { cand[m] = kTrackSkipped; continue; }
    double* z = &meas[(size_t)m * kTrackDim];
    track_h_measure((const char*)Rt + (size_t)m * 16 * (rt_f64 ? 8 : 4), rt_f64, cam16, z);
    const double* ref = (broken & BROKEN_MEANS) ? means : anchors;
    const int T = (broken & BROKEN_VISIBLE) ? visible : T0;
    std::vector<double> bd(lanes, INFINITY);
    std::vector<int> bi(lanes, -1);
    for (int lane = 0; lane < lanes; ++lane)
      for (int t = lane; t < T; t += lanes) {
        TRACK_CHECK(t, max_tracks);
        const double d = track_dist(z, ref + (size_t)t * kTrackDim);
        const bool better = (broken & BROKEN_TIE_HIGH) ? (d < bd[lane] || (d == bd[lane] && t > bi[lane])) : track_better(d, t, bd[lane], bi[lane]);
        if (better) { bd[lane] = d; bi[lane] = t; }
      }
    // the pair reduction, from the highest lane down: the answer must not depend on the order the lanes are met in
    double wd = INFINITY;
    int wi = -1;
    for (int lane = lanes - 1; lane >= 0; --lane) {
      const bool better = (broken & BROKEN_TIE_HIGH) ? (bd[lane] < wd || (bd[lane] == wd && bi[lane] > wi)) : track_better(bd[lane], bi[lane], wd, wi);
      if (better) { wd = bd[lane]; wi = bi[lane]; }
    }
    cand[m] = track_match(wd, wi, th) ? wi : kTrackUnmatched;
    if ((broken & BROKEN_VISIBLE) && cand[m] == kTrackUnmatched && visible < max_tracks) {
      for (int e = 0; e < kTrackDim; ++e) anchors[(size_t)visible * kTrackDim + e] = means[(size_t)visible * kTrackDim + e] = z[e];
      ++visible;
    }
  }
  if (count[1] != 0) return 0;                         // sticky: nothing is applied until the reset
  int fresh = 0;
  for (int m = 0; m < n; ++m) fresh += cand[m] == kTrackUnmatched;
  if (fresh > max_tracks - T0) { count[1] = 1; return 0; }
  int opened = 0;
  for (int m = 0; m < n; ++m) {
    TRACK_CHECK(m, max_meas);
    const int c = cand[m];
    if (c == kTrackSkipped) { assoc[m] = kTrackSkipped; continue; }
    if (c == kTrackUnmatched) {
      const int t = T0 + opened++;
      TRACK_CHECK(t, max_tracks);
      for (int e = 0; e < kTrackDim; ++e) anchors[(size_t)t * kTrackDim + e] = means[(size_t)t * kTrackDim + e] = meas[(size_t)m * kTrackDim + e];
      p[t] = p0;
      hits[t] = 1;
      assoc[m] = -1 - t;
      continue;
    }
    // a track opened in this frame can only be matched by the broken copy that makes it visible; it then has no filter yet
    TRACK_CHECK(c, (broken & BROKEN_VISIBLE) ? max_tracks : T0);
    assoc[m] = c;
    bool first = true;
    for (int e = 0; e < m && first; ++e) first = cand[e] != c;
    if (!first || c >= T0) continue;
    std::vector<int> mine;
    for (int mm = m; mm < n; ++mm) if (cand[mm] == c) mine.push_back(mm);
    for (size_t u = 0; u < mine.size(); ++u) {
      const int mm = (broken & BROKEN_REVERSE) ? mine[mine.size() - 1 - u] : mine[u];
      track_filter_update(means + (size_t)c * kTrackDim, p + c, &meas[(size_t)mm * kTrackDim], q, r);
      ++hits[c];
    }
  }
  count[0] = T0 + fresh;
  return 0;
}

}  // extern "C"

#ifdef TRACK_MAIN
#include <stdio.h>
#include <string.h>
namespace {
uint64_t g_rng = 0x9e3779b97f4a7c15ull;
double uniform() {                                     // xorshift64*, in [0, 1)
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (double)((g_rng * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}
struct State {
  int T, M;
  std::vector<double> anchors, means, p;
  std::vector<int32_t> hits, count, assoc;
  State(int T_, int M_) : T(T_), M(M_), anchors((size_t)T_ * 7, 0.0), means((size_t)T_ * 7, 0.0), p(T_, 0.0), hits(T_, 0), count(2, 0), assoc(M_, 0) {}
  bool same(const State& o) const {
    return anchors == o.anchors && means == o.means && p == o.p && hits == o.hits && count == o.count && assoc == o.assoc;
  }
};
void random_pose(float* P, double spread) {            // a rotation about z then x, a translation on a coarse grid
  const double a = uniform() * 6.0, b = uniform() * 3.0;
  const double R[9] = {cos(a), -sin(a) * cos(b), sin(a) * sin(b), sin(a), cos(a) * cos(b), -cos(a) * sin(b), 0, sin(b), cos(b)};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P[i * 4 + j] = (float)R[i * 3 + j];
    P[i * 4 + 3] = (float)((int)(uniform() * 6) * 0.2 + uniform() * spread);
  }
  P[12] = P[13] = P[14] = 0.f; P[15] = 1.f;
}
}  // namespace

int main() {
  const double cam[16] = {0, -1, 0, 0.5, 1, 0, 0, -0.25, 0, 0, 1, 0.125, 0, 0, 0, 1};
  int failures = 0, updates = 0;
  for (int round = 0; round < 40; ++round) {
    const int T = 4 + (int)(uniform() * 300), M = 1 + (int)(uniform() * 90);
    State a(T, M), b(T, M);
    for (int frame = 0; frame < 6; ++frame) {
      const int n = (int)(uniform() * (M + 1));
      // exactly n rows: the sanitizer sees a read behind the last one
      std::vector<float> Rt((size_t)n * 16);
      std::vector<int32_t> rel(n);
      for (int m = 0; m < n; ++m) { random_pose(&Rt[(size_t)m * 16], 0.02); rel[m] = uniform() < 0.85; }
      const State before = a;
      const int ra = track_walk(Rt.data(), 0, rel.data(), n, cam, a.anchors.data(), a.means.data(), a.p.data(), a.hits.data(), a.count.data(),
                                a.assoc.data(), T, M, 0.05, 1e-3, 0.1, 1.0, 1, 0);
      const int rb = track_walk(Rt.data(), 0, rel.data(), n, cam, b.anchors.data(), b.means.data(), b.p.data(), b.hits.data(), b.count.data(),
                                b.assoc.data(), T, M, 0.05, 1e-3, 0.1, 1.0, 64, 0);
      ++updates;
      if (ra != 0 || rb != 0 || !a.same(b)) ++failures;
      if (a.count[1] != 0) {                           // overflow: nothing but the flag may have changed
        State flagged = before;
        flagged.count[1] = 1;
        if (!a.same(flagged)) ++failures;
        break;
      }
      if (a.count[0] < before.count[0] || a.count[0] > T) ++failures;
    }
  }
  printf("%d updates, %d failures\n", updates, failures);
  return failures ? 1 : 0;
}
#endif
