// CPU-only test harness of a stream state's distance table (flope_amd/csrc/tf_encoder_stream.h): how many distances a
// state needs, the planes check, the first non-finite entry, the refusals of flope_tf_stream_open_bias in their order, the entry a
// visible key reads and the test the biased kernels make in front of their first load.  tests/test_tf_stream_bias_host.py holds each
// against brute force through the shared library, and builds this file once more with TF_STREAM_BIAS_MAIN as a stand-alone program
// under -fsanitize=address,undefined, which checks the same properties with its own brute force and no Python in the process.  Not
// part of the product.
#include "tf_encoder_stream.h"

extern "C" {

int tf_sbias_distances(int capacity, int window) { return flope_tf_plan::tf_stream_bias_distances(capacity, window); }
int tf_sbias_planes_ok(int planes, int H) { return flope_tf_plan::tf_stream_bias_planes_ok(planes, H) ? 1 : 0; }
// out2: {plane, distance} of the first NaN / +-inf entry, untouched without one.  Returns 1 / 0, -1 for a NULL argument.
int tf_sbias_nonfinite(const float* rel, int planes, int D, int* out2) {
  if (!rel || !out2) return -1;
  return flope_tf_plan::tf_stream_bias_nonfinite(rel, planes, D, out2, out2 + 1) ? 1 : 0;
}
// the refusals of the open in their order; out2 as above (written by kTfStreamBiasValue alone).  rel may be NULL: that is a refusal
int tf_sbias_check_open(int capacity, int window, int H, int planes, int distances, const float* rel, int* out2) {
  if (!out2) return 1;
  return flope_tf_plan::tf_stream_check_open_bias(capacity, window, H, planes, distances, rel, out2, out2 + 1);
}
int tf_sbias_index(int L, int j) { return flope_tf_plan::tf_stream_bias_index(L, j); }
int tf_sbias_keys_ok(int keys, int D) { return flope_tf_plan::tf_stream_bias_keys_ok(keys, D) ? 1 : 0; }
long tf_sbias_bytes(int planes, int D) { return (long)flope_tf_plan::tf_stream_bias_bytes(planes, D); }
// the visible key counts the kernels hold against D: a step at pos, a chunk of len at pos0
int tf_sbias_step_keys(int pos, int W) { return flope_tf_plan::tf_window_keys(pos, W); }
int tf_sbias_extend_keys(int pos0, int len, int W) { return flope_tf_plan::tf_extend_keys(pos0, len, W); }
int tf_sbias_code(int which) {
  using namespace flope_tf_plan;
  const int codes[] = {kTfStreamOk, kTfStreamBiasPlanes, kTfStreamBiasDistances, kTfStreamBiasNull, kTfStreamBiasValue};
  return which >= 0 && which < 5 ? codes[which] : 1;
}
int tf_sbias_step_id() { return FLOPE_TF_STEP_BIASED; }
int tf_sbias_extend_id() { return FLOPE_TF_EXTEND_BIASED; }

}  // extern "C"

#ifdef TF_STREAM_BIAS_MAIN
#include <math.h>
#include <stdio.h>

#include <vector>

namespace {
unsigned long long g_state = 0x9e3779b97f4a7c15ull;
unsigned rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (unsigned)(g_state >> 32); }
int g_fail = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)
}  // namespace

int main() {
  namespace P = flope_tf_plan;
  int tables = 0;
  for (int rep = 0; rep < 400; ++rep) {
    const int capacity = 1 + (int)(rnd() % 200), window = rep % 3 ? 1 + (int)(rnd() % (unsigned)capacity) : 0;
    const int H = 1 + (int)(rnd() % 8), planes = rep % 2 ? H : 1;
    const int D = P::tf_stream_bias_distances(capacity, window);
    EXPECT(D == (window ? window : capacity));
    std::vector<float> rel((size_t)planes * D);                     // exactly sized: the sanitizer sees an entry too many
    for (auto& v : rel) v = (float)((int)(rnd() % 2001) - 1000) / 100.f;
    EXPECT(P::tf_stream_bias_bytes(planes, D) == rel.size() * sizeof(float));
    int at[2] = {-7, -7};
    EXPECT(!P::tf_stream_bias_nonfinite(rel.data(), planes, D, at, at + 1) && at[0] == -7 && at[1] == -7);
    EXPECT(P::tf_stream_check_open_bias(capacity, window, H, planes, D, rel.data(), at, at + 1) == P::kTfStreamOk && at[0] == -7);
    // one non-finite entry somewhere, a second behind it: the first in (plane, distance) order is named
    const size_t t0 = rnd() % rel.size(), t1 = t0 + rnd() % (rel.size() - t0);
    const float keep0 = rel[t0], keep1 = rel[t1];
    const float bad[3] = {NAN, INFINITY, -INFINITY};
    rel[t1] = bad[(rep + 1) % 3];
    rel[t0] = bad[rep % 3];
    EXPECT(P::tf_stream_bias_nonfinite(rel.data(), planes, D, at, at + 1) && at[0] == (int)(t0 / D) && at[1] == (int)(t0 % D));
    at[0] = at[1] = -7;
    EXPECT(P::tf_stream_check_open_bias(capacity, window, H, planes, D, rel.data(), at, at + 1) == P::kTfStreamBiasValue);
    EXPECT(at[0] == (int)(t0 / D) && at[1] == (int)(t0 % D));
    // the refusals in front of it do not read the table: a wrong plane count, a wrong length (a table of that length would be too short)
    at[0] = at[1] = -7;
    EXPECT(P::tf_stream_check_open_bias(capacity, window, H, H + 1 + (H == 1), D, rel.data(), at, at + 1) == P::kTfStreamBiasPlanes);
    EXPECT(P::tf_stream_check_open_bias(capacity, window, H, planes, D + 1, rel.data(), at, at + 1) == P::kTfStreamBiasDistances);
    EXPECT(P::tf_stream_check_open_bias(capacity, window, H, planes, D - 1, rel.data(), at, at + 1) == P::kTfStreamBiasDistances);
    EXPECT(P::tf_stream_check_open_bias(capacity, window, H, planes, D, nullptr, at, at + 1) == P::kTfStreamBiasNull && at[0] == -7);
    rel[t0] = keep0; rel[t1] = keep1;
    // every entry a query of this state may address lies inside the planes: read it
    for (int q = 0; q < 32; ++q) {
      const int pos = window ? (int)(rnd() % 100000u) : (int)(rnd() % (unsigned)capacity);
      const int L = P::tf_window_keys(pos, window);
      EXPECT(P::tf_stream_bias_keys_ok(L, D));
      const int h = (int)(rnd() % (unsigned)H), plane = planes == H ? h : 0;
      float sum = 0.f;
      for (int j = 0; j < L; ++j) {
        const int t = P::tf_stream_bias_index(L, j);
        EXPECT(t == pos - (pos - L + 1 + j) && t >= 0 && t < D);
        sum += rel[(size_t)plane * D + t];
      }
      EXPECT(sum == sum);
      EXPECT(!P::tf_stream_bias_keys_ok(D + 1 + (int)(rnd() % 5u), D));
    }
    ++tables;
  }
  EXPECT(P::tf_stream_bias_planes_ok(1, 4) && P::tf_stream_bias_planes_ok(4, 4) && P::tf_stream_bias_planes_ok(1, 1));
  EXPECT(!P::tf_stream_bias_planes_ok(0, 4) && !P::tf_stream_bias_planes_ok(2, 4) && !P::tf_stream_bias_planes_ok(-1, 4) && !P::tf_stream_bias_planes_ok(5, 4));
  printf("tf_stream_bias host checks: %d tables, %d failures\n", tables, g_fail);
  return g_fail ? 1 : 0;
}
#endif
