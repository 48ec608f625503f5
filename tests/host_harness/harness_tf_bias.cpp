// CPU-only test harness of the compiled additive bias's host side (flope_amd/csrc/tf_attn_mask.h): the bit words derived
// from the -inf entries, both validators a bias adds, the device layout and the index of a bias entry -- what flope_tf_bias_create goes
// through before it allocates.  tests/test_tf_bias_host.py holds each against brute force through the shared library, and builds this
// file once more with TF_BIAS_MAIN as a stand-alone program under -fsanitize=address,undefined, which checks the same properties with
// its own brute force and no Python in the process.  Not part of the product.
#include "tf_attn_mask.h"

extern "C" {

int tf_bias_words(int L) { return flope_tf_plan::tf_mask_words(L); }
// bias: [planes][L][L]; plane 0's allowed set -> bits [L][words]
void tf_bias_pack(const float* bias, int L, uint32_t* bits) { if (bias && bits) flope_tf_plan::tf_bias_pack(bias, L, bits); }
// the words tf_mask_pack gives for an allowed set, to hold tf_bias_pack against
void tf_bias_mask_pack(const unsigned char* allow, int L, uint32_t* bits) { flope_tf_plan::tf_mask_pack(allow, L, bits); }
void tf_bias_first_last(const uint32_t* bits, int L, int* first, int* last) { flope_tf_plan::tf_mask_first_last(bits, L, first, last); }
int tf_bias_empty_row(const uint32_t* bits, int L) { return flope_tf_plan::tf_mask_empty_row(bits, L); }
// out3: {plane, row, col} of the first +inf / NaN entry, untouched without one.  Returns 1 / 0, -1 for a NULL argument.
int tf_bias_nonfinite(const float* bias, int L, int planes, int* out3) {
  if (!bias || !out3) return -1;
  return flope_tf_plan::tf_bias_nonfinite(bias, L, planes, out3, out3 + 1, out3 + 2) ? 1 : 0;
}
// out3: {plane, row, col} of the first entry whose masked-or-not differs from plane 0's
int tf_bias_plane_differs(const float* bias, int L, int planes, int* out3) {
  if (!bias || !out3) return -1;
  return flope_tf_plan::tf_bias_plane_differs(bias, L, planes, out3, out3 + 1, out3 + 2) ? 1 : 0;
}
long tf_bias_dev_bias_at(int L) { return (long)flope_tf_plan::tf_bias_dev_bias_at(L); }
long tf_bias_dev_bytes(int L, int planes) { return (long)flope_tf_plan::tf_bias_dev_bytes(L, planes); }
long tf_bias_index(int L, int planes, int h, int i, int j) { return (long)flope_tf_plan::tf_bias_index(L, planes, h, i, j); }
int tf_bias_attn_id() { return FLOPE_TF_ATTN_BIASED; }

}  // extern "C"

#ifdef TF_BIAS_MAIN
#include <stdio.h>
#include <stdlib.h>

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
  const int sizes[] = {1, 2, 15, 31, 32, 33, 63, 64, 65, 96, 130};
  int biases = 0;
  for (int L : sizes)
    for (int planes : {1, 4})
      for (int rep = 0; rep < 20; ++rep) {
        const unsigned density = rnd() % 101;                      // per cent of allowed entries; 0 and 100 among them
        const size_t LL = (size_t)L * L;
        std::vector<unsigned char> allow(LL);
        for (auto& a : allow) a = rnd() % 100 < density;
        std::vector<float> bias((size_t)planes * LL);               // exactly sized: the sanitizer sees an entry too many
        for (int p = 0; p < planes; ++p)
          for (size_t t = 0; t < LL; ++t) bias[(size_t)p * LL + t] = allow[t] ? (float)((int)(rnd() % 2001) - 1000) / 100.f : -INFINITY;
        const int nw = P::tf_mask_words(L);
        std::vector<uint32_t> bits((size_t)L * nw, 0xffffffffu), want((size_t)L * nw, 0u);
        P::tf_bias_pack(bias.data(), L, bits.data());
        P::tf_mask_pack(allow.data(), L, want.data());
        EXPECT(bits == want);
        int at[3] = {-7, -7, -7};
        EXPECT(!P::tf_bias_nonfinite(bias.data(), L, planes, at, at + 1, at + 2) && at[0] == -7);
        EXPECT(!P::tf_bias_plane_differs(bias.data(), L, planes, at, at + 1, at + 2) && at[0] == -7);
        // one +inf or NaN somewhere, a second behind it: the first in (plane, row, col) order is named
        const size_t t0 = rnd() % bias.size(), t1 = t0 + rnd() % (bias.size() - t0);
        const float keep0 = bias[t0], keep1 = bias[t1];
        bias[t0] = rep & 1 ? INFINITY : NAN;
        bias[t1] = rep & 2 ? INFINITY : NAN;
        EXPECT(P::tf_bias_nonfinite(bias.data(), L, planes, at, at + 1, at + 2));
        EXPECT(at[0] == (int)(t0 / LL) && at[1] == (int)(t0 % LL / L) && at[2] == (int)(t0 % L));
        bias[t0] = keep0; bias[t1] = keep1;
        if (planes > 1) {                                           // one entry of a later plane flipped
          const int p = 1 + (int)(rnd() % (unsigned)(planes - 1));
          const size_t t = rnd() % LL;
          const float keep = bias[(size_t)p * LL + t];
          bias[(size_t)p * LL + t] = keep == -INFINITY ? -1e30f : -INFINITY;
          EXPECT(P::tf_bias_plane_differs(bias.data(), L, planes, at, at + 1, at + 2));
          EXPECT(at[0] == p && at[1] == (int)(t / L) && at[2] == (int)(t % L));
          P::tf_bias_pack(bias.data(), L, bits.data());            // the words come from plane 0 alone
          EXPECT(bits == want);
          bias[(size_t)p * LL + t] = keep;
        }
        for (int h = 0; h < 4; ++h) {                               // every entry a head may address lies inside the planes
          const int i = (int)(rnd() % (unsigned)L), j = (int)(rnd() % (unsigned)L);
          const size_t idx = P::tf_bias_index(L, planes, h, i, j);
          EXPECT(idx < bias.size() && idx == ((size_t)(planes > 1 ? h : 0) * L + i) * L + j);
        }
        EXPECT(P::tf_bias_dev_bias_at(L) == ((size_t)L * nw + 2 * (size_t)L) * 4);
        EXPECT(P::tf_bias_dev_bytes(L, planes) == P::tf_bias_dev_bias_at(L) + bias.size() * 4);
        ++biases;
      }
  printf("tf_bias host checks: %d biases, %d failures\n", biases, g_fail);
  return g_fail ? 1 : 0;
}
#endif
