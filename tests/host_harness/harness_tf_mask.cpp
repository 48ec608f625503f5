// CPU-only test harness of the compiled attention mask's host side (flope_amd/csrc/tf_attn_mask.h): packing, the
// first / last tables, both validators, the per-length check, the pair counts and the masked launch -- what flope_tf_mask_create and
// the flope_tf_*_masked entry points go through.  tests/test_tf_mask_host.py holds each against brute force through the shared
// library, and builds this file once more with TF_MASK_MAIN as a stand-alone program under -fsanitize=address,undefined, which checks
// the same properties with its own brute force and no Python in the process.  Not part of the product.
#include "tf_attn_mask.h"

extern "C" {

int tf_mask_words(int L) { return flope_tf_plan::tf_mask_words(L); }
void tf_mask_pack(const unsigned char* allow, int L, uint32_t* bits) { flope_tf_plan::tf_mask_pack(allow, L, bits); }
void tf_mask_first_last(const uint32_t* bits, int L, int* first, int* last) { flope_tf_plan::tf_mask_first_last(bits, L, first, last); }
int tf_mask_empty_row(const uint32_t* bits, int L) { return flope_tf_plan::tf_mask_empty_row(bits, L); }
// out2: {column, row} of the first set padding bit, or {-1, -1}
void tf_mask_padding_bit(const uint32_t* bits, int L, int* out2) {
  int row = -1;
  out2[0] = flope_tf_plan::tf_mask_padding_bit(bits, L, &row);
  out2[1] = row;
}
int tf_mask_length_row(const int* first, int L, int n) { return flope_tf_plan::tf_mask_length_row(first, L, n); }
long long tf_mask_pairs_len(const uint32_t* bits, int L, int n) { return flope_tf_plan::tf_mask_pairs_len(bits, L, n); }
long long tf_mask_pairs(const uint32_t* bits, int L) { return flope_tf_plan::tf_mask_pairs(bits, L); }
// out4: {grid_x, grid_y, block, lds bytes}
void tf_mask_launch(int head_dim, int batch, int heads, int max_len, int L, long* out4) {
  const flope_tf_plan::TfAttnLaunch l = flope_tf_plan::tf_mask_launch(head_dim, batch, heads, max_len, L);
  out4[0] = l.grid_x; out4[1] = l.grid_y; out4[2] = l.block; out4[3] = (long)l.lds;
}
long tf_mask_lds_words_at(int max_len) { return (long)flope_tf_plan::tf_mask_lds_words_at(max_len); }
int tf_mask_attn_id() { return FLOPE_TF_ATTN_MASKED; }

}  // extern "C"

#ifdef TF_MASK_MAIN
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
  int masks = 0;
  for (int L : sizes)
    for (int rep = 0; rep < 40; ++rep) {
      const unsigned density = rnd() % 101;                        // per cent of allowed entries; 0 and 100 among them
      std::vector<unsigned char> allow((size_t)L * L);
      for (auto& a : allow) a = rnd() % 100 < density;
      if (rep % 3 == 0)
        for (int i = 0; i < L; ++i) allow[(size_t)i * L + i] = 1;
      const int nw = P::tf_mask_words(L);
      std::vector<uint32_t> bits((size_t)L * nw, 0xffffffffu);      // exactly sized: the sanitizer sees a word too many
      P::tf_mask_pack(allow.data(), L, bits.data());
      std::vector<int> first(L), last(L);
      P::tf_mask_first_last(bits.data(), L, first.data(), last.data());
      int empty = -1;
      long long pairs = 0;
      for (int i = 0; i < L; ++i) {
        int f = L, l = -1;
        for (int j = 0; j < L; ++j) {
          EXPECT(P::tf_mask_bit(bits.data(), L, i, j) == (allow[(size_t)i * L + j] != 0));
          if (allow[(size_t)i * L + j]) { if (f == L) f = j; l = j; ++pairs; }
        }
        EXPECT(first[i] == f && last[i] == l);
        if (l < 0 && empty < 0) empty = i;
      }
      EXPECT(P::tf_mask_empty_row(bits.data(), L) == empty);
      EXPECT(P::tf_mask_pairs(bits.data(), L) == pairs);
      EXPECT(P::tf_mask_padding_bit(bits.data(), L, nullptr) == -1);
      for (int n = 1; n <= L; ++n) {
        int bad = -1;
        long long pn = 0;
        for (int i = 0; i < n; ++i) {
          int cnt = 0;
          for (int j = 0; j < n; ++j) cnt += allow[(size_t)i * L + j] != 0;
          if (!cnt && bad < 0) bad = i;
          pn += cnt;
        }
        EXPECT(P::tf_mask_length_row(first.data(), L, n) == bad);
        EXPECT(P::tf_mask_pairs_len(bits.data(), L, n) == pn);
      }
      if (L & 31) {                                                 // one padding bit set: found, with its row
        const int row = (int)(rnd() % (unsigned)L), col = L + (int)(rnd() % (unsigned)(nw * 32 - L));
        bits[(size_t)row * nw + nw - 1] |= 1u << (col & 31);
        int r = -1;
        EXPECT(P::tf_mask_padding_bit(bits.data(), L, &r) == col && r == row);
        std::vector<int> f2(L), l2(L);
        P::tf_mask_first_last(bits.data(), L, f2.data(), l2.data());   // the tables do not look at padding columns
        EXPECT(f2 == first && l2 == last);
      }
      ++masks;
    }
  for (int L : sizes)
    for (int max_len = 1; max_len <= L; max_len += 1 + L / 7) {
      const P::TfAttnLaunch l = P::tf_mask_launch(8, 3, 2, max_len, L);
      EXPECT(l.block == 256 && l.grid_x == 6 && l.grid_y >= 1 && l.grid_y <= 64);
      EXPECT(l.lds == ((size_t)4 * max_len + (size_t)4 * P::tf_mask_words(L)) * 4);
      std::vector<int> seen(max_len, 0);                            // the kernel's row walk: wave w of workgroup y takes rows y * 4 + w, + 4 grid_y, ..
      for (unsigned y = 0; y < l.grid_y; ++y)
        for (int w = 0; w < 4; ++w)
          for (int i = (int)y * 4 + w; i < max_len; i += (int)l.grid_y * 4) ++seen[i];
      for (int i = 0; i < max_len; ++i) EXPECT(seen[i] == 1);
    }
  printf("tf_mask host checks: %d masks, %d failures\n", masks, g_fail);
  return g_fail ? 1 : 0;
}
#endif
