// CPU-only test harness of the tile map of a compiled attention mask (flope_amd/csrc/tf_attn_mask.h): the per-query-block
// lists of key blocks, colany, the step classes, the corner prefix, the word and bit a lane reads, tf_attn_pick_masked and the launch
// of tf_attn_tiled_masked -- what flope_tf_mask_create uploads and launch_attention_masked goes through.  tests/test_tf_mask16_host.py
// holds each against brute force in numpy through the shared library, and builds this file once more with TF_MASK16_MAIN as a
// stand-alone program under -fsanitize=address,undefined, which checks the same properties with its own brute force, every buffer sized
// exactly, and no Python in the process.  Not part of the product.
#include "tf_attn_mask.h"

extern "C" {

void tf_mask16_pack(const unsigned char* allow, int L, uint32_t* bits) { flope_tf_plan::tf_mask_pack(allow, L, bits); }
int tf_mask16_query_blocks(int L) { return flope_tf_plan::tf_mask_query_blocks(L); }
int tf_mask16_key_blocks(int L) { return flope_tf_plan::tf_mask_key_blocks(L); }
// start: nqb + 1 ints; tiles4: 4 uint32 per entry {kblock, colany_lo, colany_hi, cls}, or NULL to count
long long tf_mask16_build(const uint32_t* bits, int L, int* start, uint32_t* tiles4) {
  return flope_tf_plan::tf_mask_tiles_build(bits, L, start, (flope_tf_plan::TfMaskTile*)tiles4);
}
int tf_mask16_corner(const uint32_t* tiles4, int begin, int end, int n) {
  return flope_tf_plan::tf_mask_tiles_corner((const flope_tf_plan::TfMaskTile*)tiles4, begin, end, n);
}
int tf_mask16_class(uint32_t cls, int wave, int step) { return flope_tf_plan::tf_mask_tile_class(cls, wave, step); }
long long tf_mask16_lane_word(int L, int n, int query, int kb) { return (long long)flope_tf_plan::tf_mask_lane_word(L, n, query, kb); }
int tf_mask16_lane_bit(int u, int g, int q) { return flope_tf_plan::tf_mask_lane_bit(u, g, q); }
// out5: {query_blocks, blocks_listed, steps_none, steps_some, steps_all}
void tf_mask16_stats(int L, const int* start, const uint32_t* tiles4, long long* out5) {
  const flope_tf_plan::TfMaskTileStats s = flope_tf_plan::tf_mask_tile_stats(L, start, (const flope_tf_plan::TfMaskTile*)tiles4);
  out5[0] = s.query_blocks; out5[1] = s.blocks_listed; out5[2] = s.steps_none; out5[3] = s.steps_some; out5[4] = s.steps_all;
}
// out3: byte offsets of start and of the entries in the mask's device allocation, and its size with `entries` entries
void tf_mask16_dev_layout(int L, long long entries, long long* out3) {
  out3[0] = (long long)flope_tf_plan::tf_mask_dev_start_at(L);
  out3[1] = (long long)flope_tf_plan::tf_mask_dev_tiles_at(L);
  out3[2] = (long long)flope_tf_plan::tf_mask_dev_bytes(L, entries);
}
int tf_mask16_pick(int dtype, int head_dim, int opt_generic, int opt_mask_mfma, int aligned16) {
  return flope_tf_plan::tf_attn_pick_masked(dtype, head_dim, opt_generic, opt_mask_mfma, aligned16);
}
// out4: {grid_x, grid_y, block, lds bytes}
void tf_mask16_launch(int head_dim, int batch, int heads, int max_len, long* out4) {
  const flope_tf_plan::TfAttnLaunch l = flope_tf_plan::tf_mask16_launch(head_dim, batch, heads, max_len);
  out4[0] = l.grid_x; out4[1] = l.grid_y; out4[2] = l.block; out4[3] = (long)l.lds;
}
int tf_mask16_attn_id() { return FLOPE_TF_ATTN_MASKED16; }

}  // extern "C"

#ifdef TF_MASK16_MAIN
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
  const int sizes[] = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 257, 300};
  const unsigned dens[] = {1, 40, 99, 0, 100};                      // per cent of allowed entries; 0: one key per row, 100: all clear
  int masks = 0;
  for (int L : sizes)
    for (int rep = 0; rep < 10; ++rep) {
      const unsigned density = dens[rep % 5];
      std::vector<unsigned char> allow((size_t)L * L);
      for (auto& a : allow) a = rnd() % 100 < density;
      for (int i = 0; i < L; ++i) {                                 // every row has a key, as flope_tf_mask_create demands
        bool any = false;
        for (int j = 0; j < L; ++j) any |= allow[(size_t)i * L + j] != 0;
        if (!any) allow[(size_t)i * L + (rep & 1 ? i : (int)(rnd() % (unsigned)L))] = 1;
      }
      const int nw = P::tf_mask_words(L), nqb = P::tf_mask_query_blocks(L), nkb = P::tf_mask_key_blocks(L);
      std::vector<uint32_t> bits((size_t)L * nw);                   // exactly sized: the sanitizer sees a word too many
      P::tf_mask_pack(allow.data(), L, bits.data());
      std::vector<int> start(nqb + 1);
      const long long n = P::tf_mask_tiles_build(bits.data(), L, start.data(), nullptr);
      std::vector<P::TfMaskTile> tiles((size_t)n);
      EXPECT(P::tf_mask_tiles_build(bits.data(), L, start.data(), tiles.data()) == n);
      EXPECT(start[0] == 0 && start[nqb] == n);
      long long none = 0, some = 0, all = 0;
      for (int qb = 0; qb < nqb; ++qb) {
        EXPECT(start[qb + 1] > start[qb]);
        std::vector<int> listed(nkb, -1);
        for (int e = start[qb]; e < start[qb + 1]; ++e) {
          EXPECT(tiles[e].kblock >= 0 && tiles[e].kblock < nkb);
          if (e > start[qb]) EXPECT(tiles[e].kblock > tiles[e - 1].kblock);
          listed[tiles[e].kblock] = e;
        }
        for (int kblock = 0; kblock < nkb; ++kblock) {
          unsigned long long colany = 0;
          int cnt[4][2] = {}, tot[4][2] = {};
          for (int r = qb * 128; r < qb * 128 + 128 && r < L; ++r)
            for (int c = kblock * 64; c < kblock * 64 + 64 && c < L; ++c) {
              const int w = (r - qb * 128) / 32, s = (c - kblock * 64) / 32;
              ++tot[w][s];
              if (allow[(size_t)r * L + c]) { ++cnt[w][s]; colany |= 1ull << (c - kblock * 64); }
            }
          EXPECT((listed[kblock] >= 0) == (colany != 0));
          if (listed[kblock] < 0) continue;
          const P::TfMaskTile& t = tiles[listed[kblock]];
          EXPECT(t.colany_lo == (uint32_t)colany && t.colany_hi == (uint32_t)(colany >> 32));
          for (int w = 0; w < 4; ++w)
            for (int s = 0; s < 2; ++s) {
              const int want = !cnt[w][s] ? P::kTfMaskNone : cnt[w][s] == tot[w][s] ? P::kTfMaskAll : P::kTfMaskSome;
              EXPECT(P::tf_mask_tile_class(t.cls, w, s) == want);
              ++(want == P::kTfMaskNone ? none : want == P::kTfMaskSome ? some : all);
            }
          EXPECT((t.cls >> 16) == 0);
        }
        for (int nn = 1; nn <= L; ++nn) {                           // the corner's prefix, and every word a lane of a taken step loads
          int want = 0;
          for (int e = start[qb]; e < start[qb + 1]; ++e) want += tiles[e].kblock * 64 < nn;
          const int got = P::tf_mask_tiles_corner(tiles.data(), start[qb], start[qb + 1], nn);
          EXPECT(got == want);
          if (qb * 128 >= nn || (nn != L && nn % 13)) continue;
          for (int e = start[qb]; e < start[qb] + got; ++e)
            for (int s = 0; s < 2; ++s) {
              const int kb = tiles[e].kblock * 64 + 32 * s;
              if (kb >= nn) continue;
              for (int w = 0; w < 4; ++w) {
                if (P::tf_mask_tile_class(tiles[e].cls, w, s) != P::kTfMaskSome) continue;
                for (int l = 0; l < 32; ++l) {
                  const size_t idx = P::tf_mask_lane_word(L, nn, qb * 128 + w * 32 + l, kb);
                  EXPECT(idx < bits.size());
                  volatile uint32_t word = bits[idx];               // the load itself, under the sanitizer
                  (void)word;
                }
              }
            }
        }
      }
      const P::TfMaskTileStats st = P::tf_mask_tile_stats(L, start.data(), tiles.data());
      EXPECT(st.query_blocks == nqb && st.blocks_listed == n && st.steps_none == none && st.steps_some == some && st.steps_all == all);
      EXPECT(P::tf_mask_dev_tiles_at(L) % 16 == 0 && P::tf_mask_dev_tiles_at(L) >= P::tf_mask_dev_start_at(L) + (size_t)(nqb + 1) * 4);
      EXPECT(P::tf_mask_dev_bytes(L, n) == P::tf_mask_dev_tiles_at(L) + (size_t)n * 16);
      ++masks;
    }
  bool seen[32] = {};
  for (int u = 0; u < 2; ++u)
    for (int g = 0; g < 4; ++g)
      for (int q = 0; q < 4; ++q) { EXPECT(P::tf_mask_lane_bit(u, g, q) == 16 * u + 4 * g + q); seen[P::tf_mask_lane_bit(u, g, q)] = true; }
  for (bool b : seen) EXPECT(b);
  for (int hd : {6, 32, 64, 96, 128, 160})
    for (int dt : {FLOPE_DT_BF16, FLOPE_DT_F16, FLOPE_DT_F32})
      for (int k = 0; k < 8; ++k) {
        const bool want16 = dt != FLOPE_DT_F32 && (k & 1) && !(k & 2) && (k & 4) && (hd == 32 || hd == 64 || hd == 96 || hd == 128);
        EXPECT(P::tf_attn_pick_masked(dt, hd, (k >> 1) & 1, k & 1, (k >> 2) & 1) == (want16 ? FLOPE_TF_ATTN_MASKED16 : FLOPE_TF_ATTN_MASKED));
      }
  for (int max_len : {1, 128, 129, 300}) {
    const P::TfAttnLaunch l = P::tf_mask16_launch(96, 3, 2, max_len);
    EXPECT(l.grid_x == 6 && l.grid_y == (unsigned)(max_len + 127) / 128 && l.block == 256 && l.lds == P::tf_attn_tiled_lds(96));
  }
  printf("tf_mask16 host checks: %d masks, %d failures\n", masks, g_fail);
  return g_fail ? 1 : 0;
}
#endif
