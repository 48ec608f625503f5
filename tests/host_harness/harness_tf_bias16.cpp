// CPU-only test harness of a compiled bias on the 16-bit MFMA attention (option "bias_mfma"; flope_amd/csrc/tf_attn_mask.h; DESIGN.md
// 44): tf_attn_pick_biased, the device layout with the tile map behind the planes, the entry a lane of a taken step loads
// (tf_bias16_lane_index) and which form of the load the step takes -- what flope_tf_bias_create uploads and the BIASED instantiation of
// tf_attn_tiled_masked goes through.  tests/test_tf_bias16_host.py holds each against brute force in numpy through the shared library, and
// builds this file once more with TF_BIAS16_MAIN as a stand-alone program under -fsanitize=address,undefined, which walks every lane of
// every taken step over planes sized exactly, with no Python in the process.  Not part of the product.
#include "tf_attn_mask.h"

extern "C" {

int tf_bias16_pick(int dtype, int head_dim, int opt_generic, int opt_bias_mfma, int aligned16) {
  return flope_tf_plan::tf_attn_pick_biased(dtype, head_dim, opt_generic, opt_bias_mfma, aligned16);
}
int tf_bias16_built(int head_dim) { return flope_tf_plan::tf_attn_biased16_built(head_dim); }
int tf_bias16_attn_id() { return FLOPE_TF_ATTN_BIASED16; }
// out5: byte offsets of the planes, of start and of the entries in the bias's device allocation, its size with `entries` entries, and
// the size of the allocation without the tile map (tf_bias_dev_bytes)
void tf_bias16_dev_layout(int L, int planes, long long entries, long long* out5) {
  out5[0] = (long long)flope_tf_plan::tf_bias_dev_bias_at(L);
  out5[1] = (long long)flope_tf_plan::tf_bias_dev_start_at(L, planes);
  out5[2] = (long long)flope_tf_plan::tf_bias_dev_tiles_at(L, planes);
  out5[3] = (long long)flope_tf_plan::tf_bias_dev_bytes_tiled(L, planes, entries);
  out5[4] = (long long)flope_tf_plan::tf_bias_dev_bytes(L, planes);
}
long long tf_bias16_lane_index(int L, int planes, int n, int h, int query, int kb, int u, int g, int q) {
  return (long long)flope_tf_plan::tf_bias16_lane_index(L, planes, n, h, query, kb, u, g, q);
}
int tf_bias16_step_vec(int L, int kb) { return flope_tf_plan::tf_bias16_step_vec(L, kb); }
// Every index the lanes of the workgroups of a sequence of n tokens under head h form, in walk order, into idx (or counted when idx is
// NULL): for each query block, each listed entry of the corner's prefix, each step below n whose class for a wave is not "none", each of
// the wave's 32 queries (tile qt, lane row li), u, g, q.  allow: the allowed set, row-major [L][L].  Returns the count.
long long tf_bias16_walk(const unsigned char* allow, int L, int planes, int n, int h, long long* idx) {
  namespace P = flope_tf_plan;
  size_t nw = (size_t)P::tf_mask_words(L);
  uint32_t* bits = new uint32_t[(size_t)L * nw];
  P::tf_mask_pack(allow, L, bits);
  const int nqb = P::tf_mask_query_blocks(L);
  int* start = new int[nqb + 1];
  const long long ne = P::tf_mask_tiles_build(bits, L, start, nullptr);
  P::TfMaskTile* tiles = new P::TfMaskTile[(size_t)(ne ? ne : 1)];
  P::tf_mask_tiles_build(bits, L, start, tiles);
  long long cnt = 0;
  for (int qb = 0; qb * P::kTfAttnTiledQueries < n; ++qb) {
    const int got = P::tf_mask_tiles_corner(tiles, start[qb], start[qb + 1], n);
    for (int e = start[qb]; e < start[qb] + got; ++e)
      for (int s = 0; s < 2; ++s) {
        const int kb = tiles[e].kblock * P::kTfAttnTiledKB + 32 * s;
        if (kb >= n) continue;
        for (int w = 0; w < 4; ++w) {
          if (P::tf_mask_tile_class(tiles[e].cls, w, s) == P::kTfMaskNone) continue;
          for (int l = 0; l < 32; ++l)
            for (int u = 0; u < 2; ++u)
              for (int g = 0; g < 4; ++g)
                for (int q = 0; q < 4; ++q) {
                  if (idx) idx[cnt] = (long long)P::tf_bias16_lane_index(L, planes, n, h, qb * 128 + w * 32 + l, kb, u, g, q);
                  ++cnt;
                }
        }
      }
  }
  delete[] bits; delete[] start; delete[] tiles;
  return cnt;
}

}  // extern "C"

#ifdef TF_BIAS16_MAIN
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
  const int sizes[] = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 300};
  const unsigned dens[] = {1, 40, 99, 100};                         // per cent of allowed entries; 100: all clear
  const int H = 3;
  int biases = 0;
  long long loads = 0;
  for (int L : sizes)
    for (int rep = 0; rep < 4; ++rep) {
      const int planes = rep & 1 ? H : 1;
      std::vector<unsigned char> allow((size_t)L * L);
      for (auto& a : allow) a = rnd() % 100 < dens[rep];
      for (int i = 0; i < L; ++i) allow[(size_t)i * L + i] = 1;     // the diagonal: every corner leaves every row a key
      std::vector<float> bias((size_t)planes * L * L);              // exactly sized: the sanitizer sees an entry too many
      for (int p = 0; p < planes; ++p)
        for (size_t t = 0; t < (size_t)L * L; ++t) bias[(size_t)p * L * L + t] = allow[t] ? (float)(p * 1000) + (float)(t % 997) : -INFINITY;
      const int nw = P::tf_mask_words(L), nqb = P::tf_mask_query_blocks(L);
      std::vector<uint32_t> bits((size_t)L * nw);
      P::tf_bias_pack(bias.data(), L, bits.data());
      std::vector<int> start(nqb + 1);
      const long long ne = P::tf_mask_tiles_build(bits.data(), L, start.data(), nullptr);
      std::vector<P::TfMaskTile> tiles((size_t)ne);
      P::tf_mask_tiles_build(bits.data(), L, start.data(), tiles.data());
      // the layout: the two old values, the map behind the planes, the entries on a 16-byte boundary
      EXPECT(P::tf_bias_dev_bias_at(L) == ((size_t)L * nw + 2 * (size_t)L) * 4);
      EXPECT(P::tf_bias_dev_bytes(L, planes) == P::tf_bias_dev_bias_at(L) + (size_t)planes * L * L * 4);
      EXPECT(P::tf_bias_dev_start_at(L, planes) == P::tf_bias_dev_bytes(L, planes));
      EXPECT(P::tf_bias_dev_tiles_at(L, planes) % 16 == 0 && P::tf_bias_dev_tiles_at(L, planes) >= P::tf_bias_dev_start_at(L, planes) + (size_t)(nqb + 1) * 4);
      EXPECT(P::tf_bias_dev_tiles_at(L, planes) < P::tf_bias_dev_start_at(L, planes) + (size_t)(nqb + 1) * 4 + 16);
      EXPECT(P::tf_bias_dev_bytes_tiled(L, planes, ne) == P::tf_bias_dev_tiles_at(L, planes) + (size_t)ne * 16);
      if (!(L & 3)) EXPECT(P::tf_bias_dev_bias_at(L) % 16 == 0);    // what the 16-byte form of the load relies on
      for (int n = 1; n <= L; ++n) {                                // every corner length
        if (n != L && n != 1 && n % 7 && n != L - 1) continue;
        for (int h = 0; h < H; ++h)
          for (int qb = 0; qb * 128 < n; ++qb) {
            const int got = P::tf_mask_tiles_corner(tiles.data(), start[qb], start[qb + 1], n);
            EXPECT(got >= 1);
            for (int e = start[qb]; e < start[qb] + got; ++e)
              for (int s = 0; s < 2; ++s) {
                const int kb = tiles[e].kblock * 64 + 32 * s;
                if (kb >= n) continue;
                const bool vec = P::tf_bias16_step_vec(L, kb);
                EXPECT(vec == (L % 4 == 0 && kb + 32 <= L));
                for (int w = 0; w < 4; ++w) {
                  if (P::tf_mask_tile_class(tiles[e].cls, w, s) == P::kTfMaskNone) continue;
                  for (int l = 0; l < 32; ++l) {
                    const int query = qb * 128 + w * 32 + l, row = query < n ? query : n - 1;
                    const size_t lo = ((size_t)(planes > 1 ? h : 0) * L + row) * L;
                    for (int u = 0; u < 2; ++u)
                      for (int g = 0; g < 4; ++g) {
                        for (int q = 0; q < 4; ++q) {
                          const int key = kb + 16 * u + 4 * g + q;
                          const size_t idx = P::tf_bias16_lane_index(L, planes, n, h, query, kb, u, g, q);
                          EXPECT(idx >= lo && idx < lo + (size_t)L && idx < bias.size());
                          EXPECT(idx - lo == (size_t)(key < L ? key : L - 1));
                          volatile float b = bias[idx];             // the load itself, under the sanitizer
                          if (key < n && allow[(size_t)row * L + key]) EXPECT(b == (float)((planes > 1 ? h : 0) * 1000) + (float)(((size_t)row * L + key) % 997));
                          ++loads;
                        }
                        if (vec) {                                  // the 16-byte form: four entries of the row, on a 16-byte boundary of the planes
                          const size_t i0 = P::tf_bias16_lane_index(L, planes, n, h, query, kb, u, g, 0);
                          EXPECT(i0 % 4 == 0 && i0 + 3 < lo + (size_t)L && P::tf_bias16_lane_index(L, planes, n, h, query, kb, u, g, 3) == i0 + 3);
                        }
                      }
                  }
                }
              }
          }
      }
      ++biases;
    }
  for (int hd : {6, 32, 64, 96, 128, 160})
    for (int dt : {FLOPE_DT_BF16, FLOPE_DT_F16, FLOPE_DT_F32})
      for (int k = 0; k < 8; ++k) {
        const bool want16 = dt != FLOPE_DT_F32 && (k & 1) && !(k & 2) && (k & 4) && (hd == 32 || hd == 64 || hd == 96 || hd == 128);
        EXPECT(P::tf_attn_pick_biased(dt, hd, (k >> 1) & 1, k & 1, (k >> 2) & 1) == (want16 ? FLOPE_TF_ATTN_BIASED16 : FLOPE_TF_ATTN_BIASED));
      }
  EXPECT(P::tf_attn_pick_biased(FLOPE_DT_F16, 64, 0, 2, 1) == FLOPE_TF_ATTN_BIASED);
  printf("tf_bias16 host checks: %d biases, %lld loads, %d failures\n", biases, loads, g_fail);
  return g_fail ? 1 : 0;
}
#endif
