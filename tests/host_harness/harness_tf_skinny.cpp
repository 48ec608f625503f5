// CPU-only test harness of the planner of option "skinny" (flope_amd/csrc/tf_skinny_plan.h, which tf_gemm_skinny calls per lane;
// DESIGN.md 48): the eligibility rule, the token-tile count, and for one shape (N, K, MT) a walk of the whole launch -- every
// workgroup, wave, lane, chunk and ks -- that checks
//   cover     the grid's waves own every (feature tile, token tile) exactly once, and their lanes every (token row, feature) once;
//   bounds    every 16-byte weight load lies inside the packed image of N K 2 bytes, every token load inside 16 MT rows of K 2 bytes
//             (the loads are made, from buffers of exactly those sizes, so a sanitizer build sees one that is not);
//   gemm      the loads are the ones tf_gemm_mfma's LDS read addresses select from the chunk's image: its weight tile is a linear copy
//             of the image, its token tile the per-lane swizzled copy; both address computations are restated here from the kernel;
//   meaning   through the packer's row order (host_pack.h lds_row_to_channel) and slot swizzle, restated: element j of the A fragment
//             of MFMA row li is W[feature of that row][64 c + 8 (4 ks + g) + j], and accumulator element q of a lane is feature
//             tf_skinny_feature + q.
// Not part of the product.  With -DTF_SKINNY_MAIN the file is a program of its own (built under -fsanitize=address,undefined by the
// test and run as a child process) that runs every shape of the test.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "host_pack.h"
#include "tf_skinny_plan.h"

using namespace flope_tf_plan;
using flope_host::lds_row_to_channel;

namespace {

// tf_gemm_mfma, restated: the byte of the packed image its wave (wn) reads from LDS as weight fragment t of (chunk, ks); the weight
// half of a ring buffer is a linear copy of the chunk's 16384-byte image
size_t gemm_w_image_off(int nt, int nch, int chunk, int wn, int t, int ks, int lane) {
  const int g = lane >> 4, sw = (lane >> 1) & 7;
  const int rdW = (wn * 64 + (lane & 15)) * 128;
  const int so = ((ks * 4 + g) ^ sw) << 4;
  return ((size_t)nt * nch + chunk) * 16384 + (size_t)(rdW + t * 2048 + so);
}

// ... and the byte of X [rows][K] its wave (wm) reads as token fragment t: the LDS address of the read, taken back through the
// per-lane source address of the copy (thread (wave w, i, lane) fills LDS byte w 4096 + i 1024 + lane 16 of the token half)
size_t gemm_x_global_off(int K, int chunk, int wm, int t, int ks, int lane) {
  const int g = lane >> 4, sw = (lane >> 1) & 7;
  const int rdX = (wm * 64 + (lane & 15)) * 128;
  const int lds = rdX + t * 2048 + (((ks * 4 + g) ^ sw) << 4);           // relative to the token half
  const int w = lds / 4096, i = (lds % 4096) / 1024, l = (lds % 1024) / 16;
  const int row = (w * 4 + i) * 8 + (l >> 3), slot = l & 7;
  return (size_t)row * K * 2 + (size_t)((slot ^ ((row >> 1) & 7)) << 4) + (size_t)chunk * 128;
}

}  // namespace

extern "C" {

int tf_skinny_h_ok(int dtype16, int opt_skinny, int opt_generic, int packed, int y_f32, int M) {
  return tf_skinny_ok(dtype16, opt_skinny, opt_generic, packed, y_f32, M) ? 1 : 0;
}
int tf_skinny_h_mt(int M) { return tf_skinny_mt(M); }
int tf_skinny_h_consts(int* out3) { out3[0] = kTfSkinnyMaxRows; out3[1] = kTfSkinnyWaves; out3[2] = kTfSkinnyDepth; return 0; }
void tf_skinny_h_launch(int N, int MT, unsigned* grid, unsigned* block) {
  const TfSkinnyLaunch l = tf_skinny_launch(N, MT);
  *grid = l.grid; *block = l.block;
}

// One shape: N % 128 == 0, K % 64 == 0 (the padded K), MT 1 or 2.  fails[0 .. 3] = cover, bounds, gemm, meaning; returns their sum.
// `broken`: 1 = the weight swizzle dropped, 2 = token tile 1 read at row 8, 4 = the feature order of an unpermuted image
int tf_skinny_h_shape(int N, int K, int MT, int broken, long long* fails) {
  const int nch = K / 64, tiles = N / 16;
  const size_t wbytes = (size_t)N * K * 2, xbytes = (size_t)16 * MT * K * 2;
  // exactly as large as what the kernel may read; the weight "image" holds, per 16-bit element, the id n K + k the packer puts there
  std::vector<uint32_t> id((size_t)N * K);
  for (int nt = 0; nt < N / 128; ++nt)
    for (int c = 0; c < nch; ++c)
      for (int r = 0; r < 128; ++r) {
        const int n = nt * 128 + (r >> 6) * 64 + lds_row_to_channel(r & 63);
        for (int j = 0; j < 8; ++j) {
          const int kslot = j ^ ((r >> 1) & 7);
          for (int k = 0; k < 8; ++k) id[(((size_t)nt * nch + c) * 128 + r) * 64 + j * 8 + k] = (uint32_t)((size_t)n * K + c * 64 + kslot * 8 + k);
        }
      }
  std::vector<uint8_t> wimg(wbytes, 1), x(xbytes, 2);
  std::vector<int> own((size_t)tiles * MT, 0), out((size_t)16 * MT * N, 0);
  long long cover = 0, bounds = 0, gemm = 0, meaning = 0;
  const TfSkinnyLaunch l = tf_skinny_launch(N, MT);
  if (l.block % 64 || l.block == 0 || l.block > 1024) ++cover;
  for (unsigned b = 0; b < l.grid; ++b)
    for (unsigned wv = 0; wv < l.block / 64; ++wv) {
      const int ft = tf_skinny_tile((int)b, (int)wv);
      if (ft < 0 || ft >= tiles) { ++cover; continue; }
      for (int tt = 0; tt < MT; ++tt) ++own[(size_t)ft * MT + tt];
      for (int lane = 0; lane < 64; ++lane) {
        const int li = lane & 15, g = lane >> 4;
        int n0 = tf_skinny_feature(ft, lane);
        if (broken & 4) n0 = ft * 16 + g * 4;
        for (int tt = 0; tt < MT; ++tt) {
          const int row = tf_skinny_x_row(tt, lane);
          if (row < 0 || row >= 16 * MT || n0 < 0 || n0 + 4 > N) { ++bounds; continue; }
          for (int q = 0; q < 4; ++q) ++out[(size_t)row * N + n0 + q];
        }
        for (int c = 0; c < nch; ++c)
          for (int ks = 0; ks < 2; ++ks) {
            size_t wo = tf_skinny_w_off(ft, c, ks, lane, nch);
            if (broken & 1) wo = (((size_t)(ft >> 3) * nch + c) * 128 + (ft & 7) * 16 + li) * 128 + (size_t)((ks * 4 + g) << 4);
            if (wo + 16 > wbytes || wo % 16) { ++bounds; continue; }
            uint8_t frag[16];
            memcpy(frag, wimg.data() + wo, 16);                          // the load itself
            if (wo != gemm_w_image_off(ft >> 3, nch, c, (ft >> 2) & 1, ft & 3, ks, lane)) ++gemm;
            // MFMA row li = 4 gq + q of the tile is feature base + 16 gq + 4 (ft & 3) + q
            const int nrow = (ft >> 3) * 128 + ((ft >> 2) & 1) * 64 + (li >> 2) * 16 + (ft & 3) * 4 + (li & 3);
            for (int j = 0; j < 8; ++j)
              if (id[wo / 2 + j] != (uint32_t)((size_t)nrow * K + c * 64 + (ks * 4 + g) * 8 + j)) ++meaning;
            for (int tt = 0; tt < MT; ++tt) {
              size_t xo = tf_skinny_x_off(tt, c, ks, lane, K);
              if ((broken & 2) && tt == 1) xo -= (size_t)8 * K * 2;
              if (xo + 16 > xbytes || xo % 16) { ++bounds; continue; }
              memcpy(frag, x.data() + xo, 16);
              if (xo != gemm_x_global_off(K, c, 0, tt, ks, lane)) ++gemm;
              if (xo != (size_t)(tt * 16 + li) * K * 2 + (size_t)(c * 64 + (ks * 4 + g) * 8) * 2) ++meaning;
            }
          }
        // the accumulator's rows are the A rows 4 g + q: feature n0 + q must be the feature of A row 4 g + q
        for (int q = 0; q < 4; ++q)
          if (n0 + q != (ft >> 3) * 128 + ((ft >> 2) & 1) * 64 + g * 16 + (ft & 3) * 4 + q) ++meaning;
      }
    }
  for (int v : own) cover += v != 1;
  for (int v : out) cover += v != 1;
  fails[0] = cover; fails[1] = bounds; fails[2] = gemm; fails[3] = meaning;
  return (int)((cover + bounds + gemm + meaning) != 0);
}

}  // extern "C"

#ifdef TF_SKINNY_MAIN
#include <stdio.h>
int main() {
  const int Ns[] = {128, 256, 384, 1152, 1536}, Ks[] = {64, 128, 256, 384, 1536};
  int shapes = 0, failures = 0;
  for (int N : Ns)
    for (int K : Ks)
      for (int MT = 1; MT <= 2; ++MT) {
        long long f[4];
        failures += tf_skinny_h_shape(N, K, MT, 0, f);
        ++shapes;
      }
  for (int M = 0; M <= 40; ++M)
    for (int bits = 0; bits < 32; ++bits) {
      const int d16 = bits & 1, sk = (bits >> 1) & 1, gen = (bits >> 2) & 1, pk = (bits >> 3) & 1, yf = (bits >> 4) & 1;
      const bool want = d16 && sk && !gen && pk && !yf && M >= 1 && M <= 32;
      failures += (tf_skinny_h_ok(d16, sk, gen, pk, yf, M) != 0) != want;
    }
  for (int M = 1; M <= 32; ++M) failures += tf_skinny_h_mt(M) != (M + 15) / 16;
  printf("%d shapes, %d failures\n", shapes, failures);
  return failures ? 1 : 0;
}
#endif
