// The planner of option "skinny" (tf_gemm_skinny in tf_encoder.hip), in ONE place and without HIP: when launch_linear
// takes the skinny kernel, its grid and block, and which 16 bytes of the packed weight image and of the token rows a lane loads for a
// (feature tile, chunk, ks).  The kernel calls these per lane; tests/host_harness/harness_tf_skinny.cpp compiles the same definitions
// for the CPU tests (tests/test_tf_skinny_host.py).  Plain integer code, in the way tf_stream_feed.h is.
//
// The weight image is tf_gemm_mfma's and is read where it lies (pack_linear): [N / 128 tiles][K / 64 chunks][128 rows][128 B], the
// 16-byte slot j of row r holding k-slot j ^ ((r >> 1) & 7) of the chunk, and row 64 h + 16 ct + 4 g + q of a tile holding feature
// 64 h + 16 g + 4 ct + q.  A FEATURE TILE ft is 16 consecutive rows of that image: rows 16 (ft & 7) .. + 15 of tile ft >> 3.  It is the
// A operand of one v_mfma_f32_16x16x32 -- the rows tf_gemm_mfma's wave wn = (ft >> 2) & 1 reads as its fragment ct = ft & 3 -- so lane
// (li = lane & 15, g = lane >> 4) ends with features tf_skinny_feature(ft, lane) .. + 3 of token li of each of its token tiles.
// A wave owns one feature tile and the MT token tiles of 16 rows; nothing is shared between waves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef TF_SKINNY_HD
#if defined(__HIPCC__)
#define TF_SKINNY_HD __host__ __device__
#else
#define TF_SKINNY_HD
#endif
#endif

namespace flope_tf_plan {

constexpr int kTfSkinnyMaxRows = 32;                // M above it keeps tf_gemm_mfma
constexpr int kTfSkinnyWaves = 1;                   // waves (feature tiles) per workgroup: N / 16 workgroups of one wave
constexpr int kTfSkinnyDepth = 8;                   // chunks of 64 k a wave keeps in flight in front of their MFMAs (a register ring)

// launch_linear runs tf_gemm_skinny exactly where it would run tf_gemm_mfma (a 16-bit handle, a packed image, a 16-bit result, option
// "generic" off), option "skinny" is 1 and 1 <= M <= 32
TF_SKINNY_HD inline bool tf_skinny_ok(int dtype16, int opt_skinny, int opt_generic, int packed, int y_f32, int M) {
  return dtype16 && packed && !y_f32 && !opt_generic && opt_skinny == 1 && M >= 1 && M <= kTfSkinnyMaxRows;
}

// token tiles of 16 rows
TF_SKINNY_HD inline int tf_skinny_mt(int M) { return M <= 16 ? 1 : 2; }

struct TfSkinnyLaunch { unsigned grid, block; };
// N % 128 == 0, so N / 16 is a multiple of 8 and of kTfSkinnyWaves
TF_SKINNY_HD inline TfSkinnyLaunch tf_skinny_launch(int N, int MT) {
  (void)MT;                                         // a wave walks its token tiles itself
  TfSkinnyLaunch l;
  l.grid = (unsigned)(N / 16 / kTfSkinnyWaves);
  l.block = 64u * kTfSkinnyWaves;
  return l;
}
// the feature tile of wave `wave` of workgroup `block`
TF_SKINNY_HD inline int tf_skinny_tile(int block, int wave) { return block * kTfSkinnyWaves + wave; }

// byte offset into the packed image of the 16 bytes lane `lane` loads as its A fragment of (feature tile, chunk, ks); nch = Kp / 64
TF_SKINNY_HD inline size_t tf_skinny_w_off(int ft, int chunk, int ks, int lane, int nch) {
  const int li = lane & 15, g = lane >> 4, r = (ft & 7) * 16 + li;
  return (((size_t)(ft >> 3) * nch + chunk) * 128 + r) * 128 + (size_t)(((ks * 4 + g) ^ ((r >> 1) & 7)) << 4);
}

// the token row of lane `lane` in token tile tt, and the byte offset into X [rows][Kp] of its B fragment of (chunk, ks)
TF_SKINNY_HD inline int tf_skinny_x_row(int tt, int lane) { return tt * 16 + (lane & 15); }
TF_SKINNY_HD inline size_t tf_skinny_x_off(int tt, int chunk, int ks, int lane, int Kp) {
  return (size_t)tf_skinny_x_row(tt, lane) * Kp * 2 + (size_t)chunk * 128 + (size_t)((ks * 4 + (lane >> 4)) << 4);
}

// the first of the four consecutive features lane `lane` holds for feature tile ft (accumulator element q is feature + q)
TF_SKINNY_HD inline int tf_skinny_feature(int ft, int lane) {
  return (ft >> 3) * 128 + ((ft >> 2) & 1) * 64 + (lane >> 4) * 16 + (ft & 3) * 4;
}

}  // namespace flope_tf_plan
