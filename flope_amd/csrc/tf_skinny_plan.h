// The planner of option "skinny" (tf_gemm_skinny in tf_encoder.hip), in ONE place and without HIP: when launch_linear
// takes the skinny kernel, its grid and block, and which 16 bytes of the packed weight image and of the token rows a lane loads for a
// (feature tile, chunk, ks).  The kernel calls these per lane; tests/host_harness/harness_tf_skinny.cpp compiles the same definitions
// for the CPU tests (tests/test_tf_skinny_host.py).  Plain integer code, in the way tf_stream_feed.h is.  The planner of option
// "skinny_ln" (tf_gemm_skinny_ln; tests/host_harness/harness_tf_skinny_ln.cpp) is at the end of the file.
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

// ---- option "skinny_ln": the LayerNorm in front of a skinny linear inside that linear's token load (tf_gemm_skinny_ln) ----
// A wave of tf_gemm_skinny loads the whole token rows as its B operand.  With model_dim <= 64 kTfSkinnyDepth all K / 64 chunks sit in
// the register ring in front of the first MFMA, and the four lanes (li, g = 0 .. 3) of token li hold the full pre-norm row: lane g the
// 16-byte vectors v = 8 chunk + 4 ks + g (tf_skinny_x_off).  The wave normalises them in place and runs the MFMAs it runs anyway.

constexpr int kTfSkinnyLnSlots = 2 * kTfSkinnyDepth;          // (chunk, ks) pairs of a full ring: the 16-byte vectors of a row a lane holds

// launch_layernorm runs tf_layernorm_vec: 16-bit rows of whole 16-byte vectors, at most four per lane
TF_SKINNY_HD inline bool tf_ln_vec_ok(int dtype16, int d) { return dtype16 && d % 8 == 0 && d <= 2048; }

// A LayerNorm over N_of_ln (= model_dim) columns directly in front of a linear of K (padded Kp) columns is folded into that linear's
// launch exactly where the linear is a skinny one (skinny_ok = tf_skinny_ok(...) of the consumer: a 16-bit handle), option "skinny_ln"
// is 1, the linear reads the normalised rows as they are (Kp == K == model_dim), the whole row sits in the ring (whole chunks, at most
// kTfSkinnyDepth of them: one tf_layernorm_vec vector per lane of ITS wave, the tree below) and the stand-alone launch would be
// tf_layernorm_vec, whose bits the fold returns
TF_SKINNY_HD inline bool tf_skinny_ln_ok(bool skinny_ok, int opt_skinny_ln, int K, int Kp, int N_of_ln) {
  return skinny_ok && opt_skinny_ln == 1 && Kp == K && K == N_of_ln && N_of_ln % 64 == 0 && N_of_ln >= 64 &&
         N_of_ln <= 64 * kTfSkinnyDepth && tf_ln_vec_ok(1, N_of_ln);
}

// ring slot of (chunk, ks), and the index of the 16-byte vector of its row that lane group g holds there: tf_layernorm_vec's lane
TF_SKINNY_HD inline int tf_skinny_ln_slot(int chunk, int ks) { return (chunk << 1) | ks; }
TF_SKINNY_HD inline int tf_skinny_ln_vec(int slot, int g) { return (slot << 2) | g; }

// tf_layernorm_vec sums its per-vector partials by wave_sum: xor 32, 16, 8, 4, 2, 1 over the vector index, bit 5 first.  Bits 5 .. 2 of
// the vector index are the slot and stay in the lane, bits 1 .. 0 are g = lane bits 5 .. 4.  The same tree in three steps:
//   in the lane   steps 0 .. 3 combine slot s with slot s + tf_skinny_ln_tree_off(step) (8, 4, 2, 1), every slot of the FULL ring taking
//                 part: a slot at or past K / 64 chunks counts as 0.f, which is what the lanes past d / 8 hold in tf_layernorm_vec;
//   across lanes  += the lane at xor tf_skinny_ln_lane_xor(0) = 32, then at xor tf_skinny_ln_lane_xor(1) = 16 (the same token, g ^ 2, g ^ 1).
constexpr int kTfSkinnyLnTreeSteps = 4;
TF_SKINNY_HD inline int tf_skinny_ln_tree_off(int step) { return (kTfSkinnyLnSlots / 2) >> step; }
TF_SKINNY_HD inline int tf_skinny_ln_lane_xor(int step) { return 32 >> step; }
// the in-lane part over p[kTfSkinnyLnSlots] (overwritten); the sum of the lane's vectors in tree order
TF_SKINNY_HD inline float tf_skinny_ln_lane_tree(float* p) {
#pragma unroll
  for (int st = 0; st < kTfSkinnyLnTreeSteps; ++st) {
    const int o = tf_skinny_ln_tree_off(st);
#pragma unroll
    for (int s = 0; s < kTfSkinnyLnSlots / 2; ++s)
      if (s < o) p[s] = p[s] + p[s + o];
  }
  return p[0];
}

// The post-norm rows H [16 MT][d]: every wave holds all of them, so the store is shared out by chunk -- wave (feature tile) ft stores the
// 64 columns of chunk ft from its own fragments, or nothing where ft >= K / 64 (N / 16 >= 8 >= K / 64 waves exist).  Returns that chunk or -1
TF_SKINNY_HD inline int tf_skinny_ln_h_chunk(int ft, int nch) { return ft >= 0 && ft < nch ? ft : -1; }
// ... and the byte offset into H of the 16 bytes lane `lane` stores for (token tile, chunk, ks): where it loaded them from in X
TF_SKINNY_HD inline size_t tf_skinny_ln_h_off(int tt, int chunk, int ks, int lane, int d) { return tf_skinny_x_off(tt, chunk, ks, lane, d); }
// the first of the 8 columns of gamma / beta a lane needs for (chunk, ks): the columns of its vector
TF_SKINNY_HD inline int tf_skinny_ln_col(int chunk, int ks, int lane) { return tf_skinny_ln_vec(tf_skinny_ln_slot(chunk, ks), lane >> 4) * 8; }

}  // namespace flope_tf_plan
