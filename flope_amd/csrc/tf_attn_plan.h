// Which attention kernel one encoder launch takes, and the LDS bytes it is launched with -- plain integer arithmetic, no HIP,
// shared by tf_encoder.hip (launch_attention: flope_tf_forward and flope_tf_attention) and tests/host_harness/harness_tf_attn.cpp
// (tests/test_tf_attn_plan_host.py checks the table on the CPU, tests/test_gpu_tf_attn_tiled.py the device against it).
// Below it, the planner of ragged batches (launch_attention_varlen and the flope_tf_*_varlen entry points;
// tests/host_harness/harness_tf_varlen.cpp, tests/test_tf_varlen_host.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/flope_amd.h"

// ids flope_tf_attention returns
enum {
  FLOPE_TF_ATTN_GENERIC = 0,   // tf_attn_generic: any shape, vector ALU
  FLOPE_TF_ATTN_MFMA64 = 1,    // tf_attn_mfma: 16-bit, head_dim 64, all keys of a head resident in LDS (padded seq_len <= 512)
  FLOPE_TF_ATTN_TILED = 2,     // tf_attn_tiled: 16-bit, head_dim 32 / 64 / 96 / 128, any seq_len (option attn_tiled)
  FLOPE_TF_ATTN_F32M = 3,      // tf_attn_f32m: float32 on v_mfma_f32_16x16x4_f32 (option f32mfma)
  FLOPE_TF_ATTN_MASKED = 4,    // tf_attn_masked: any shape under a compiled mask (flope_tf_attention_masked; tf_attn_mask.h)
  FLOPE_TF_ATTN_MASKED16 = 5,  // tf_attn_tiled_masked: 16-bit, head_dim 32 / 64 / 96 / 128 under a compiled mask (option mask_mfma; tf_attn_mask.h)
  FLOPE_TF_ATTN_BIASED16 = 7,  // tf_attn_tiled_masked, BIASED: 16-bit, head_dim 32 / 64 / 96 / 128 under a compiled bias (option bias_mfma; tf_attn_mask.h)
  FLOPE_TF_ATTN_BIASED = 6     // tf_attn_masked, BIASED: any shape under a compiled additive bias (flope_tf_bias_create; tf_attn_mask.h)
};

namespace flope_tf_plan {

constexpr size_t kTfAttnLds = 160 * 1024;    // tf_attn_f32m: the most LDS a launch may ask for
constexpr int kTfAttnMfma64MaxLp = 512;      // tf_attn_mfma: 256 bytes of LDS per key (K row + V row)
constexpr int kTfAttnTiledKB = 64;           // tf_attn_tiled: keys per streamed block (two 32-key steps)
constexpr int kTfAttnTiledRing = 2;          // ... blocks the LDS ring holds
constexpr int kTfAttnTiledQueries = 128;     // ... queries per workgroup (4 waves x 32)

inline int tf_attn_pad32(int seq_len) { return (seq_len + 31) / 32 * 32; }

// tf_attn_mfma: K image [Lp][128 B] | V image [Lp][128 B]
inline size_t tf_attn_mfma64_lds(int seq_len) { return (size_t)tf_attn_pad32(seq_len) * 256; }

// tf_attn_f32m: 16-wide tiles of head_dim the kernel is built for, and 16 score rows + the partial outputs of three waves
inline int tf_attn_f32m_nt(int head_dim) { return head_dim <= 16 ? 1 : head_dim <= 32 ? 2 : head_dim <= 64 ? 4 : 8; }
inline size_t tf_attn_f32m_lds(int head_dim, int seq_len) {
  return ((size_t)16 * (((seq_len + 15) & ~15) + 4) + (size_t)3 * tf_attn_f32m_nt(head_dim) * 256) * sizeof(float);
}

// tf_attn_tiled: ring of (K block | V block), rows of 2 * head_dim bytes: 16 / 32 / 48 / 64 KiB for head_dim 32 / 64 / 96 / 128
inline size_t tf_attn_tiled_lds(int head_dim) { return (size_t)kTfAttnTiledRing * 2 * kTfAttnTiledKB * head_dim * 2; }
inline bool tf_attn_tiled_ok(int head_dim) { return head_dim > 0 && head_dim % 32 == 0 && head_dim <= 128; }

// dtype: FLOPE_DT_*; opt_*: the handle's options "generic", "f32mfma", "attn_tiled"; aligned16: qkv and out are 16-byte aligned
// (every kernel but the generic one moves 8- or 16-byte vectors).
inline int tf_attn_pick(int dtype, int head_dim, int seq_len, int opt_generic, int opt_f32m, int opt_tiled, int aligned16) {
  if (!aligned16) return FLOPE_TF_ATTN_GENERIC;
  if (dtype == FLOPE_DT_F32) {                 // ("generic" and "attn_tiled" are stored and ignored)
    if (opt_f32m && head_dim % 4 == 0 && head_dim <= 128 && tf_attn_f32m_lds(head_dim, seq_len) <= kTfAttnLds) return FLOPE_TF_ATTN_F32M;
    return FLOPE_TF_ATTN_GENERIC;
  }
  if (opt_generic) return FLOPE_TF_ATTN_GENERIC;
  int pick = FLOPE_TF_ATTN_GENERIC;
  if (head_dim == 64 && tf_attn_pad32(seq_len) <= kTfAttnMfma64MaxLp) pick = FLOPE_TF_ATTN_MFMA64;
  if (tf_attn_tiled_ok(head_dim) && (opt_tiled == 2 || (opt_tiled == 1 && pick == FLOPE_TF_ATTN_GENERIC))) pick = FLOPE_TF_ATTN_TILED;
  return pick;
}

// ---- causal attention (option "causal") ------------------------------------------------------------------------------
// Query i attends to keys j <= i of its own sequence of L tokens.  Kernel choice, grid, block and LDS above and below do not depend on
// the option; what depends on it is how far a query group walks the keys.  The kernels call these, and so does
// tests/host_harness/harness_tf_causal.cpp (tests/test_tf_causal_host.py holds them against brute force).
// Keys visible to the group of nq queries that starts at query q_first: keys 0 .. min(L, q_first + nq) - 1
constexpr int tf_causal_keys(int q_first, int nq, int L) { return q_first + nq < L ? q_first + nq : L; }
// tf_attn_tiled: 64-key blocks the workgroup of query block qblock walks (every wave of it: one trip count, one barrier count)
constexpr int tf_causal_tiled_blocks(int qblock, int L) {
  return (tf_causal_keys(qblock * kTfAttnTiledQueries, kTfAttnTiledQueries, L) + kTfAttnTiledKB - 1) / kTfAttnTiledKB;
}
// tf_attn_tiled / tf_attn_mfma: whether the wave whose 32 queries start at q0 takes the 32-key step that starts at key kb
constexpr bool tf_causal_step_taken(int q0, int kb) { return kb <= q0 + 31; }
// tf_attn_f32m: 16-key tiles the workgroup of queries q0 .. q0 + 15 walks in its score and value passes
constexpr int tf_causal_f32m_tiles(int q0, int L) { return (tf_causal_keys(q0, 16, L) + 15) / 16; }

// ---- sliding-window causal attention (option "window") ------------------------------------------------------------------
// With causal and a window W >= 1, query i attends to keys i - W < j <= i of its own sequence; W = 0: no window.  First visible key
// of query i: max(0, i + 1 - W).  tf_attn_row, tf_attn_stream_row and tests/host_harness/harness_tf_window.cpp call this
// (tests/test_tf_window_host.py holds it against brute force); the last visible key stays tf_causal_keys(i, 1, L) - 1 = i.
constexpr int tf_window_lo(int i, int W) { return W > 0 && i >= W ? i - W + 1 : 0; }
// ... and how many keys that is: min(i + 1, W), i + 1 without a window
constexpr int tf_window_keys(int i, int W) { return i - tf_window_lo(i, W) + 1; }

// ---- the window on the 16-bit MFMA kernels (option "window_mfma") ---------------------------------------------------------
// tf_attn_mfma / tf_attn_tiled walk 32-key steps; under a window a wave also leaves out the steps that lie wholly below the window of
// its FIRST query (the lowest window of the wave).  The kernels call these, and so does tests/host_harness/harness_tf_window16.cpp
// (tests/test_tf_window16_host.py holds them against brute force).
// First 32-key step the wave of queries q0 .. q0 + 31 takes: the one that holds the first visible key of query q0; 0 for W = 0
constexpr int tf_window_first_step(int q0, int W) { return tf_window_lo(q0, W) & ~31; }
// ... whether that wave takes the step that starts at key kb: not above its last query, not wholly below its first query's window
constexpr bool tf_window_step_taken(int q0, int kb, int W) { return tf_causal_step_taken(q0, kb) && kb + 31 >= tf_window_lo(q0, W); }
// tf_attn_tiled: first 64-key block the workgroup of query block qblock loads (its first wave's first step lies in it); the last
// stays tf_causal_tiled_blocks(qblock, L) - 1
constexpr int tf_window_tiled_first_block(int qblock, int W) { return tf_window_lo(qblock * kTfAttnTiledQueries, W) / kTfAttnTiledKB; }
// The pick under causal with a window: tf_attn_pick's where the option is set and that kernel has a WINDOW instantiation
// (tf_attn_mfma, tf_attn_tiled), the generic kernel otherwise -- option 0, float32 (tf_attn_f32m has none), misaligned pointers
inline int tf_attn_pick_window(int dtype, int head_dim, int seq_len, int opt_generic, int opt_f32m, int opt_tiled, int opt_window_mfma,
                               int aligned16) {
  if (!opt_window_mfma) return FLOPE_TF_ATTN_GENERIC;
  const int pick = tf_attn_pick(dtype, head_dim, seq_len, opt_generic, opt_f32m, opt_tiled, aligned16);
  return pick == FLOPE_TF_ATTN_MFMA64 || pick == FLOPE_TF_ATTN_TILED ? pick : (int)FLOPE_TF_ATTN_GENERIC;
}

// ---- ragged batches (flope_tf_forward_varlen / flope_tf_attention_varlen) ------------------------------------------
// A batch of B sequences of lengths[b] tokens (1 <= lengths[b] <= L) lives in the handle as T = sum lengths packed rows;
// sequence b starts at packed row off[b], off[B] = T.
enum {
  kTfVarlenOk = 0,
  kTfVarlenBatch = -1,      // B <= 0 (or a NULL table)
  kTfVarlenLength = -2,     // a length < 1 or > L; *bad = its index
  kTfVarlenTokens = -3,     // T > max_tokens
  kTfVarlenOverflow = -4    // T does not fit an int
};

// off: B + 1 ints.  On kTfVarlenOk: off, *T and *max_len are written; otherwise nothing but *bad (kTfVarlenLength) is.
inline int tf_varlen_plan(const int* lengths, int B, int L, int max_tokens, int* off, int* T, int* max_len, int* bad) {
  if (B <= 0 || !lengths || !off) return kTfVarlenBatch;
  long long sum = 0;
  int mx = 0;
  for (int b = 0; b < B; ++b) {
    if (lengths[b] < 1 || lengths[b] > L) {
      if (bad) *bad = b;
      return kTfVarlenLength;
    }
    sum += lengths[b];
    if (lengths[b] > mx) mx = lengths[b];
  }
  if (sum > (long long)INT32_MAX) return kTfVarlenOverflow;
  if (sum > (long long)max_tokens) return kTfVarlenTokens;
  int run = 0;
  for (int b = 0; b < B; ++b) { off[b] = run; run += lengths[b]; }
  off[B] = run;
  if (T) *T = run;
  if (max_len) *max_len = mx;
  return kTfVarlenOk;
}

// Grid, block and dynamic LDS of the variable-length launch of kernel `which` (FLOPE_TF_ATTN_*): sized by the longest sequence of
// the batch; a workgroup past its own sequence's length leaves at once.
struct TfAttnLaunch { unsigned grid_x, grid_y, block; size_t lds; };
inline TfAttnLaunch tf_attn_varlen_launch(int which, int head_dim, int B, int H, int max_len) {
  TfAttnLaunch l = {(unsigned)B * (unsigned)H, 1u, 256u, 0};
  switch (which) {
    case FLOPE_TF_ATTN_MFMA64:
      l.block = (unsigned)(tf_attn_pad32(max_len) / 32 * 64);
      l.lds = tf_attn_mfma64_lds(max_len);
      break;
    case FLOPE_TF_ATTN_TILED:
      l.grid_y = (unsigned)((max_len + kTfAttnTiledQueries - 1) / kTfAttnTiledQueries);
      l.lds = tf_attn_tiled_lds(head_dim);
      break;
    case FLOPE_TF_ATTN_F32M:
      l.grid_y = (unsigned)((max_len + 15) / 16);
      l.lds = tf_attn_f32m_lds(head_dim, max_len);
      break;
    default: {                                   // generic: four waves, one query each per trip, at most 64 workgroups per head
      const int gy = (max_len + 3) / 4;
      l.grid_y = (unsigned)(gy < 64 ? gy : 64);
      l.lds = (size_t)4 * max_len * sizeof(float);
    }
  }
  return l;
}

}  // namespace flope_tf_plan
