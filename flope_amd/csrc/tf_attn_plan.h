// Which attention kernel one encoder launch takes, and the LDS bytes it is launched with -- plain integer arithmetic, no HIP,
// shared by tf_encoder.hip (launch_attention: flope_tf_forward and flope_tf_attention) and tests/host_harness/harness_tf_attn.cpp
// (tests/test_tf_attn_plan_host.py checks the table on the CPU, tests/test_gpu_tf_attn_tiled.py the device against it).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/flope_amd.h"

// ids flope_tf_attention returns
enum {
  FLOPE_TF_ATTN_GENERIC = 0,   // tf_attn_generic: any shape, vector ALU
  FLOPE_TF_ATTN_MFMA64 = 1,    // tf_attn_mfma: 16-bit, head_dim 64, all keys of a head resident in LDS (padded seq_len <= 512)
  FLOPE_TF_ATTN_TILED = 2,     // tf_attn_tiled: 16-bit, head_dim 32 / 64 / 96 / 128, any seq_len (option attn_tiled)
  FLOPE_TF_ATTN_F32M = 3       // tf_attn_f32m: float32 on v_mfma_f32_16x16x4_f32 (option f32mfma)
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

}  // namespace flope_tf_plan
