// The single-launch float32 forward of the encoder (option "fused"): where one sequence's buffers lie in a
// workgroup's LDS, which summation order a linear takes, and when a forward is eligible -- plain integer arithmetic, no HIP,
// shared by tf_encoder.hip (tf_fused_f32 and its dispatch in flope_tf_forward / flope_tf_forward_varlen / flope_tf_forward_plan)
// and tests/host_harness/harness_tf_fused.cpp (tests/test_tf_fused_host.py walks the forward through these offsets on the CPU).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/flope_amd.h"

namespace flope_tf_plan {

constexpr size_t kTfFusedLds = 64 * 1024;    // what a launch gets without a function attribute; leaves two workgroups per CU
constexpr int kTfFusedWaves = 4;             // tf_fused_f32: 256 threads; one score row per wave

// Byte offsets of one sequence's buffers from the start of the workgroup's dynamic LDS, all rows of floats.  A function of
// (in_dim, d, ff, L) only; L is the longest sequence of the call (a shorter one uses the head of every buffer).
//   h, h2   [L][d]         the residual stream and the pre-LayerNorm sum: live across phases, never aliased
//   one region, three tenants:
//     x     [L][in_dim]    the input rows                                   load .. embedding
//     qkv   [L][qkv_ld] | att [L][d] | sc [waves][L]                        in_proj .. out_proj
//     ffb   [L][ff]        the feed-forward activations                     linear1 .. linear2
// qkv_ld = 3 d rounded up to odd: lane j of an attention wave reads key row j, and an odd row stride spreads the rows over the banks.
// Weights are read through L2, so no bytes are staged for them.
struct TfFusedLayout {
  uint32_t h, h2, x, qkv, att, sc, ffb;      // byte offsets
  uint32_t qkv_ld, sc_ld;                    // row strides in floats
  uint64_t total;                            // bytes of dynamic LDS
};

inline TfFusedLayout tf_fused_layout(int in_dim, int d, int ff, int L) {
  const uint64_t l = (uint64_t)(L > 0 ? L : 0), qld = (uint64_t)3 * d | 1;
  const uint64_t hs = l * d, xs = l * in_dim, qs = l * qld, as = l * d, ss = (uint64_t)kTfFusedWaves * l, fs = l * ff;
  uint64_t region = xs;
  if (qs + as + ss > region) region = qs + as + ss;
  if (fs > region) region = fs;
  TfFusedLayout o;
  const uint64_t r0 = 2 * hs;                // floats
  o.total = (r0 + region) * sizeof(float);
  // offsets are meaningful only where total fits 32 bits (an ineligible shape is never launched); saturate instead of wrapping
  auto off = [](uint64_t floats) { const uint64_t b = floats * sizeof(float); return (uint32_t)(b > 0xffffffffull ? 0xffffffffull : b); };
  o.h = 0; o.h2 = off(hs);
  o.x = off(r0); o.qkv = off(r0); o.att = off(r0 + qs); o.sc = off(r0 + qs + as); o.ffb = off(r0);
  o.qkv_ld = (uint32_t)qld; o.sc_ld = (uint32_t)l;
  return o;
}

// The rule by which the float32 launch sequence sends a linear to tf_linear_rowwave (lane-strided k, butterfly sum) instead of
// tf_linear_generic (one fmaf chain): launch_linear in tf_encoder.hip.
constexpr bool tf_fused_rowwave_order(int N, int has_residual) { return N <= 16 && !has_residual; }

// dtype: FLOPE_DT_*; opt_fused, opt_f32m: the handle's options "fused" and "f32mfma"; L_longest: seq_len of a fixed-length forward, the
// longest length of a ragged one.  No alignment condition: the kernel reads x and writes y as plain floats.
inline bool tf_fused_ok(int dtype, int opt_fused, int opt_f32m, int in_dim, int d, int ff, int L_longest) {
  if (dtype != FLOPE_DT_F32 || opt_fused != 1 || opt_f32m != 0 || L_longest < 1) return false;
  return tf_fused_layout(in_dim, d, ff, L_longest).total <= kTfFusedLds;
}

}  // namespace flope_tf_plan
