// The encoder's architecture, stated ONCE and without HIP: which ops a forward runs for (norm_first, activation,
// final_norm) and a layer count, in which order, and which buffer each op reads, adds as its residual and writes.  run_forward_with
// (tf_encoder.hip) walks this list -- step, extend, prefill and every forward with it --, and tests/host_harness/harness_tf_arch.cpp
// compiles the same definitions for the CPU tests (tests/test_tf_arch_host.py).  Plain integer code, in the way tf_skinny_plan.h is.
//
// With S the residual stream:
//   post-norm (torch's default)   S = LN1(S + out_proj(att(in_proj(S)))),  S = LN2(S + linear2(act(linear1(S))))
//   pre-norm  (norm_first)        S = S + out_proj(att(in_proj(LN1(S)))),  S = S + linear2(act(linear1(LN2(S))))
//   then LN_final(S) if final_norm, then out_layer.
// Buffers: the stream enters every layer in H.
//   post-norm   in_proj(H) -> QKV, attention -> ATT, out_proj(ATT, res H) -> H2, LN1(H2) -> H, linear1(H) -> FFB,
//               linear2(FFB, res H) -> H2, LN2(H2) -> H.  (The LayerNorm H2 -> H of layer l is listed in front of what reads it.)
//   pre-norm    LN1(H) -> H2, in_proj(H2) -> QKV, attention -> ATT, out_proj(ATT, res H) -> H2 (the stream is now in H2),
//               LN2(H2) -> H, linear1(H) -> FFB, linear2(FFB, res H2) -> H.  The residual is always the un-normalised stream.
//   final norm  LN_final(H) -> H2, out_layer(H2); without it out_layer(H).
// No op's output is its input or its residual.
#pragma once
#include "tf_act.h"

#ifndef TF_ARCH_HD
#if defined(__HIPCC__)
#define TF_ARCH_HD __host__ __device__
#else
#define TF_ARCH_HD
#endif
#endif

namespace flope_tf_plan {

struct TfArch { int norm_first; int act; int final_norm; };

TF_ARCH_HD inline bool tf_arch_valid(const TfArch& a) {
  return (a.norm_first == 0 || a.norm_first == 1) && (a.act == FLOPE_TF_ACT_RELU || a.act == FLOPE_TF_ACT_GELU) && (a.final_norm == 0 || a.final_norm == 1);
}
// torch's nn.TransformerEncoderLayer defaults: what every handle is until told otherwise, and the only architecture of tf_fused_f32
TF_ARCH_HD inline bool tf_arch_default(const TfArch& a) { return a.norm_first == 0 && a.act == FLOPE_TF_ACT_RELU && a.final_norm == 0; }

enum TfOpKind { kTfOpLinear = 0, kTfOpLayerNorm = 1, kTfOpAttention = 2 };
enum TfOpName {
  kTfLinEmbedding = 0, kTfLinInProj = 1, kTfLinOutProj = 2, kTfLinLinear1 = 3, kTfLinLinear2 = 4, kTfLinOutLayer = 5,
  kTfLnNorm1 = 6, kTfLnNorm2 = 7, kTfLnFinal = 8, kTfAttn = 9
};
enum TfBuf { kTfBufNone = 0, kTfBufX = 1, kTfBufH = 2, kTfBufH2 = 3, kTfBufQkv = 4, kTfBufAtt = 5, kTfBufFfb = 6, kTfBufY = 7 };

struct TfOp {
  int kind;       // TfOpKind
  int name;       // TfOpName
  int layer;      // whose weights: 0 .. num_layers - 1, -1 for embedding, out_layer and the final norm
  int in, res, out;   // TfBuf
  int act;        // FLOPE_TF_ACT_*: linears only
  int fold;       // a LayerNorm: 1 = the next op is a linear of K = model_dim that reads its output, the pair option skinny_ln may run as one launch
};

// ops of a forward: embedding, 7 per layer, the final norm, out_layer
TF_ARCH_HD inline int tf_arch_op_count(const TfArch& a, int num_layers) { return 2 + 7 * num_layers + (a.final_norm ? 1 : 0); }

TF_ARCH_HD inline TfOp tf_arch_mk(int kind, int name, int layer, int in, int res, int out, int act, int fold) {
  TfOp o;
  o.kind = kind; o.name = name; o.layer = layer; o.in = in; o.res = res; o.out = out; o.act = act; o.fold = fold;
  return o;
}

// op i of the forward, 0 <= i < tf_arch_op_count
TF_ARCH_HD inline TfOp tf_arch_op(const TfArch& a, int num_layers, int i) {
  const int N = FLOPE_TF_ACT_NONE;
  if (i == 0) return tf_arch_mk(kTfOpLinear, kTfLinEmbedding, -1, kTfBufX, kTfBufNone, kTfBufH, N, 0);
  const int body = 1 + 7 * num_layers;
  if (i >= body) {
    if (a.final_norm && i == body) return tf_arch_mk(kTfOpLayerNorm, kTfLnFinal, -1, kTfBufH, kTfBufNone, kTfBufH2, N, 0);   // never folded
    return tf_arch_mk(kTfOpLinear, kTfLinOutLayer, -1, a.final_norm ? kTfBufH2 : kTfBufH, kTfBufNone, kTfBufY, N, 0);
  }
  const int l = (i - 1) / 7, s = (i - 1) % 7;
  if (a.norm_first) {
    switch (s) {
      case 0: return tf_arch_mk(kTfOpLayerNorm, kTfLnNorm1, l, kTfBufH, kTfBufNone, kTfBufH2, N, 1);
      case 1: return tf_arch_mk(kTfOpLinear, kTfLinInProj, l, kTfBufH2, kTfBufNone, kTfBufQkv, N, 0);
      case 2: return tf_arch_mk(kTfOpAttention, kTfAttn, l, kTfBufQkv, kTfBufNone, kTfBufAtt, N, 0);
      case 3: return tf_arch_mk(kTfOpLinear, kTfLinOutProj, l, kTfBufAtt, kTfBufH, kTfBufH2, N, 0);
      case 4: return tf_arch_mk(kTfOpLayerNorm, kTfLnNorm2, l, kTfBufH2, kTfBufNone, kTfBufH, N, 1);
      case 5: return tf_arch_mk(kTfOpLinear, kTfLinLinear1, l, kTfBufH, kTfBufNone, kTfBufFfb, a.act, 0);
      default: return tf_arch_mk(kTfOpLinear, kTfLinLinear2, l, kTfBufFfb, kTfBufH2, kTfBufH, N, 0);
    }
  }
  // post-norm: a layer's seven ops are in_proj .. linear2 and its LN2; LN2 of layer l stands in front of layer l + 1's in_proj (folded
  // with it) or, behind the last layer, in front of the final norm or out_layer (a launch of its own)
  switch (s) {
    case 0: return tf_arch_mk(kTfOpLinear, kTfLinInProj, l, kTfBufH, kTfBufNone, kTfBufQkv, N, 0);
    case 1: return tf_arch_mk(kTfOpAttention, kTfAttn, l, kTfBufQkv, kTfBufNone, kTfBufAtt, N, 0);
    case 2: return tf_arch_mk(kTfOpLinear, kTfLinOutProj, l, kTfBufAtt, kTfBufH, kTfBufH2, N, 0);
    case 3: return tf_arch_mk(kTfOpLayerNorm, kTfLnNorm1, l, kTfBufH2, kTfBufNone, kTfBufH, N, 1);
    case 4: return tf_arch_mk(kTfOpLinear, kTfLinLinear1, l, kTfBufH, kTfBufNone, kTfBufFfb, a.act, 0);
    case 5: return tf_arch_mk(kTfOpLinear, kTfLinLinear2, l, kTfBufFfb, kTfBufH, kTfBufH2, N, 0);
    default: return tf_arch_mk(kTfOpLayerNorm, kTfLnNorm2, l, kTfBufH2, kTfBufNone, kTfBufH, N, l + 1 < num_layers ? 1 : 0);
  }
}

// Option skinny_ln where tf_skinny_ln_ok takes every candidate: the LayerNorms that run inside the next linear's launch, and the
// stand-alone launches left (what flope_tf_last_ln reports).  Post-norm: 2 L - 1 folded, the last LN2 launched; pre-norm: all 2 L
// folded; the final norm is always a launch.
TF_ARCH_HD inline int tf_arch_ln_folded(const TfArch& a, int num_layers) {
  int n = 0;
  for (int i = 0; i < tf_arch_op_count(a, num_layers); ++i) n += tf_arch_op(a, num_layers, i).fold;
  return n;
}
TF_ARCH_HD inline int tf_arch_ln_launched(const TfArch& a, int num_layers) {
  return 2 * num_layers + (a.final_norm ? 1 : 0) - tf_arch_ln_folded(a, num_layers);
}

}  // namespace flope_tf_plan
