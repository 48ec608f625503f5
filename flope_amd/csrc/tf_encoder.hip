// TransformerEncoder of the reference (scripts/tf_encoder.py:5-27) on gfx950, behind the C-ABI
// flope_tf_* of include/flope_amd.h:
//     embedding Linear(in, d)  ->  L x post-norm TransformerEncoderLayer(d, heads, ff, ReLU, batch_first)
//     ->  out_layer Linear(d, out);   eval-mode semantics (dropout = identity), no mask, no positions.
// Two arithmetic modes share one launch sequence:
//   FLOPE_DT_F32          every op in fp32 on the vector ALU (any dimensions; pins the reference's toy fixture)
//     option f32mfma = 1  the same buffers and launches, linears with K % 4 == 0 on tf_linear_f32m and attention with
//                         head_dim % 4 == 0 (<= 128) on tf_attn_f32m: v_mfma_f32_16x16x4_f32, exact float32, another summation order
//   FLOPE_DT_F16 / BF16   activations in HBM as 16-bit row-major [tokens][features];
//                         linears whose (N % 128 == 0, K % 64 == 0) run on v_mfma_f32_16x16x32 (tf_gemm_mfma),
//                         attention with head_dim 64 and at most 512 keys runs on MFMA with the softmax in registers (tf_attn_mfma);
//     option attn_tiled   head_dim 32 / 64 / 96 / 128 at any length on the streaming form of that kernel (tf_attn_tiled);
//                         everything else (embedding, out_layer, odd shapes) falls to the generic kernels.
// Bias, residual add and ReLU live in the linear kernels' epilogues; LayerNorm is one wave per token row.
// FLOPE_DT_F32 with option fused = 1: a forward whose longest sequence fits 64 KiB of LDS is ONE launch (tf_fused_f32), same bits.
// Option causal = 1 (any dtype): query i attends to keys j <= i of its own sequence -- the CAUSAL instantiation of whichever attention
// kernel the shape picks, and of tf_fused_f32; key blocks above the diagonal are skipped, not loaded and masked.
// Option window = W > 0 (with causal, any dtype): query i attends to keys i - W < j <= i -- tf_attn_generic's WINDOW instantiation for every
// shape, the keys below the window not loaded either; never the single launch.  Option window_mfma = 1: a 16-bit launch
// keeps tf_attn_mfma / tf_attn_tiled under a window, their WINDOW instantiations.
// flope_tf_stream_* (any dtype): one new token per track instead of the causal forward again -- the same launch sequence at one row per
// track, with tf_attn_step over a per-track cache of every layer's keys and values where the forward has its attention kernel
// (the checks and launch shapes are in tf_encoder_stream.h).  flope_tf_stream_open_window: the same over a ring cache
// with sliding-window attention, never full.
// flope_tf_stream_open_bias: a state with a distance table [planes][D], a relative bias such as ALiBi -- step, extend and
// prefill run the BIASED instantiations of tf_attn_step / tf_attn_extend, the bits of the forward under the expanded compiled bias.
// flope_tf_stream_extend: several tokens per track and call behind what the track holds -- the ragged launch sequence over the packed
// chunks with tf_attn_extend over cache and chunk, tf_cache_append behind it in every layer; the bits of the same steps.
// Option step_split = 1 (any dtype): _step and _extend run tf_attn_step_split / tf_attn_extend_split where tf_step_split_ok --
// one workgroup per token and head, its visible keys split over the four waves, partial softmax states merged in a fixed order; not the
// forward's bits, element-wise within a derived bound of fp64.  flope_tf_stream_attention runs the step's attention launch alone.
// Option extend_mfma = 1 (16-bit handles): _extend runs tf_attn16_extend where tf_extend_mfma_ok -- tf_attn_tiled's ring and
// 32-key step over the track's cache and the call's chunk, in absolute key blocks: the bits of the MFMA forward's rows.  It wins over
// step_split for _extend alone; _step, _prefill and the forwards do not read it.  flope_tf_stream_attention_extend runs that launch alone.
// flope_tf_mask_* / flope_tf_forward_masked (any dtype): any [L, L] mask compiled once to bits on the device -- the launch
// sequence with tf_attn_masked where the forward has its attention kernel, for every shape: a softmax over exactly the allowed keys in the
// generic kernel's order, a masked key never loaded; never the single launch, options causal / window neither read nor written (the host
// side is tf_attn_mask.h).
// Option mask_mfma = 1 (16-bit handles): a masked launch runs tf_attn_tiled_masked where tf_attn_pick_masked says so --
// tf_attn_tiled's ring and tf_attn16_step's MASKED form over the key blocks of the mask's tile map, which every mask carries beside its
// bits; tf_attn_tiled's bits where the mask is all-clear, causal, a causal band or block-diagonal at multiples of 32.
// flope_tf_bias_create (any dtype): an additive float mask -- the allowed set of its -inf entries plus a float32 value per
// allowed pair, one [L, L] plane or one per head -- on the mask's handle type; a launch under it is tf_attn_masked's BIASED instantiation
// for every dtype and option but bias_mfma: the unbiased order with bias[h][i][j] added to the scaled score in a rounding of its own, a
// zero bias giving its bits (why a flag and not a kernel of its own).
// Option bias_mfma = 1 (16-bit handles): a launch under a compiled bias runs tf_attn_tiled_masked's BIASED instantiation where
// tf_attn_pick_biased says so -- the walk of mask_mfma over the tile map of the bias's allowed set, which every bias carries behind its
// planes, with tf_attn16_step's BIASED form: one fma per score; a zero bias gives the bits of the compiled mask under mask_mfma = 1.
// flope_tf_stream_open_device / _step_assoc / _step_tracker (any dtype): a windowed state whose positions live on the device,
// stepped by an association only the device knows (the device tracker's): tf_stream_feed_kernel turns it into the step's table and the
// token rows by the rule of tf_stream_feed.h, the step's launch sequence runs for every row at smax = window, tf_feed_fill_bias writes
// out_layer's bias into the rows that fed nothing.
// Option skinny = 1 (16-bit handles): a linear that would run tf_gemm_mfma on 1 .. 32 rows runs tf_gemm_skinny -- one wave
// per 16-row feature tile of the same packed image, the operands from global memory straight into registers, the same MFMAs over the
// same operands in the same order: tf_gemm_mfma's bits (the planner is tf_skinny_plan.h).  Every caller of launch_linear takes it.
// Option skinny_ln = 1 (with skinny = 1): a LayerNorm of the forward directly in front of such a linear of K = model_dim
// <= 512 is not launched; the linear runs as tf_gemm_skinny_ln, which normalises the rows in its token load by tf_layernorm_vec's own
// definitions in its summation order and stores them: the bits of the two launches (run_forward_with: tf_ln_then_linear).
// Options norm_first / activation / final_norm (any dtype): torch's pre-norm layer, its erf GELU and
// nn.TransformerEncoder(norm=LayerNorm), stated before the weights are loaded.  The order of a forward and the buffers of every op are
// tf_arch_plan.h's list, which run_forward_with walks; GELU is tf_act.h's tf_gelu_f32 on the float32 accumulator of every linear kernel.
// The defaults are the architecture of the first line above: the same launches and bits.  tf_fused_f32 runs the default alone.
#include "../../include/flope_amd.h"
#include "common.h"
#include "host_pack.h"
#include "tf_act.h"
#include "tf_arch_plan.h"
#include "tf_attn_plan.h"
#include "tf_attn_mask.h"
#include "tf_encoder_stream.h"
#include "tf_fused_plan.h"
#include "tf_skinny_plan.h"
#include "tf_stream_feed.h"

#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <type_traits>
#include <vector>

using namespace flope_host;

namespace {

std::string g_tf_error;

#define GLDS16(gptr, lptr)                                                                             \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gptr),              \
                                   (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)
#define WAIT_VM(n_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n_) : "memory")
#define BLOCK_BARRIER()                  \
  do {                                   \
    asm volatile("" ::: "memory");       \
    __builtin_amdgcn_s_barrier();        \
    asm volatile("" ::: "memory");       \
  } while (0)

template <typename T> __device__ __forceinline__ float ld_any(const void* p, size_t i, int f32) {
  return f32 ? ((const float*)p)[i] : to_f32<T>(((const T*)p)[i]);
}
template <typename T> __device__ __forceinline__ void st_any(void* p, size_t i, int f32, float v) {
  if (f32) ((float*)p)[i] = v; else ((T*)p)[i] = from_f32<T>(v);
}
// the runtime activation of the generic linears: 0 none, FLOPE_TF_ACT_RELU, FLOPE_TF_ACT_GELU (tf_act.h), on the float32 accumulator
__device__ __forceinline__ float tf_act_f32(float v, int act) {
  if (act == FLOPE_TF_ACT_RELU) return fmaxf(v, 0.f);
  if (act == FLOPE_TF_ACT_GELU) return tf_gelu_f32(v);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---- generic kernels (any shape; fp32 accumulate) ------------------------------------------------------------
// The float32 summation orders, one definition each: the generic kernels below and tf_fused_f32 (its float instantiations, on LDS
// rows) call these, so a caller only decides which thread or wave takes which element or row.  Row strides are parameters.
// One element of Y = act(X W^T + b (+ R)): one fmaf chain k = 0 .. K - 1 from 0.f, + b[n], + residual, the activation (tf_act_f32)
template <typename T>
__device__ __forceinline__ void tf_linear_elem(const void* X, int xld, int x_f32, const float* W, const float* b, const void* R, int rld,
                                               void* Y, int yld, int y_f32, int m, int n, int K, int act) {
  const float* w = W + (size_t)n * K;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(ld_any<T>(X, (size_t)m * xld + k, x_f32), w[k], acc);
  acc += b[n];
  if (R) acc += ld_any<T>(R, (size_t)m * rld + n, 0);
  acc = tf_act_f32(acc, act);
  st_any<T>(Y, (size_t)m * yld + n, y_f32, acc);
}

// One row of a narrow linear (N <= 16, no residual) on one wave: lanes stride K, one wave reduction per output feature, lane 0 stores
template <typename T>
__device__ __forceinline__ void tf_rowwave_row(const void* X, int xld, int x_f32, const float* W, const float* b, void* Y, int yld,
                                               int y_f32, int m, int K, int N, int act, int lane) {
  float acc[16];
#pragma unroll
  for (int n = 0; n < 16; ++n) acc[n] = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float x = ld_any<T>(X, (size_t)m * xld + k, x_f32);
#pragma unroll
    for (int n = 0; n < 16; ++n)
      if (n < N) acc[n] = fmaf(x, W[(size_t)n * K + k], acc[n]);
  }
#pragma unroll
  for (int n = 0; n < 16; ++n)
    if (n < N) {
      float v = wave_sum(acc[n]) + b[n];
      v = tf_act_f32(v, act);
      if (lane == 0) st_any<T>(Y, (size_t)m * yld + n, y_f32, v);
    }
}

// LayerNorm (eps 1e-5, biased variance), one definition per expression: every LayerNorm kernel and tf_gemm_skinny_ln
// call these, so a caller only decides which lane holds which elements and in which order the partial sums meet.
// mean and 1 / std of a row of d from the row's sum and the sum of its squared deviations
__device__ __forceinline__ float tf_ln_mean(float sum, int d) { return sum / d; }
__device__ __forceinline__ float tf_ln_rstd(float sqsum, int d) { return 1.f / sqrtf(sqsum / d + 1e-5f); }
// one element of the result
__device__ __forceinline__ float tf_ln_elem(float x, float mean, float rstd, float w, float b) { return (x - mean) * rstd * w + b; }
// a 16-byte vector of eight 16-bit elements: its sum onto s (s += lo + hi, q = 0 .. 3), ...
template <typename T> __device__ __forceinline__ float tf_ln_vec_sum(const u32x4& r, float s) {
#pragma unroll
  for (int q = 0; q < 4; ++q) s += unpack_lo<T>(r[q]) + unpack_hi<T>(r[q]);
  return s;
}
// ... its squared deviations onto v (one fmaf chain, hi then lo of q = 0 .. 3), ...
template <typename T> __device__ __forceinline__ float tf_ln_vec_sq(const u32x4& r, float mean, float v) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float a = unpack_lo<T>(r[q]) - mean, c = unpack_hi<T>(r[q]) - mean;
    v = fmaf(a, a, fmaf(c, c, v));
  }
  return v;
}
// ... and its normalised elements, rounded to 16 bits: w and b are the eight columns of the vector
template <typename T> __device__ __forceinline__ u32x4 tf_ln_vec_out(const u32x4& r, float mean, float rstd, const float* w, const float* b) {
  u32x4 o;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    o[q] = pack2<T>(tf_ln_elem(unpack_lo<T>(r[q]), mean, rstd, w[q * 2], b[q * 2]), tf_ln_elem(unpack_hi<T>(r[q]), mean, rstd, w[q * 2 + 1], b[q * 2 + 1]));
  return o;
}

// LayerNorm of one row of d on one wave
template <typename T>
__device__ __forceinline__ void tf_layernorm_row(const T* x, T* y, const float* w, const float* b, int d, int lane) {
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += to_f32<T>(x[c]);
  const float mean = tf_ln_mean(wave_sum(s), d);
  float v = 0.f;
  for (int c = lane; c < d; c += 64) { const float t = to_f32<T>(x[c]) - mean; v = fmaf(t, t, v); }
  const float rstd = tf_ln_rstd(wave_sum(v), d);
  for (int c = lane; c < d; c += 64) y[c] = from_f32<T>(tf_ln_elem(to_f32<T>(x[c]), mean, rstd, w[c], b[c]));
}

// softmax(q k^T / sqrt(dh)) v for query i of one head on one wave.  base: the head's q columns of the sequence's first row, rows of
// ld elements (q | k | v at 0, d, 2 d); s: this wave's score row (L floats of LDS); orow: the dh outputs of the query.
// CAUSAL (all four attention kernels): query i attends to keys j <= i of its own sequence.  Here the three key loops end
// at i + 1 instead of L: the keys above the diagonal are never loaded.
// WINDOW (with CAUSAL; the 16-bit MFMA kernels have their own form): query i attends to keys lo .. i, lo = tf_window_lo(i, W) = max(0, i + 1 - W);
// the three key loops start at lo, so the keys below the window are never loaded either.  The order, fixed here once: lane l takes keys
// lo + l, lo + l + 64, ..; the value chain runs j = lo .. i from 0.f.  With lo = 0 (no window, or i < W) that is the order above.
template <typename T, bool CAUSAL = false, bool WINDOW = false>
__device__ __forceinline__ void tf_attn_row(const T* base, size_t ld, T* orow, float* s, int i, int L, int d, int dh, float scale, int lane,
                                            int W = 0) {
  static_assert(CAUSAL || !WINDOW, "a window without causal has no meaning");
  if constexpr (CAUSAL) L = flope_tf_plan::tf_causal_keys(i, 1, L);      // kend = i + 1
  int lo = 0;
  if constexpr (WINDOW) lo = flope_tf_plan::tf_window_lo(i, W);
  const T* q = base + (size_t)i * ld;
  float mx = -INFINITY;
  for (int j = lo + lane; j < L; j += 64) {
    const T* k = base + (size_t)j * ld + d;
    float a = 0.f;
    for (int c = 0; c < dh; ++c) a = fmaf(to_f32<T>(q[c]), to_f32<T>(k[c]), a);
    a *= scale;
    s[j] = a;
    mx = fmaxf(mx, a);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lo + lane; j < L; j += 64) { const float p = expf(s[j] - mx); s[j] = p; sum += p; }
  sum = wave_sum(sum);
  __builtin_amdgcn_wave_barrier();
  const float inv = 1.f / sum;
  for (int c = lane; c < dh; c += 64) {
    float o = 0.f;
    for (int j = lo; j < L; ++j) o = fmaf(s[j], to_f32<T>(base[(size_t)j * ld + 2 * d + c]), o);
    orow[c] = from_f32<T>(o * inv);
  }
  __builtin_amdgcn_wave_barrier();
}

// Y[m][n] = act(sum_k X[m][k] * W[n][k] + b[n] (+ R[m][n]))        W fp32 [N][K] as stored in the checkpoint
template <typename T>
__global__ void tf_linear_generic(const void* X, int x_f32, const float* W, const float* b, const void* R, void* Y,
                                  int y_f32, int M, int K, int N, int act) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)M * N) return;
  const int m = (int)(idx / N), n = (int)(idx - (size_t)m * N);
  tf_linear_elem<T>(X, K, x_f32, W, b, R, N, Y, N, y_f32, m, n, K, act);
}

// Narrow outputs (N <= 16, e.g. out_layer): one wave per token row, lanes stride K (coalesced X and W reads), one
// wave reduction per output feature.
template <typename T>
__global__ void tf_linear_rowwave(const void* X, int x_f32, const float* W, const float* b, void* Y, int y_f32, int M,
                                  int K, int N, int act) {
  const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int m = blockIdx.x * nw + (threadIdx.x >> 6); m < M; m += gridDim.x * nw)
    tf_rowwave_row<T>(X, K, x_f32, W, b, Y, N, y_f32, m, K, N, act, lane);
}

// The same for 16-bit activations with K % 8 == 0 (r03: the kernel above took 184 us for the out_layer of the throughput shape --
// 2-byte loads, one row per wave at a time -- against ~10 us of HBM time for its 50 MB): W is staged once per workgroup in LDS
// (N x K floats), a lane reads 16 bytes of its row per step and keeps two rows in flight.
template <typename T>
__global__ __launch_bounds__(256) void tf_linear_rowwave_vec(const T* __restrict__ X, const float* __restrict__ W,
                                                             const float* __restrict__ b, void* Y, int y_f32, int M, int K, int N, int act) {
  extern __shared__ __attribute__((aligned(16))) float sw[];          // [N][K]
  for (int i = threadIdx.x; i < N * K; i += 256) sw[i] = W[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, nw = 4;
  const int k8 = K >> 3;
  for (int m0 = (blockIdx.x * nw + (threadIdx.x >> 6)) * 2; m0 < M; m0 += gridDim.x * nw * 2) {
    float acc[2][16];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int n = 0; n < 16; ++n) acc[r][n] = 0.f;
    for (int c = lane; c < k8; c += 64) {
      u32x4 xv[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) xv[r] = *(const u32x4*)(X + (size_t)min(m0 + r, M - 1) * K + c * 8);
#pragma unroll
      for (int n = 0; n < 16; ++n)
        if (n < N) {
          const f32x4 w0 = *(const f32x4*)(sw + n * K + c * 8), w1 = *(const f32x4*)(sw + n * K + c * 8 + 4);
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            float a = acc[r][n];
            a = fmaf(unpack_lo<T>(xv[r][0]), w0[0], a); a = fmaf(unpack_hi<T>(xv[r][0]), w0[1], a);
            a = fmaf(unpack_lo<T>(xv[r][1]), w0[2], a); a = fmaf(unpack_hi<T>(xv[r][1]), w0[3], a);
            a = fmaf(unpack_lo<T>(xv[r][2]), w1[0], a); a = fmaf(unpack_hi<T>(xv[r][2]), w1[1], a);
            a = fmaf(unpack_lo<T>(xv[r][3]), w1[2], a); a = fmaf(unpack_hi<T>(xv[r][3]), w1[3], a);
            acc[r][n] = a;
          }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int n = 0; n < 16; ++n)
        if (n < N) {
          float v = wave_sum(acc[r][n]) + b[n];
          v = tf_act_f32(v, act);
          if (lane == 0 && m0 + r < M) st_any<T>(Y, (size_t)(m0 + r) * N + n, y_f32, v);
        }
  }
}

// float32 [M][K] -> 16-bit [M][Kp], columns K..Kp-1 zero (feeds the MFMA linear when K is not a multiple of 64)
template <typename T>
__global__ void tf_cast_pad(const float* X, T* Y, int M, int K, int Kp) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)M * Kp) return;
  const int m = (int)(idx / Kp), k = (int)(idx - (size_t)m * Kp);
  Y[idx] = from_f32<T>(k < K ? X[(size_t)m * K + k] : 0.f);
}

// Ragged batches (flope_tf_forward_varlen): rows i < off[b + 1] - off[b] of X [B][L][K] -> packed rows off[b] + i of Y [T][Kp]
// (TO = float, Kp = K: a copy; TO 16-bit: tf_cast_pad's conversion and zero columns).  Rows behind a sequence are never read.
template <typename TO>
__global__ void tf_gather_rows(const float* X, TO* Y, const int* __restrict__ off, int L, int K, int Kp, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t r = idx / Kp;
  const int k = (int)(idx - r * Kp), b = (int)(r / L), i = (int)(r - (size_t)b * L);
  const int o = off[b];
  if (i >= off[b + 1] - o) return;
  Y[(size_t)(o + i) * Kp + k] = from_f32<TO>(k < K ? X[r * K + k] : 0.f);
}

// ... and back: packed Yp [T][N] -> Y [B][L][N]; rows behind a sequence get the bias of out_layer (what the reference module
// returns there: its eval path zeroes padded tokens behind the encoder stack, and out_layer(0) = bias).  Y is fully written.
__global__ void tf_scatter_rows(const float* Yp, const float* __restrict__ bias, float* Y, const int* __restrict__ off, int L, int N, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t r = idx / N;
  const int c = (int)(idx - r * N), b = (int)(r / L), i = (int)(r - (size_t)b * L);
  const int o = off[b];
  Y[idx] = i < off[b + 1] - o ? Yp[(size_t)(o + i) * N + c] : bias[c];
}

// LayerNorm over the last dimension, one wave per row
template <typename T>
__global__ void tf_layernorm(const T* in, T* out, const float* w, const float* b, int M, int d) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  tf_layernorm_row<T>(in + (size_t)row * d, out + (size_t)row * d, w, b, d, lane);
}

// 16-bit rows with d % 8 == 0 and d <= 2048: each lane keeps its 16-byte vectors in registers (one HBM read)
template <typename T>
__global__ void tf_layernorm_vec(const T* in, T* out, const float* w, const float* b, int M, int d) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const int nv = d >> 3;
  const u32x4* x = (const u32x4*)(in + (size_t)row * d);
  u32x4 r[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + i * 64;
    if (c < nv) {
      r[i] = x[c];
      s = tf_ln_vec_sum<T>(r[i], s);
    }
  }
  const float mean = tf_ln_mean(wave_sum(s), d);
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (lane + i * 64 < nv) v = tf_ln_vec_sq<T>(r[i], mean, v);
  const float rstd = tf_ln_rstd(wave_sum(v), d);
  u32x4* y = (u32x4*)(out + (size_t)row * d);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + i * 64;
    if (c < nv) y[c] = tf_ln_vec_out<T>(r[i], mean, rstd, w + c * 8, b + c * 8);
  }
}

// softmax(q k^T / sqrt(dh)) v for one (batch, head) per blockIdx.x; one wave per query row.  Any L / dh.
// VARLEN (all four attention kernels): qkv and out are packed [T][.] rows of a ragged batch, sequence b is rows
// off[b] .. off[b + 1] - 1 and the L argument is the longest length, which sized the grid and the LDS; the kernel takes its own
// sequence's length for L, so every bound, mask and clamp below stays inside the sequence (row off[b] + L is the next sequence's
// first key, not padding).  The fixed-length instantiations (VARLEN = false, off unused) compile from the source they had.
// WINDOW (every launch under a window unless option window_mfma keeps a 16-bit MFMA kernel): keys i - W < j <= i; W is read by those instantiations alone and sits where the argument
// block had four bytes of padding, so every other argument keeps its offset.
template <typename T, bool VARLEN = false, bool CAUSAL = false, bool WINDOW = false>
__global__ void tf_attn_generic(const T* qkv, T* out, int L, int d, int H, int W, const int* __restrict__ off) {
  extern __shared__ float sc[];                 // [waves][L]
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, dh = d / H;
  const float scale = 1.f / sqrtf((float)dh);
  size_t row0 = 0;                              // first row of this sequence
  if constexpr (VARLEN) { row0 = (size_t)off[b]; L = off[b + 1] - off[b]; }
  float* s = sc + (size_t)wave * L;
  const T* base = VARLEN ? qkv + row0 * 3 * d + h * dh : qkv + (size_t)b * L * 3 * d + h * dh;
  for (int i = blockIdx.y * nw + wave; i < L; i += gridDim.y * nw)
    tf_attn_row<T, CAUSAL, WINDOW>(base, (size_t)3 * d, out + ((VARLEN ? row0 : (size_t)b * L) + i) * d + h * dh, s, i, L, d, dh, scale, lane, W);
}

// ---- streaming step (flope_tf_stream_*) ----------------------------------------------------------------------------
// VE consecutive elements of a head slice as floats: one 16-byte load (VEC) or VE = 1 element
template <typename T, bool VEC> struct TfSlice {
  static constexpr int VE = VEC ? 16 / (int)sizeof(T) : 1;
  float f[VE];
  __device__ __forceinline__ void load(const T* p) {
    if constexpr (!VEC) f[0] = to_f32<T>(p[0]);
    else if constexpr (std::is_same<T, float>::value) {
      const f32x4 v = *(const f32x4*)p;
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = v[e];
    } else {
      const u32x4 v = *(const u32x4*)p;
#pragma unroll
      for (int w = 0; w < 4; ++w) { f[2 * w] = unpack_lo<T>(v[w]); f[2 * w + 1] = unpack_hi<T>(v[w]); }
    }
  }
  __device__ __forceinline__ void store(T* p) const {
    if constexpr (!VEC) p[0] = from_f32<T>(f[0]);
    else if constexpr (std::is_same<T, float>::value) *(f32x4*)p = f32x4{f[0], f[1], f[2], f[3]};
    else {
      // element-wise conversions, as tf_attn_row's store makes them
      struct { T t[VE]; } w;
#pragma unroll
      for (int e = 0; e < VE; ++e) w.t[e] = from_f32<T>(f[e]);
      *(u32x4*)p = __builtin_bit_cast(u32x4, w);
    }
  }
};

// The streamed attention row, one definition for the step and the extend: tf_attn_row<T, true> (WINDOW:
// <T, true, true>) for the query at chunk row i of a sequence whose track holds pos0 tokens -- position p = pos0 + i, keys lo .. p,
// lo = tf_window_lo(p, W) under WINDOW and 0 otherwise -- operation for operation.  The order is tf_attn_row's: per key one fmaf chain
// over c = 0 .. dh - 1 from 0.f, * scale; lane l takes keys lo + l, lo + l + 64, ..; wave_max, expf, wave_sum; per output dim one fmaf
// chain over j = lo .. p from 0.f; * (1 / sum), float16 in one rounding (tf_mul_f16_bits) -- and so are the bits: the tests of
// tests/test_gpu_tf_stream.py, _window.py and _extend.py hold step, extend and tf_attn_row to that.  It is a second definition beside
// tf_attn_row, not a call, because what differs is the loops themselves: a key comes from one of two buffers, a lane reads its key's
// slice as 16-byte vectors, and the value pass gives a lane VE output dims and keeps kTfStepUnroll keys' loads in flight in front of
// their fmafs, where tf_attn_row has one scalar load per trip; each of these would change the loops tf_attn_generic and tf_fused_f32
// compile from.
// The keys lie in up to three contiguous runs of rows.  The nc = tf_extend_cached cached keys lo .. pos0 - 1 are cache rows lo .. (kv:
// the head's k columns of cache row 0 of the track, rows of 2 d: k | v); on a ring key j lives in row j % capacity, the nc keys are
// consecutive rows from slo = lo % capacity on that wrap at most once (nc < W <= capacity), so a key's row is one add and one
// conditional subtract in the score pass and the value pass walks two runs (tf_stream_run0), no modulo per key.  Keys max(lo, pos0)
// .. p are the chunk's own packed qkv rows c0 = tf_extend_chunk0 .. i (chunk: the head's q columns of the sequence's first packed
// row, rows of 3 d: q | k | v), the query's own among them -- never a cache row the same call writes.  s: the wave's score row, key j
// at s[j - lo] (the loops count from key lo: an absolute position may be near INT_MAX).
// ONE: the caller's promise that the chunk is the single row `chunk` (i = 0), which is what a step is: then nc = p - lo, c0 = 0 and
// the last run is one row.  Without it the compiler cannot see that and unrolls the last run again.
// BIASED (a state with a distance table, flope_tf_stream_open_bias; brel: the head's row of the table in global memory,
// float32 [D], indexed by the distance p - key; unread otherwise): ONE change, in the score pass, the one tf_attn_masked_row<T, true>
// makes.  The lane that owns the visible key with index j (0 .. L - 1 counted from lo, as s[j] is) loads brel[L - 1 - j]
// (tf_stream_bias_index: the query's own key has distance 0), and the score is fl(fl(chain * scale) + brel[L - 1 - j]): the product
// and the sum are the plain operators under `#pragma clang fp contract(off)`, two roundings, never one fma -- so over the contiguous key
// range lo .. p this row is tf_attn_masked_row<T, true>'s, operation for operation, and with a zero table the unbiased row's.  The
// caller guarantees L <= D (tf_stream_bias_keys_ok), so 0 <= L - 1 - j <= D - 1.  The table is read from global memory, as the planes
// of a compiled bias are, not staged in LDS: an entry is read once per row, by one lane, a trip's 64 entries are one contiguous 256
// bytes, and no other wave of the workgroup shares them in a step (every wave is another track or head) -- staging would add a barrier
// and LDS beside score rows that already take up to 64 KiB.
constexpr int kTfStepUnroll = 16;
// (float16)(a * b) in ONE rounding, as bits: what the compiler makes of tf_attn_row's `from_f32<f16_t>(o * inv)`, one v_fma_mixlo_f16.
// A packed store of two such products (v_mul_f32, then v_cvt_pk_f16_f32) rounds to float32 first and to float16 second, and the two
// roundings differ from the one in the last bit of about one element in 2^13 -- which is what the VEC float16 store of the step row
// once compiled to, against DESIGN.md 25's bit contract with tf_attn_row (no test there had a shape that showed it).  That store spells the
// instruction out, so that its bits do not hang on which of the two forms the compiler picks.
__device__ __forceinline__ unsigned tf_mul_f16_bits(float a, float b) {
  unsigned r = 0;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(r) : "v"(a), "v"(b));
  return r & 0xffffu;
}
template <typename T, bool VEC, bool WINDOW, bool ONE, bool BIASED = false>
__device__ __forceinline__ void tf_attn_stream_row(const T* chunk, const T* kv, T* orow, float* s, int pos0, int i, int d, int dh, float scale,
                                                   int lane, int capacity, int W, const float* __restrict__ brel = nullptr) {
  typedef TfSlice<T, VEC> Sl;
  constexpr int VE = Sl::VE;
  const size_t ld = (size_t)2 * d, ldc = (size_t)3 * d;
  const int p = pos0 + i;
  int lo = 0, slo = 0;                            // first visible key and, where it is a cached one, its cache row
  if constexpr (WINDOW) { lo = flope_tf_plan::tf_window_lo(p, W); slo = flope_tf_plan::tf_stream_slot(lo, capacity); }
  const int nc = ONE ? p - lo : flope_tf_plan::tf_extend_cached(pos0, lo), c0 = ONE ? 0 : flope_tf_plan::tf_extend_chunk0(pos0, lo);
  const int L = p - lo + 1, own = ONE ? 1 : L - nc;   // visible keys: nc cached ones, then the `own` chunk rows c0 .. i
  const T* q = chunk + (size_t)i * ldc;
  float mx = -INFINITY;
  for (int j = lane; j < L; j += 64) {
    const T* k;
    if (j < nc) {
      int row = j;
      if constexpr (WINDOW) { row = slo + j; if (row >= capacity) row -= capacity; }
      k = kv + (size_t)row * ld;
    } else k = chunk + (ONE ? 0 : (size_t)(c0 + j - nc) * ldc) + d;
    float bj = 0.f;
    if constexpr (BIASED) bj = brel[flope_tf_plan::tf_stream_bias_index(L, j)];
    float a = 0.f;
    for (int c = 0; c < dh; c += VE) {
      Sl qv, kx;
      qv.load(q + c);
      kx.load(k + c);
#pragma unroll
      for (int e = 0; e < VE; ++e) a = fmaf(qv.f[e], kx.f[e], a);
    }
    if constexpr (BIASED) {
#pragma clang fp contract(off)
      a = a * scale;
      a = a + bj;
    } else a *= scale;
    s[j] = a;
    mx = fmaxf(mx, a);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < L; j += 64) { const float pr = expf(s[j] - mx); s[j] = pr; sum += pr; }
  sum = wave_sum(sum);
  __builtin_amdgcn_wave_barrier();
  const float inv = 1.f / sum;
  for (int c = lane * VE; c < dh; c += 64 * VE) {
    float o[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) o[e] = 0.f;
    // cnt consecutive rows of ldr elements from vr on, their probabilities from sp on, kTfStepUnroll loads in flight: the chain goes on
    // in key order.  (tf_attn_split_row's value loop is strided by lane group and predicated per key: another loop, not a copy of this.)
    auto run = [&](const T* vr, size_t ldr, const float* sp, int cnt) {
      int j = 0;
      for (; j + kTfStepUnroll <= cnt; j += kTfStepUnroll) {
        Sl vv[kTfStepUnroll];
#pragma unroll
        for (int u = 0; u < kTfStepUnroll; ++u) vv[u].load(vr + (size_t)(j + u) * ldr);
#pragma unroll
        for (int u = 0; u < kTfStepUnroll; ++u) {
          const float pr = sp[j + u];
#pragma unroll
          for (int e = 0; e < VE; ++e) o[e] = fmaf(pr, vv[u].f[e], o[e]);
        }
      }
      for (; j < cnt; ++j) {
        Sl vv;
        vv.load(vr + (size_t)j * ldr);
#pragma unroll
        for (int e = 0; e < VE; ++e) o[e] = fmaf(sp[j], vv.f[e], o[e]);
      }
    };
    const T* v = kv + d + c;
    if constexpr (WINDOW) {
      const int first = flope_tf_plan::tf_stream_run0(slo, nc, capacity);      // keys lo .. pos0 - 1: rows slo .., then rows 0 ..
      run(v + (size_t)slo * ld, ld, s, first);
      run(v, ld, s + first, nc - first);
    } else run(v, ld, s, nc);                                                  // rows 0 .. pos0 - 1
    run(chunk + (size_t)c0 * ldc + 2 * d + c, ldc, s + nc, own);               // chunk rows c0 .. i
    if constexpr (std::is_same<T, f16_t>::value) {      // one rounding per element, as tf_attn_row's store
      if constexpr (VEC) {
        u32x4 w;
#pragma unroll
        for (int e = 0; e < VE; e += 2) w[e / 2] = tf_mul_f16_bits(o[e], inv) | (tf_mul_f16_bits(o[e + 1], inv) << 16);
        *(u32x4*)(orow + c) = w;
      } else *(unsigned short*)(orow + c) = (unsigned short)tf_mul_f16_bits(o[0], inv);
    } else {
      Sl vv;
#pragma unroll
      for (int e = 0; e < VE; ++e) vv.f[e] = o[e] * inv;
      vv.store(orow + c);
    }
  }
  __builtin_amdgcn_wave_barrier();
}

// ---- attention under a compiled mask or additive bias (flope_tf_*_masked, flope_tf_bias_create; host side tf_attn_mask.h) ----
// softmax(q k^T / sqrt(dh) [+ brow]) v for query i of one head on one wave, over exactly the keys the mask allows it: bit j % 32 of
// mw[j / 32] (mw: this wave's copy of row i's mask words in LDS).  first / last: the first and last allowed key of the row, last already
// clamped to the sequence's last token.  The order, fixed here once for both instantiations:
//   score pass  lane l takes keys first + l, first + l + 64, .. up to last.  An allowed key gets tf_attn_row's fmaf chain over
//               c = 0 .. dh - 1 from 0.f, then * scale, into s[j] and the maximum.  A masked key is skipped: no load, no store to the
//               score row, not in the maximum.  A 64-key trip in which no lane has an allowed key (one wave-wide vote) issues nothing.
//   sum pass    the same lane walk: expf(s - max) and sum += p over allowed keys only, then wave_sum.
//   value pass  per output dim one fmaf chain from 0.f over the allowed keys in ascending j -- a walk over the set bits of the words
//               first / 32 .. last / 32, kTfMaskUnroll keys' loads in flight in front of their fmafs, no test per j -- then
//               * (1 / sum) and the store as tf_attn_row makes them: float16 in ONE rounding (tf_mul_f16_bits).
// Where the allowed keys of a row are the contiguous range lo .. hi this is tf_attn_row's order for that range, operation for
// operation, and so are the bits (tests/test_gpu_tf_mask.py: all-clear, causal, bands and block-diagonal masks against tf_attn_generic's
// instantiations).  It is a second definition beside tf_attn_row because the loops themselves differ (a vote per trip, a predicate per
// key, a bit walk in place of the counted value loop); BIASED is a compile-time flag on it, which costs neither instantiation an
// instruction of its loops.
// BIASED (brow: row i of head h's bias plane in global memory, float32, stride the mask's L, indexed by the key's own position j;
// unread otherwise): ONE change, in the score pass.  After a = fl(chain * scale) the lane that owns key j loads brow[j] and the score is
// fl(a + brow[j]): a rounding of its own, NOT an fma with the scale (the reference adds the bias to the already scaled, already rounded
// score; with brow[j] = 0 the score is the unbiased instantiation's bit for bit, which tests/test_gpu_tf_bias.py holds).  The product and
// the sum are the plain operators in a block under `#pragma clang fp contract(off)`.  The round-to-nearest intrinsics __fmul_rn /
// __fadd_rn do NOT keep them apart here: this toolchain's header defines both as the plain operators in functions of its own, outside
// the pragma's lexical reach, and with them -- with and without the pragma -- the compiler contracted the pair into one v_fma_f32 (the
// -S dump: one fma more and one v_mul_f32 fewer than the unbiased kernel).  As written the dump holds the unbiased kernel's v_fma /
// v_mul counts and one v_add_f32 more.
// A masked key is never addressed -- not its k, not its v, not its bias entry (which holds -inf) -- so NaN or Inf in a key that no query
// allows reaches no output.
constexpr int kTfMaskUnroll = 8;
template <typename T, bool BIASED>
__device__ __forceinline__ void tf_attn_masked_row(const T* base, size_t ld, T* orow, float* s, const uint32_t* mw, const float* __restrict__ brow, int i,
                                                   int first, int last, int d, int dh, float scale, int lane) {
  const T* q = base + (size_t)i * ld;
  float mx = -INFINITY;
  for (int j0 = first; j0 <= last; j0 += 64) {
    const int j = j0 + lane;
    const bool on = j <= last && ((mw[j >> 5] >> (j & 31)) & 1u);
    if (!__builtin_amdgcn_ballot_w64(on)) continue;
    if (on) {
      const T* k = base + (size_t)j * ld + d;
      float bj = 0.f;
      if constexpr (BIASED) bj = brow[j];
      float a = 0.f;
      for (int c = 0; c < dh; ++c) a = fmaf(to_f32<T>(q[c]), to_f32<T>(k[c]), a);
      if constexpr (BIASED) {
#pragma clang fp contract(off)
        a = a * scale;
        a = a + bj;
      } else a *= scale;
      s[j] = a;
      mx = fmaxf(mx, a);
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j0 = first; j0 <= last; j0 += 64) {
    const int j = j0 + lane;
    const bool on = j <= last && ((mw[j >> 5] >> (j & 31)) & 1u);
    if (on) { const float p = expf(s[j] - mx); s[j] = p; sum += p; }
  }
  sum = wave_sum(sum);
  __builtin_amdgcn_wave_barrier();
  const float inv = 1.f / sum;
  const int w0 = first >> 5, w1 = last >> 5;
  for (int c = lane; c < dh; c += 64) {
    const T* v = base + 2 * d + c;
    float o = 0.f;
    for (int w = w0; w <= w1; ++w) {
      uint32_t m = __builtin_amdgcn_readfirstlane(mw[w]);
      if (w == w0) m &= ~0u << (first & 31);                     // nothing below first, nothing above last: whatever the words hold,
      if (w == w1) m &= (2u << (last & 31)) - 1u;                // no key outside first .. last is addressed
      const int jb = w * 32;
      while (__builtin_popcount(m) >= kTfMaskUnroll) {
        int js[kTfMaskUnroll];
        float vv[kTfMaskUnroll];
#pragma unroll
        for (int u = 0; u < kTfMaskUnroll; ++u) { js[u] = jb + __builtin_ctz(m); m &= m - 1u; }
#pragma unroll
        for (int u = 0; u < kTfMaskUnroll; ++u) vv[u] = to_f32<T>(v[(size_t)js[u] * ld]);
#pragma unroll
        for (int u = 0; u < kTfMaskUnroll; ++u) o = fmaf(s[js[u]], vv[u], o);
      }
      while (m) {
        const int j = jb + __builtin_ctz(m);
        m &= m - 1u;
        o = fmaf(s[j], to_f32<T>(v[(size_t)j * ld]), o);
      }
    }
    if constexpr (std::is_same<T, f16_t>::value) *(unsigned short*)(orow + c) = (unsigned short)tf_mul_f16_bits(o, inv);
    else orow[c] = from_f32<T>(o * inv);
  }
  __builtin_amdgcn_wave_barrier();
}

// Workgroup (b, h) x blockIdx.y, one wave per query row, as tf_attn_generic; L: the sequence length (VARLEN: the longest of the batch),
// which sized the grid and the score rows.  Lm: the mask's sequence length; bits [Lm][ceil(Lm / 32)], first / last [Lm]: the compiled
// mask's device tables.  LDS: [4][L] floats of score rows, behind them [4][ceil(Lm / 32)] mask words (tf_mask_launch).
// Memory safety does not hang on the tables' contents: a sequence has n <= min(L, Lm) tokens here whatever `off` says about it, row
// i < n reads the words first / 32 .. last / 32 of its own mask row only, last is clamped to n - 1, and a row whose first is not inside
// its sequence leaves before its first store (the host refuses such a call: tf_mask_length_row).
// BIASED: bias is float32 [planes][Lm][Lm] behind the mask's tables in the same allocation, planes = 1 (every head reads plane 0) or H;
// otherwise both are unread, and sit behind `off` so that the unbiased kernels find every argument where they always did.  A row reaches
// tf_attn_masked_row only with i < n <= Lm and first <= last <= n - 1, the plane index is 0 or h < H = planes, and the row loads brow[j]
// only for an allowed key first <= j <= last -- so every bias address lies inside the planes whatever the tables hold.
template <typename T, bool VARLEN, bool BIASED>
__global__ void tf_attn_masked(const T* qkv, T* out, int L, int d, int H, int Lm, const uint32_t* __restrict__ bits, const int* __restrict__ first,
                               const int* __restrict__ last, const int* __restrict__ off, const float* __restrict__ bias, int planes) {
  extern __shared__ float sc[];                 // [waves][L] | [waves][words]
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, dh = d / H;
  const int words = flope_tf_plan::tf_mask_words(Lm);
  const float scale = 1.f / sqrtf((float)dh);
  size_t row0 = 0;                              // first row of this sequence
  int n = L;
  if constexpr (VARLEN) { row0 = (size_t)off[b]; n = off[b + 1] - off[b]; }
  if (n > L) n = L;
  if (n > Lm) n = Lm;
  float* s = sc + (size_t)wave * L;
  uint32_t* mw = (uint32_t*)(sc + (size_t)nw * L) + (size_t)wave * words;
  const T* base = VARLEN ? qkv + row0 * 3 * d + h * dh : qkv + (size_t)b * L * 3 * d + h * dh;
  const float* plane = nullptr;
  if constexpr (BIASED) plane = bias + (size_t)(planes > 1 ? h : 0) * Lm * Lm;
  for (int i = blockIdx.y * nw + wave; i < n; i += gridDim.y * nw) {
    const int fi = __builtin_amdgcn_readfirstlane(first[i]);
    int la = __builtin_amdgcn_readfirstlane(last[i]);
    if ((unsigned)fi >= (unsigned)n) continue;
    if (la > n - 1) la = n - 1;
    if (la < fi) continue;
    for (int w = (fi >> 5) + lane; w <= (la >> 5); w += 64) mw[w] = bits[(size_t)i * words + w];
    __builtin_amdgcn_wave_barrier();
    tf_attn_masked_row<T, BIASED>(base, (size_t)3 * d, out + ((VARLEN ? row0 : (size_t)b * L) + i) * d + h * dh, s, mw,
                                  BIASED ? plane + (size_t)i * Lm : nullptr, i, fi, la, d, dh, scale, lane);
  }
}

// Whether the table entry (track, pos0) of a step (len = 1) or of a chunk of len tokens may touch its track's cache: the track is one,
// the chunk has a token, and its positions pos0 .. pos0 + len - 1 are rows of a linear cache, or ints over a ring whose window W is
// one this cache can hold.  Every stream kernel leaves on `false` before its first load from or store to the cache; the two with a
// score row test smax beside it.  What each had of its own before this was one function:
//   tf_attn_step, tf_attn_step_split, linear: `(unsigned)pos >= (unsigned)capacity` is pos0 < 0 || pos0 > capacity - 1, the last line
//     at len = 1 (that one-compare form is kept: with two signed compares the f16 step measured 0.3 - 0.5 % slower);  WINDOW: track, pos < 0, W < 1, W > capacity -- and now pos0 == INT_MAX too, which the host refuses (kTfStreamFull)
//   tf_attn_extend, tf_attn_extend_split: these very tests (linear: pos0 < 0 || pos0 > capacity - len, with len <= capacity in front
//     so that capacity - len is no negative number turned large)
//   tf_attn16_extend: tf_extend_mfma_positions_ok is pos0 >= 0, len >= 1 and a bound below INT_MAX - len; it stays at the call
//   tf_cache_append (W = capacity: it has no window to test): track, pos0 < 0, the two position tests; i < len gives len >= 1
template <bool WINDOW>
__device__ __forceinline__ bool tf_stream_entry_ok(int track, int pos0, int len, int tracks, int capacity, int W) {
  if ((unsigned)track >= (unsigned)tracks || len < 1) return false;
  if constexpr (WINDOW) return pos0 >= 0 && W >= 1 && W <= capacity && pos0 <= INT_MAX - len;
  else return len <= capacity && (unsigned)pos0 <= (unsigned)(capacity - len);     // 0 <= pos0 <= capacity - len in one compare
}

// One new token per track: wave (row r, head h) takes q, k and v of the token from row r of qkv [n][3 d], stores that k | v slice
// into row pos of its track in cache [tracks][capacity][2 d] (one layer's part; for later steps only) and writes
// softmax(q K^T / sqrt(dh)) V over keys 0 .. pos to att [n][d].  tab: (track, pos) per row.  smax: floats of a wave's score row
// (the call's largest pos + 1).  A row whose table entry is no track, no row of the cache or past the score row is left alone:
// nothing is written outside the track's capacity rows, whatever the table holds.
// WINDOW: pos is absolute and unbounded, the cache a ring -- the slice goes to row pos % capacity, attention is over keys
// tf_window_lo(pos, W) .. pos, smax the call's largest visible key count (<= W).  The overwrite is safe: row pos % capacity held key
// pos - capacity <= pos - W, which is outside every window that includes pos, so no wave of this launch reads it (the launch's rows
// are distinct tracks, and the heads of one row touch distinct columns).  Left alone: a row whose track is out of range, whose pos is
// negative or whose visible keys exceed the score row; pos % capacity is a row of the track whatever else the table holds.
// BIASED: REL is (const float* rel, int planes, int D) -- rel the state's distance table, float32 [planes][D], planes = 1
// (every head reads plane 0) or H -- and the empty pack otherwise: an unbiased instantiation's argument block is byte for byte what it
// was, and with it the offset of the hidden arguments behind it (three unread arguments at the end moved that offset, one immediate
// in every tf_attn_extend that reads gridDim.y).  A row whose
// visible key count exceeds D leaves with the others above, before its first load from or store to the cache
// (tf_stream_bias_keys_ok, beside the smax test): the plane index is 0 or h < H = planes and the row loads brel[L - 1 - j] for
// 0 <= j <= L - 1 <= D - 1 only -- so every table address lies inside the planes whatever the device table of positions holds.
// the arguments of a BIASED instantiation behind W, as one value
struct TfRel { const float* rel; int planes, D; };
template <typename T, bool VEC, bool WINDOW = false, bool BIASED = false, typename... REL>
__global__ __launch_bounds__(256) void tf_attn_step(const T* __restrict__ qkv, T* cache, T* __restrict__ att, const int* __restrict__ tab, int n,
                                                    int d, int H, int tracks, int capacity, int smax, int W, REL... rel_args) {
  static_assert(sizeof...(REL) == (BIASED ? 3 : 0), "a BIASED instantiation takes (rel, planes, D), an unbiased one nothing");
  extern __shared__ __attribute__((aligned(16))) float sc[];     // [waves][smax]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int it = blockIdx.x * flope_tf_plan::kTfStepWaves + wave;
  if (it >= n * H) return;
  const int r = it / H, h = it - r * H, dh = d / H;
  const int track = tab[2 * r], pos = tab[2 * r + 1];
  if (!tf_stream_entry_ok<WINDOW>(track, pos, 1, tracks, capacity, W) || flope_tf_plan::tf_window_keys(pos, WINDOW ? W : 0) > smax) return;
  if constexpr (BIASED) { if (!flope_tf_plan::tf_stream_bias_keys_ok(flope_tf_plan::tf_window_keys(pos, WINDOW ? W : 0), TfRel{rel_args...}.D)) return; }
  const int slot = WINDOW ? flope_tf_plan::tf_stream_slot(pos, capacity) : pos;      // the cache row of the token
  const float scale = 1.f / sqrtf((float)dh);
  const size_t ld = (size_t)2 * d;
  const T* tok = qkv + (size_t)r * 3 * d + h * dh;
  T* kv = cache + (size_t)track * capacity * ld + h * dh;
  constexpr int VE = TfSlice<T, VEC>::VE;
  for (int c = lane * VE; c < 2 * dh; c += 64 * VE) {            // k slice | v slice of the token -> cache row pos (WINDOW: pos % capacity)
    const int col = c < dh ? c : c - dh + d;
    if constexpr (VEC) *(u32x4*)(kv + slot * ld + col) = *(const u32x4*)(tok + d + col);
    else kv[slot * ld + col] = tok[d + col];
  }
  // a step is an extend of one row: chunk = the token's row, pos0 = pos, i = 0
  if constexpr (BIASED) {
    const TfRel t{rel_args...};
    tf_attn_stream_row<T, VEC, WINDOW, true, true>(tok, kv, att + (size_t)r * d + h * dh, sc + (size_t)wave * smax, pos, 0, d, dh, scale, lane, capacity, W,
                                                   t.rel + (size_t)(t.planes == H ? h : 0) * t.D);
  } else
    tf_attn_stream_row<T, VEC, WINDOW, true>(tok, kv, att + (size_t)r * d + h * dh, sc + (size_t)wave * smax, pos, 0, d, dh, scale, lane, capacity, W);
}

// ---- extend: several tokens per track and call (flope_tf_stream_extend) ----------------------------------------------

// n sequences of a ragged batch (qkv: packed rows, sequence b = rows off[b] .. off[b + 1] - 1), each the next tokens of one track.
// Workgroup (b, h) x blockIdx.y: its four waves take consecutive queries of that sequence and head, as tf_attn_generic<.., VARLEN>
// does, so they stream the same cache rows -- in tf_attn_step every wave walks another track.  tab: (track, pos0) per sequence.
// smax: floats of a wave's score row, the call's largest visible key count.  Reads the cache, writes att alone; a workgroup whose
// table entry is no track, whose positions leave the cache (linear: pos0 + len > capacity; a ring: past INT_MAX, or a window that is
// none of this cache's) or whose keys exceed the score row exits before it stores anything (tf_stream_entry_ok, and smax).
// BIASED: REL = (rel, planes, D) as in tf_attn_step, behind W, and the empty pack otherwise.  A workgroup whose largest visible key count
// (its last query's, tf_extend_keys) exceeds D exits with the others above, before its first load (tf_stream_bias_keys_ok): every query
// of the chunk then has L <= D keys, the plane index is 0 or h < H = planes, and a row loads brel[L - 1 - j] for 0 <= j <= L - 1 only --
// every table address lies inside the planes whatever the device tables hold.  A prefill of a biased state is this kernel at pos0 = 0,
// where no cached key is read (nc = 0) and the row is the biased forward's.
template <typename T, bool VEC, bool WINDOW, bool BIASED = false, typename... REL>
__global__ __launch_bounds__(256) void tf_attn_extend(const T* __restrict__ qkv, const T* __restrict__ cache, T* __restrict__ att,
                                                      const int* __restrict__ tab, const int* __restrict__ off, int n, int d, int H, int tracks,
                                                      int capacity, int smax, int W, REL... rel_args) {
  static_assert(sizeof...(REL) == (BIASED ? 3 : 0), "a BIASED instantiation takes (rel, planes, D), an unbiased one nothing");
  extern __shared__ __attribute__((aligned(16))) float sc[];     // [waves][smax]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, dh = d / H;
  if (b >= n) return;
  const int track = tab[2 * b], pos0 = tab[2 * b + 1];
  const int o = off[b], len = off[b + 1] - o;
  if (!tf_stream_entry_ok<WINDOW>(track, pos0, len, tracks, capacity, W) || flope_tf_plan::tf_extend_keys(pos0, len, WINDOW ? W : 0) > smax) return;
  if constexpr (BIASED) { if (!flope_tf_plan::tf_stream_bias_keys_ok(flope_tf_plan::tf_extend_keys(pos0, len, WINDOW ? W : 0), TfRel{rel_args...}.D)) return; }
  const float scale = 1.f / sqrtf((float)dh);
  const T* chunk = qkv + (size_t)o * 3 * d + h * dh;
  const T* kv = cache + (size_t)track * capacity * 2 * d + h * dh;
  float* s = sc + (size_t)wave * smax;
  for (int i = blockIdx.y * flope_tf_plan::kTfStepWaves + wave; i < len; i += gridDim.y * flope_tf_plan::kTfStepWaves) {
    if constexpr (BIASED) {
      const TfRel t{rel_args...};
      tf_attn_stream_row<T, VEC, WINDOW, false, true>(chunk, kv, att + (size_t)(o + i) * d + h * dh, s, pos0, i, d, dh, scale, lane, capacity, W,
                                                      t.rel + (size_t)(t.planes == H ? h : 0) * t.D);
    } else
      tf_attn_stream_row<T, VEC, WINDOW, false>(chunk, kv, att + (size_t)(o + i) * d + h * dh, s, pos0, i, d, dh, scale, lane, capacity, W);
  }
}

// The one cache copy: the k | v columns (d .. 3 d) of the valid packed rows of qkv [T][3 d] -> the cache [tracks][capacity][2 d]: row
// i of sequence b goes to cache row pos0 + i of its track (a ring: row (pos0 + i) % capacity, and only the sequence's last min(len,
// capacity) tokens go, tf_stream_append_writes -- the earlier ones share their rows with those, and two threads would write one
// address).  off: the ragged batch's offsets; tab: (track, pos0) per sequence -- tf_attn_extend's table for the append of an extend,
// (track, 0) for a prefill.  V: u32x4 (dv = d / elements per 16 bytes) or the element type (dv = d).  A sequence whose entry is no
// track or whose rows leave the cache is skipped as a whole (tf_stream_entry_ok).
// An extend runs it BEHIND the layer's tf_attn_extend: on a ring the token at p takes the row of key p - capacity, which an earlier
// query of the same chunk still sees once len >= capacity - W + 2 (at capacity == W: every chunk of two tokens).  A prefill runs it
// in front of the layer's attention, which reads the packed rows and not the cache.
template <typename V, bool WINDOW>
__global__ void tf_cache_append(const V* __restrict__ qkv, V* __restrict__ cache, const int* __restrict__ off, const int* __restrict__ tab,
                                int max_len, int dv, int tracks, int capacity, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t r = idx / (2 * dv);
  const int c = (int)(idx - r * (2 * dv)), b = (int)(r / max_len), i = (int)(r - (size_t)b * max_len);
  const int o = off[b], len = off[b + 1] - o, t = tab[2 * b], pos0 = tab[2 * b + 1];
  if (i >= len || !tf_stream_entry_ok<WINDOW>(t, pos0, len, tracks, capacity, capacity)) return;
  int row = pos0 + i;
  if constexpr (WINDOW) {
    if (!flope_tf_plan::tf_stream_append_writes(i, len, capacity)) return;
    row = flope_tf_plan::tf_stream_append_slot(pos0, i, capacity);
  }
  cache[((size_t)t * capacity + row) * 2 * dv + c] = qkv[(size_t)(o + i) * 3 * dv + dv + c];
}

// ---- a device-positioned state: the step's table and tokens from an association (flope_tf_stream_step_assoc / _step_tracker)

// One thread per row m < n of a frame: the feed rule of tf_stream_feed.h (tf_feed_row: the table entry tab[2 m], tab[2 m + 1] and, for a
// row that feeds, its track's position) and the float32 token row tok[m][0 .. input_dim - 1].  No two feeding rows name one track and
// a row reads pos[] only for the track it feeds, so the threads need no order among themselves: no LDS, no atomics, no barrier.
// assoc: int32 [n] in the tracker's encoding; overflow: one int32 or nullptr (clear).  The token of a feeding row:
//   SOURCE FLOPE_TF_FEED_MEAS   vec7 [n][7] float64, row m           (the frame's measurements)
//   SOURCE FLOPE_TF_FEED_MEAN   vec7 [vec_rows][7] float64, row track (the filtered means; track < vec_rows is tested, a tracker's
//                               association never names a track it has not opened)
//   SOURCE kTfFeedRows          x [n][input_dim] float32, row m       (flope_tf_stream_step_assoc: the caller's rows)
// the first two rounded once to float32 with zeros behind column 6 (tf_feed_token).  A row that feeds nothing is all zero.  Every
// address is bounded by n, tracks or vec_rows whatever the association holds: the track of a feeding row is below `tracks` by rule.
constexpr int kTfFeedRows = 2;
constexpr int kTfFeedBlock = 64;
template <int SOURCE>
__global__ __launch_bounds__(kTfFeedBlock) void tf_stream_feed_kernel(const int* __restrict__ assoc, const int* __restrict__ overflow, int n, int tracks,
                                                                      int* pos, int* __restrict__ tab, const double* __restrict__ vec7, int vec_rows,
                                                                      const float* __restrict__ x, int input_dim, float* __restrict__ tok) {
  const int m = blockIdx.x * kTfFeedBlock + threadIdx.x;
  if (m >= n) return;
  const int t = flope_tf_plan::tf_feed_row(assoc, m, overflow ? overflow[0] : 0, tracks, pos, tab);
  float* row = tok + (size_t)m * input_dim;
  if constexpr (SOURCE == kTfFeedRows) {
    for (int c = 0; c < input_dim; ++c) row[c] = t >= 0 ? x[(size_t)m * input_dim + c] : 0.f;
  } else {
    const int src = SOURCE == FLOPE_TF_FEED_MEAN ? t : m;
    flope_tf_plan::tf_feed_token(t >= 0 && src < vec_rows ? vec7 + (size_t)src * flope_tf_plan::kTfFeedDim : nullptr, input_dim, row);
  }
}

// The last launch of such a step: out_layer's bias into the rows of y [n][out_dim] whose table entry is a code -- what the library
// returns behind a ragged length (tf_scatter_rows).  The rows that fed are left as the forward wrote them.
__global__ void tf_feed_fill_bias(const int* __restrict__ tab, const float* __restrict__ bias, float* __restrict__ y, int out_dim, size_t total) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const size_t r = idx / out_dim;
  if (tab[2 * r] < 0) y[idx] = bias[idx - r * out_dim];
}

// ---- step_split: a token's visible keys over the four waves of a workgroup (option "step_split") -----------------------
// Where the L visible keys of a query lie, counted k = 0 .. L - 1 from its first visible key: the first nc in the track's cache (kv: the
// head's k columns of cache row 0, rows of ld elements; a ring: row (slo + k) % capacity), the others in rows of ldo elements from
// `own` on (the head's k columns of the token's qkv row, or of chunk row tf_extend_chunk0 of an extend).  In both places a row's v
// columns lie d elements behind its k columns.
template <typename T, bool WINDOW> struct TfSplitKeys {
  const T* kv; size_t ld; int nc, slo, capacity;
  const T* own; size_t ldo;
  __device__ __forceinline__ const T* key(int k) const {
    if (k >= nc) return own + (size_t)(k - nc) * ldo;
    int row = k;
    if constexpr (WINDOW) row = flope_tf_plan::tf_split_cache_row(k, slo, capacity);
    return kv + (size_t)row * ld;
  }
};

// softmax(q K^T / sqrt(dh)) V over the L >= 1 keys of `keys` on the four waves of a workgroup, every thread of which calls this with
// the same arguments.  The order, fixed here once for the step and the extend:
//   wave w walks blocks b = w, w + 4, .. of 64 keys (tf_split_wave) in ascending order.  In a block lane l scores key 64 b + l -- one
//   fmaf chain over c = 0 .. dh - 1 from 0.f, * scale, as tf_attn_stream_row -- the block maximum goes across the wave, the running
//   (m, l, o) is rescaled by expf(m - m'), p = expf(score - m') is added to the lane's own l, and the 64 p go to the wave's LDS row.
//   Value pass: the lanes form G = 64 / LPS groups of LPS = dh / VE lanes; group g adds keys g, g + G, .. of the block to its partial
//   o (lane s of the group: dims s VE .. s VE + VE - 1), one 16-byte load per lane and key, the block's loads in flight before their
//   fmafs (at most kTfSplitUnroll at a time).  Behind its last block the wave adds the groups' o by a butterfly (xor 32, 16, .., LPS)
//   and the lanes' l by wave_sum, and leaves (m, l, o) in LDS.
//   Merge, after one workgroup barrier, by lanes 0 .. LPS - 1 of wave 0: M = max of the m of the waves that had a block
//   (tf_split_wave_blocks > 0; the others are skipped by that rule), l and o summed in wave order 0 .. 3 with expf(m_w - M) from 0.f,
//   o * (1 / l), float16 in one rounding (tf_mul_f16_bits), one 16-byte store per lane.
// lds: tf_split_lds(dh) bytes.  Ends with a workgroup barrier, so a caller may call it again.
constexpr int kTfSplitUnroll = 8;
template <typename T, bool WINDOW>
__device__ __forceinline__ void tf_attn_split_row(const TfSplitKeys<T, WINDOW>& keys, const T* q, T* orow, float* lds, int L, int d, int dh, float scale) {
  typedef TfSlice<T, true> Sl;
  constexpr int VE = Sl::VE, KB = flope_tf_plan::kTfSplitBlock, NW = flope_tf_plan::kTfSplitWaves;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int LPS = dh / VE, G = 64 / LPS, g = lane / LPS, c = (lane - g * LPS) * VE;
  float* ps = lds + wave * KB;                      // the block's probabilities
  float* part = lds + NW * KB;                      // [wave][2 + dh]: m, l, o
  const int stride = 2 + dh;
  float m = -INFINITY, l = 0.f, o[VE];
#pragma unroll
  for (int e = 0; e < VE; ++e) o[e] = 0.f;
  const int nb = flope_tf_plan::tf_split_blocks(L);
  for (int b = wave; b < nb; b += NW) {
    const int k0 = b * KB, cnt = L - k0 < KB ? L - k0 : KB;      // keys of this block
    float a = -INFINITY;
    if (lane < cnt) {
      const T* k = keys.key(k0 + lane);
      a = 0.f;
      for (int cc = 0; cc < dh; cc += VE) {
        Sl qv, kx;
        qv.load(q + cc);
        kx.load(k + cc);
#pragma unroll
        for (int e = 0; e < VE; ++e) a = fmaf(qv.f[e], kx.f[e], a);
      }
      a *= scale;
    }
    const float mn = fmaxf(m, wave_max(a));
    const float alpha = expf(m - mn);                // the wave's first block: expf(-inf) = 0 on l = 0, o = 0
    const float p = lane < cnt ? expf(a - mn) : 0.f;
    m = mn;
    l = fmaf(l, alpha, p);
#pragma unroll
    for (int e = 0; e < VE; ++e) o[e] *= alpha;
    ps[lane] = p;
    __builtin_amdgcn_wave_barrier();
    for (int t = g; t < cnt; t += G * kTfSplitUnroll) {          // keys t, t + G, ..: kTfSplitUnroll loads, then their fmafs
      Sl vv[kTfSplitUnroll];
#pragma unroll
      for (int u = 0; u < kTfSplitUnroll; ++u)
        if (t + u * G < cnt) vv[u].load(keys.key(k0 + t + u * G) + d + c);
#pragma unroll
      for (int u = 0; u < kTfSplitUnroll; ++u)
        if (t + u * G < cnt) {
          const float pr = ps[t + u * G];
#pragma unroll
          for (int e = 0; e < VE; ++e) o[e] = fmaf(pr, vv[u].f[e], o[e]);
        }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (wave < nb) {                                   // uniform per wave
    for (int off = 32; off >= LPS; off >>= 1) {
#pragma unroll
      for (int e = 0; e < VE; ++e) o[e] += __shfl_xor(o[e], off);
    }
    l = wave_sum(l);
    float* pw = part + wave * stride;
    if (lane == 0) { pw[0] = m; pw[1] = l; }
    if (lane < LPS) {
#pragma unroll
      for (int e = 0; e < VE; ++e) pw[2 + c + e] = o[e];
    }
  }
  __syncthreads();
  if (threadIdx.x < LPS) {                           // wave 0, group 0: lane s merges dims s VE ..
    const int waves = nb < NW ? nb : NW;
    float M = part[0];
    for (int w = 1; w < waves; ++w) M = fmaxf(M, part[w * stride]);
    float ls = 0.f, os[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) os[e] = 0.f;
    for (int w = 0; w < waves; ++w) {
      const float* pw = part + w * stride;
      const float f = expf(pw[0] - M);
      ls = fmaf(f, pw[1], ls);
#pragma unroll
      for (int e = 0; e < VE; ++e) os[e] = fmaf(f, pw[2 + c + e], os[e]);
    }
    const float inv = 1.f / ls;
    if constexpr (std::is_same<T, f16_t>::value) {
      u32x4 w;
#pragma unroll
      for (int e = 0; e < VE; e += 2) w[e / 2] = tf_mul_f16_bits(os[e], inv) | (tf_mul_f16_bits(os[e + 1], inv) << 16);
      *(u32x4*)(orow + c) = w;
    } else {
      Sl r;
#pragma unroll
      for (int e = 0; e < VE; ++e) r.f[e] = os[e] * inv;
      r.store(orow + c);
    }
  }
  __syncthreads();
}

// tf_attn_step with the row above: workgroup (row r, head h).  The slice store, the table and the memory-safety exit
// (tf_stream_entry_ok; no score row, so no smax) are tf_attn_step's; the exit depends on the workgroup's table entry alone, so a workgroup leaves as one,
// before its first store and before any barrier.  The token's own key and value come from its qkv row, never from the cache row
// stored here.
template <typename T, bool WINDOW>
__global__ __launch_bounds__(256) void tf_attn_step_split(const T* __restrict__ qkv, T* cache, T* __restrict__ att, const int* __restrict__ tab, int n,
                                                          int d, int H, int tracks, int capacity, int W) {
  extern __shared__ __attribute__((aligned(16))) float sc[];     // tf_split_lds(dh)
  const int r = blockIdx.x / H, h = blockIdx.x - r * H, dh = d / H;
  if (r >= n) return;
  const int track = tab[2 * r], pos = tab[2 * r + 1];
  if (!tf_stream_entry_ok<WINDOW>(track, pos, 1, tracks, capacity, W)) return;
  const int slot = WINDOW ? flope_tf_plan::tf_stream_slot(pos, capacity) : pos, lo = WINDOW ? flope_tf_plan::tf_window_lo(pos, W) : 0;
  const float scale = 1.f / sqrtf((float)dh);
  const size_t ld = (size_t)2 * d;
  const T* tok = qkv + (size_t)r * 3 * d + h * dh;
  T* kv = cache + (size_t)track * capacity * ld + h * dh;
  constexpr int VE = TfSlice<T, true>::VE;
  for (int c = threadIdx.x * VE; c < 2 * dh; c += 256 * VE) {    // k slice | v slice of the token -> cache row pos (WINDOW: pos % capacity)
    const int col = c < dh ? c : c - dh + d;
    *(u32x4*)(kv + slot * ld + col) = *(const u32x4*)(tok + d + col);
  }
  const TfSplitKeys<T, WINDOW> keys = {kv, ld, pos - lo, WINDOW ? flope_tf_plan::tf_stream_slot(lo, capacity) : 0, capacity, tok + d, (size_t)3 * d};
  tf_attn_split_row<T, WINDOW>(keys, tok, att + (size_t)r * d + h * dh, sc, pos - lo + 1, d, dh, scale);
}

// tf_attn_extend with the row above: workgroup (sequence b, head h) x blockIdx.y takes queries blockIdx.y, + gridDim.y, .. of the
// sequence, one at a time on its four waves.  Reads the cache, writes att alone (tf_cache_append runs behind it); the exit is
// tf_stream_entry_ok's and uniform for the workgroup, as is the trip count.
template <typename T, bool WINDOW>
__global__ __launch_bounds__(256) void tf_attn_extend_split(const T* __restrict__ qkv, const T* __restrict__ cache, T* __restrict__ att,
                                                            const int* __restrict__ tab, const int* __restrict__ off, int n, int d, int H, int tracks,
                                                            int capacity, int W) {
  extern __shared__ __attribute__((aligned(16))) float sc[];     // tf_split_lds(dh)
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, dh = d / H;
  if (b >= n) return;
  const int track = tab[2 * b], pos0 = tab[2 * b + 1];
  const int o = off[b], len = off[b + 1] - o;
  if (!tf_stream_entry_ok<WINDOW>(track, pos0, len, tracks, capacity, W)) return;
  const float scale = 1.f / sqrtf((float)dh);
  const size_t ld = (size_t)2 * d, ldc = (size_t)3 * d;
  const T* chunk = qkv + (size_t)o * ldc + h * dh;
  const T* kv = cache + (size_t)track * capacity * ld + h * dh;
  for (int i = blockIdx.y; i < len; i += gridDim.y) {
    const int p = pos0 + i, lo = WINDOW ? flope_tf_plan::tf_window_lo(p, W) : 0;
    const TfSplitKeys<T, WINDOW> keys = {kv, ld, flope_tf_plan::tf_extend_cached(pos0, lo), WINDOW ? flope_tf_plan::tf_stream_slot(lo, capacity) : 0, capacity,
                                         chunk + (size_t)flope_tf_plan::tf_extend_chunk0(pos0, lo) * ldc + d, ldc};
    tf_attn_split_row<T, WINDOW>(keys, chunk + (size_t)i * ldc, att + (size_t)(o + i) * d + h * dh, sc, p - lo + 1, d, dh, scale);
  }
}

// ---- MFMA linear: Y[128-token tile][128-feature tile], K walked in 64-wide chunks ----------------------------
// Weights are the MFMA A operand, tokens the B operand (same roles as the conv kernels): a lane ends with one token x
// 16 consecutive features, so bias / residual / ReLU / 16-bit pack happen in registers and leave as 32-byte stores.
// Both operand tiles reach LDS by LDS-DMA (16 B per lane, 1 KiB per wave instruction) into a 2-deep ring:
//   weights: host-packed as the swizzled LDS image ([ntile][chunk][128 rows][128 B]) -> linear copy
//   tokens : swizzle applied on the per-lane source address
// LDS image: row r (128 B = 64 k), 16-byte slot j holds k-chunk j ^ ((r >> 1) & 7)  -> ds_read_b128 conflict-free.
#ifdef FLOPE_STAG_DBG
// diagnostic build: shader-clock stamps of workgroup 0, wave 0 of every tf_gemm_mfma launch {entry, first DMA issued, first chunk landed, K loop done,
// epilogue issued, realtime entry, realtime exit, K | N << 32}; flope_tfdbg_read
__device__ unsigned long long g_tfdbg[8 * 512];
__device__ unsigned g_tfdbg_n;
#define TFDBG_STAMP(i_) do { __builtin_amdgcn_sched_barrier(0); tst[i_] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define TFDBG_STAMP(i_) do {} while (0)
#endif

// ACT (this kernel, tf_gemm_skinny, tf_gemm_skinny_ln): FLOPE_TF_ACT_* of tf_act.h.  ReLU works on the packed 16-bit pair; GELU
// (never with a residual: DESIGN.md 50) is tf_gelu_f32 on the float32 accumulator in front of the pack.
template <typename T, int ACT, bool RES>
__global__ __launch_bounds__(256, 2) void tf_gemm_mfma(const T* __restrict__ X, const void* __restrict__ Wp,
                                                       const float* __restrict__ bias, const T* __restrict__ res,
                                                       T* __restrict__ Y, int K, int N) {
  typedef typename Elem<T>::frag frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [2][ W 16 KiB | X 16 KiB ]
#ifdef FLOPE_STAG_DBG
  unsigned long long tst[5] = {0, 0, 0, 0, 0};
  const unsigned long long trt0 = __builtin_amdgcn_s_memrealtime();
  TFDBG_STAMP(0);
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int ntiles = N >> 7, mt = id / ntiles, nt = id - mt * ntiles, nch = K >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const char* wsrc = (const char*)Wp + (size_t)nt * nch * 16384 + wave * 4096 + lane * 16;
  const char* xsrc = (const char*)X + (size_t)mt * 128 * K * 2;
  int xoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + (lane >> 3), slot = lane & 7;
    xoff[i] = row * K * 2 + ((slot ^ ((row >> 1) & 7)) << 4);
  }
  const int sw = (lane >> 1) & 7;
  const int rdW = (wn * 64 + (lane & 15)) * 128, rdX = 16384 + (wm * 64 + (lane & 15)) * 128;

  const int n0 = nt * 128 + wn * 64 + g * 16;
  f32x4 acc[4][4];
  {
    float bv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) bv[i] = bias[n0 + i];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[pt][ct] = f32x4{bv[ct * 4], bv[ct * 4 + 1], bv[ct * 4 + 2], bv[ct * 4 + 3]};
  }

#define TF_ISSUE(c_, b_)                                                                        \
  do {                                                                                          \
    char* d_ = smem + (b_) * 32768 + wave * 4096;                                               \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) GLDS16(wsrc + (size_t)(c_) * 16384 + i * 1024, d_ + i * 1024); \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) GLDS16(xsrc + (c_) * 128 + xoff[i], d_ + 16384 + i * 1024);    \
  } while (0)

  TF_ISSUE(0, 0);
  TFDBG_STAMP(1);
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) { TF_ISSUE(c + 1, (c + 1) & 1); WAIT_VM(8); } else { WAIT_VM(0); }
    BLOCK_BARRIER();
#ifdef FLOPE_STAG_DBG
    if (c == 0) TFDBG_STAMP(2);
#endif
    const char* bs = smem + (c & 1) * 32768;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int so = ((ks * 4 + g) ^ sw) << 4;
      frag wf[4], xf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        wf[t] = *(const frag*)(bs + rdW + t * 2048 + so);
        xf[t] = *(const frag*)(bs + rdX + t * 2048 + so);
      }
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[pt][ct] = Elem<T>::mfma(wf[ct], xf[pt], acc[pt][ct]);
    }
    BLOCK_BARRIER();
  }
#undef TF_ISSUE
#ifdef FLOPE_STAG_DBG
  { float keep_ = acc[0][0][0]; asm volatile("" : "+v"(keep_)); }
  TFDBG_STAMP(3);
#endif

#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const size_t m = (size_t)mt * 128 + wm * 64 + pt * 16 + (lane & 15);
    const size_t off = m * N + n0;
    float v[16];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int q = 0; q < 4; ++q) v[ct * 4 + q] = acc[pt][ct][q];
    if constexpr (RES) {
      const u32x4 r0 = *(const u32x4*)(res + off), r1 = *(const u32x4*)(res + off + 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q * 2] += unpack_lo<T>(r0[q]); v[q * 2 + 1] += unpack_hi<T>(r0[q]);
        v[8 + q * 2] += unpack_lo<T>(r1[q]); v[8 + q * 2 + 1] += unpack_hi<T>(r1[q]);
      }
    }
    if constexpr (ACT == FLOPE_TF_ACT_GELU) {
      static_assert(!RES, "GELU has no residual form");
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = tf_gelu_f32(v[q]);
    }
    u32x4 o0, o1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o0[q] = pack2<T>(v[q * 2], v[q * 2 + 1]);
      o1[q] = pack2<T>(v[8 + q * 2], v[8 + q * 2 + 1]);
      if constexpr (ACT == FLOPE_TF_ACT_RELU) { o0[q] = pk_relu16(o0[q]); o1[q] = pk_relu16(o1[q]); }
    }
    *(u32x4*)(Y + off) = o0;
    *(u32x4*)(Y + off + 8) = o1;
  }
#ifdef FLOPE_STAG_DBG
  TFDBG_STAMP(4);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned slot = atomicAdd(&g_tfdbg_n, 1u) & 511u;
    for (int i = 0; i < 5; ++i) g_tfdbg[slot * 8 + i] = tst[i];
    g_tfdbg[slot * 8 + 5] = trt0; g_tfdbg[slot * 8 + 6] = __builtin_amdgcn_s_memrealtime(); g_tfdbg[slot * 8 + 7] = (unsigned long long)K | ((unsigned long long)N << 32);
  }
#endif
}

// ---- skinny MFMA linear: at most 32 tokens, one wave per 16-row feature tile of tf_gemm_mfma's packed image (option "skinny") ----
// tf_gemm_mfma gives 1 .. 32 rows ceil(M / 128) N / 128 = 3 .. 12 workgroups at cfg5, each pushing a 128-row token tile through a
// barrier-stepped LDS ring.  Here a wave owns one feature tile (tf_skinny_plan.h: 16 rows of the image, the A operand of one MFMA) and the
// MT token tiles of 16 rows: N / 16 waves, each in a workgroup of its own.  A lane loads its A and B fragments from global memory as 16-byte
// vectors into a register ring of kTfSkinnyDepth chunks, refilled as the MFMAs drain it -- no LDS, no barrier, no word between waves.
// An output element is what it is in tf_gemm_mfma, operation for operation: the accumulator starts at the bias, takes one
// v_mfma_f32_16x16x32 per 32 k with the same 16 feature rows as A and its token in the same column of B, chunks ascending and ks = 0, 1
// inside a chunk, then residual, 16-bit pack, ReLU.  The same bits, so the option changes no result.
// Reads token and residual rows 0 .. 16 MT - 1 (inside the roundup(rows, 128) rows every caller allocates) and writes those rows of Y only.
template <typename T, int ACT, bool RES, int MT>
__global__ __launch_bounds__(64 * flope_tf_plan::kTfSkinnyWaves) void tf_gemm_skinny(const T* __restrict__ X, const void* __restrict__ Wp,
                                                                                     const float* __restrict__ bias, const T* __restrict__ res,
                                                                                     T* __restrict__ Y, int K, int N) {
  typedef typename Elem<T>::frag frag;
  constexpr int D = flope_tf_plan::kTfSkinnyDepth;
  const int lane = threadIdx.x & 63, nch = K >> 6;
  const int ft = flope_tf_plan::tf_skinny_tile(blockIdx.x, threadIdx.x >> 6);
  const char* wsrc = (const char*)Wp + flope_tf_plan::tf_skinny_w_off(ft, 0, 0, lane, nch);
  const int wks = (int)flope_tf_plan::tf_skinny_w_off(ft, 0, 1, lane, nch) - (int)flope_tf_plan::tf_skinny_w_off(ft, 0, 0, lane, nch);
  const char* xsrc[MT];
#pragma unroll
  for (int tt = 0; tt < MT; ++tt) xsrc[tt] = (const char*)X + flope_tf_plan::tf_skinny_x_off(tt, 0, 0, lane, K);
  const int n0 = flope_tf_plan::tf_skinny_feature(ft, lane);

  f32x4 acc[MT];
  {
    const f32x4 bv = *(const f32x4*)(bias + n0);
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) acc[tt] = bv;
  }

  frag wf[D][2], xf[D][MT][2];
  // chunk c_ into ring slot i_: a chunk is 16384 bytes of the image further and 128 bytes along a token row, ks = 1 is 64 bytes along the
  // token row and wks bytes along the (swizzled) image row
#define TF_SK_LOAD(i_, c_)                                                                        \
  do {                                                                                            \
    wf[i_][0] = *(const frag*)(wsrc + (size_t)(c_) * 16384);                                      \
    wf[i_][1] = *(const frag*)(wsrc + (size_t)(c_) * 16384 + wks);                                \
    _Pragma("unroll") for (int tt = 0; tt < MT; ++tt) {                                           \
      xf[i_][tt][0] = *(const frag*)(xsrc[tt] + (size_t)(c_) * 128);                              \
      xf[i_][tt][1] = *(const frag*)(xsrc[tt] + (size_t)(c_) * 128 + 64);                         \
    }                                                                                             \
  } while (0)

#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < nch) TF_SK_LOAD(i, i);
#define TF_SK_MFMA(i_)                                                                            \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                \
    _Pragma("unroll") for (int tt = 0; tt < MT; ++tt) acc[tt] = Elem<T>::mfma(wf[i_][ks], xf[i_][tt][ks], acc[tt])
  int c0 = 0;
  for (; c0 + 2 * D <= nch; c0 += D) {             // a whole turn of the ring with every refill in range: straight-line code, no test per slot
#pragma unroll
    for (int i = 0; i < D; ++i) {
      TF_SK_MFMA(i);
      TF_SK_LOAD(i, c0 + i + D);
    }
  }
  for (; c0 < nch; c0 += D) {                      // the last one or two turns: chunks and refills that end at nch
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int c = c0 + i;
      if (c < nch) {
        TF_SK_MFMA(i);
        if (c + D < nch) TF_SK_LOAD(i, c + D);
      }
    }
  }
#undef TF_SK_MFMA
#undef TF_SK_LOAD

#pragma unroll
  for (int tt = 0; tt < MT; ++tt) {
    const size_t off = (size_t)flope_tf_plan::tf_skinny_x_row(tt, lane) * N + n0;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = acc[tt][q];
    if constexpr (RES) {
      const u32x2 r = *(const u32x2*)(res + off);
      v[0] += unpack_lo<T>(r[0]); v[1] += unpack_hi<T>(r[0]);
      v[2] += unpack_lo<T>(r[1]); v[3] += unpack_hi<T>(r[1]);
    }
    if constexpr (ACT == FLOPE_TF_ACT_GELU) {
      static_assert(!RES, "GELU has no residual form");
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = tf_gelu_f32(v[q]);
    }
    u32x2 o = {pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3])};
    if constexpr (ACT == FLOPE_TF_ACT_RELU) { o[0] = pk_relu16(o[0]); o[1] = pk_relu16(o[1]); }
    *(u32x2*)(Y + off) = o;
  }
}

// ---- ... with the LayerNorm in front of it inside its token load (option "skinny_ln") ----
// Y = act(LayerNorm(X) W^T + b) and H = LayerNorm(X) in one launch, where tf_skinny_ln_ok: K = model_dim <= 64 kTfSkinnyDepth, so the
// whole ring is loaded once and the four lanes (li, g) of token li hold its full pre-norm row, lane g the 16-byte vectors
// 8 chunk + 4 ks + g.  A wave issues its token fragments and its weight fragments, and while the
// weights are on their way turns the token fragments into the normalised, 16-bit-rounded row: per-vector partials by tf_layernorm_vec's
// own definitions (tf_ln_vec_sum / _sq), summed in tf_layernorm_vec's wave_sum order -- the in-lane tree over the ring slots, then the
// lanes at xor 32 and 16 (tf_skinny_plan.h) --, tf_ln_mean / tf_ln_rstd / tf_ln_vec_out.  The fragments then hold the bits
// tf_layernorm_vec would have stored, and the MFMAs and the epilogue are tf_gemm_skinny's: the bits of the two launches.
// Every wave normalises every token (no word between waves); wave ft < K / 64 also stores chunk ft of H.  Statistics stay inside the
// four lanes of a token, so what rows M .. 16 MT - 1 of X hold reaches those rows of H and Y only.  X must not alias H or Y.
// NCH = K / 64 is a template parameter of the wave's work: with the chunk count known, the ring, the tree and the rewrite are straight-line
// code over registers (as a runtime value it put a merge of the whole ring behind every test: five times the instructions)
template <typename T, int ACT, int MT, int NCH>
__device__ __forceinline__ void tf_skinny_ln_wave(const T* __restrict__ X, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  const void* __restrict__ Wp, const float* __restrict__ bias, T* __restrict__ H, T* __restrict__ Y, int N) {
  using namespace flope_tf_plan;
  typedef typename Elem<T>::frag frag;
  constexpr int D = kTfSkinnyDepth, S = kTfSkinnyLnSlots;
  constexpr int nch = NCH, K = 64 * NCH;         // constants: every test on a ring slot below is decided when the kernel is compiled
  const int lane = threadIdx.x & 63;
  const int ft = tf_skinny_tile(blockIdx.x, threadIdx.x >> 6);
  const char* wsrc = (const char*)Wp + tf_skinny_w_off(ft, 0, 0, lane, nch);
  const int wks = (int)tf_skinny_w_off(ft, 0, 1, lane, nch) - (int)tf_skinny_w_off(ft, 0, 0, lane, nch);
  const int n0 = tf_skinny_feature(ft, lane);

  // the whole ring at once, the tokens first: the statistics wait for them alone, the weights arrive under the arithmetic
  u32x4 xr[MT][S];
  frag wf[D][2];
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < nch) {
#pragma unroll
      for (int tt = 0; tt < MT; ++tt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) xr[tt][tf_skinny_ln_slot(i, ks)] = *(const u32x4*)((const char*)X + tf_skinny_x_off(tt, i, ks, lane, K));
    }
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < nch) {
      wf[i][0] = *(const frag*)(wsrc + (size_t)i * 16384);
      wf[i][1] = *(const frag*)(wsrc + (size_t)i * 16384 + wks);
    }
  f32x4 acc[MT];
  {
    const f32x4 bv = *(const f32x4*)(bias + n0);
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) acc[tt] = bv;
  }

  float mean[MT], rstd[MT];
#pragma unroll
  for (int tt = 0; tt < MT; ++tt) {
    float p[S];
#pragma unroll
    for (int sl = 0; sl < S; ++sl) {
      p[sl] = 0.f;
      if ((sl >> 1) < nch) p[sl] = tf_ln_vec_sum<T>(xr[tt][sl], 0.f);
    }
    float s = tf_skinny_ln_lane_tree(p);
    s += __shfl_xor(s, tf_skinny_ln_lane_xor(0));
    s += __shfl_xor(s, tf_skinny_ln_lane_xor(1));
    mean[tt] = tf_ln_mean(s, K);
#pragma unroll
    for (int sl = 0; sl < S; ++sl) {
      p[sl] = 0.f;
      if ((sl >> 1) < nch) p[sl] = tf_ln_vec_sq<T>(xr[tt][sl], mean[tt], 0.f);
    }
    float v = tf_skinny_ln_lane_tree(p);
    v += __shfl_xor(v, tf_skinny_ln_lane_xor(0));
    v += __shfl_xor(v, tf_skinny_ln_lane_xor(1));
    rstd[tt] = tf_ln_rstd(v, K);
  }
  // the fragments in place: a slot's eight gamma / beta columns (two 32-byte loads, the same for both token tiles) only while it is
  // being rewritten -- all K of them at once would be 256 registers at K = 512
#pragma unroll
  for (int sl = 0; sl < S; ++sl)
    if ((sl >> 1) < nch) {
      const int col = tf_skinny_ln_col(sl >> 1, sl & 1, lane);
      const f32x4 w0 = *(const f32x4*)(gamma + col), w1 = *(const f32x4*)(gamma + col + 4);
      const f32x4 b0 = *(const f32x4*)(beta + col), b1 = *(const f32x4*)(beta + col + 4);
      const float w8[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
      const float b8[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
      for (int tt = 0; tt < MT; ++tt) xr[tt][sl] = tf_ln_vec_out<T>(xr[tt][sl], mean[tt], rstd[tt], w8, b8);
    }

  // H: this wave's chunk of the post-norm rows, from its own fragments (the test per slot keeps every register index a constant)
  const int hc = tf_skinny_ln_h_chunk(ft, nch);
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i == hc) {
#pragma unroll
      for (int tt = 0; tt < MT; ++tt)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) *(u32x4*)((char*)H + tf_skinny_ln_h_off(tt, i, ks, lane, K)) = xr[tt][tf_skinny_ln_slot(i, ks)];
    }

  // tf_gemm_skinny's MFMAs in its order: chunks ascending, ks = 0, 1 inside a chunk, the token tiles inside a ks
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < nch) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int tt = 0; tt < MT; ++tt)
          acc[tt] = Elem<T>::mfma(wf[i][ks], __builtin_bit_cast(frag, xr[tt][tf_skinny_ln_slot(i, ks)]), acc[tt]);
    }

#pragma unroll
  for (int tt = 0; tt < MT; ++tt) {
    const size_t off = (size_t)tf_skinny_x_row(tt, lane) * N + n0;
    if constexpr (ACT == FLOPE_TF_ACT_GELU) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[tt][q] = tf_gelu_f32(acc[tt][q]);
    }
    u32x2 o = {pack2<T>(acc[tt][0], acc[tt][1]), pack2<T>(acc[tt][2], acc[tt][3])};
    if constexpr (ACT == FLOPE_TF_ACT_RELU) { o[0] = pk_relu16(o[0]); o[1] = pk_relu16(o[1]); }
    *(u32x2*)(Y + off) = o;
  }
}

template <typename T, int ACT, int MT>
__global__ __launch_bounds__(64 * flope_tf_plan::kTfSkinnyWaves) void tf_gemm_skinny_ln(const T* __restrict__ X, const float* __restrict__ gamma,
                                                                                        const float* __restrict__ beta, const void* __restrict__ Wp,
                                                                                        const float* __restrict__ bias, T* __restrict__ H,
                                                                                        T* __restrict__ Y, int K, int N) {
  static_assert(flope_tf_plan::kTfSkinnyDepth == 8, "one case per chunk count");
  switch (K >> 6) {                                 // tf_skinny_ln_ok: 1 .. kTfSkinnyDepth
#define TF_SKL_CASE(n_) case n_: tf_skinny_ln_wave<T, ACT, MT, n_>(X, gamma, beta, Wp, bias, H, Y, N); break
    TF_SKL_CASE(1); TF_SKL_CASE(2); TF_SKL_CASE(3); TF_SKL_CASE(4); TF_SKL_CASE(5); TF_SKL_CASE(6); TF_SKL_CASE(7); TF_SKL_CASE(8);
#undef TF_SKL_CASE
    default: break;
  }
}

// ---- MFMA attention, 16-bit: head_dim 64 with the keys resident (tf_attn_mfma), head_dim 32 HD32 with the keys streamed (tf_attn_tiled) ----
// A wave owns 32 queries of one (batch, head), Q fragments in registers, and walks the keys 32 at a time in ascending order, K and V
// rows of the step in LDS images (row-major [key][head_dim], rows of RB = 64 HD32 bytes).  One 32-key step (tf_attn16_step):
//   S^T[key][query] = K . Q^T        (A = K rows by ds_read_b128, B = Q fragments kept in registers)
//   online softmax over keys         (in-lane over 8 values, then lanes +16 / +32 that share the query column)
//   O^T[dh][query] += V^T . P^T      (B = P^T straight from the S^T accumulators: k-slot j of lane group g is key
//                                     4g+j (j<4) or 16+4g+(j-4); A = V^T read with ds_read_b64_tr_b16 in the SAME
//                                     permuted key order: two 4-row x 16-column transposed blocks per fragment)
// Both kernels call that one step, so at head_dim 64 their key loops give equal bits by construction; a kernel keeps how the images
// get into LDS, its barriers and which steps it runs.  The epilogue (tf_attn16_store) is tf_attn_tiled's; tf_attn_mfma holds a copy.
// ds_read_b64_tr_b16 needs EXEC all ones: the step has no lane-dependent branch and no early return, and its callers put none
// around it; queries past L are clamped to L - 1 and not stored, keys at or past L hold zeros in the images and their scores become
// -inf before the maximum.  Without WINDOW the first step always holds key 0 < L, so every query's running maximum is finite from
// the first step on, and exp2(-inf - max) is 0, never NaN.  With WINDOW a wave starts at the step that holds the first
// visible key of its FIRST query, and a later query of the wave may see no key of that step: its maximum stays -inf across it, and
// the step subtracts 0 instead of that maximum (msafe below), which keeps its sum and output at exactly 0 until its first own key.
// LDS images (bank = (addr / 4) % 64 for ds_read_b128 and the transposed read; r = key row in its image, c = 16-byte chunk of the
// row; both XORs stay inside an aligned group of four chunks, so rows of 12 chunks are safe; both depend on r & 15 or less, so an
// image may start at any multiple of 16 rows):
//   K rows, ds_read_b128 (a 16-lane group = 16 rows li, eight of them at chunk c0 and eight at c0 ^ 1):
//     64-B and 192-B rows   c ^ (-(r >> 2) & 3)   rows r, r + 4, r + 8, r + 12 start on one slot quad and take its four slots
//     128-B rows            c ^ ((r >> 1) & 7)
//     256-B rows            c ^ (r & 15)
//   V rows, transposed read (a 32-lane half = 8 rows x one 32-byte column pair p; the XOR moves whole pairs, which keeps the 32-byte
//   column pairs of the transposed reads adjacent):
//     64-B and 192-B rows   p ^ ((r >> 2) & 1)    128-B rows  p ^ ((r >> 1) & 3)    256-B rows  p ^ (r & 7)
//   each makes the 8 rows of a half cover the 8 32-byte segments of the 256-byte bank row once.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

template <int HD32> __device__ __forceinline__ int tf_tiled_kswz(int r) {
  return HD32 == 2 ? (r >> 1) & 7 : HD32 == 4 ? r & 15 : (-(r >> 2)) & 3;
}
template <int HD32> __device__ __forceinline__ int tf_tiled_vswz(int r) {
  return (HD32 == 2 ? (r >> 1) & 3 : HD32 == 4 ? r & 7 : (r >> 2) & 1) << 1;
}

// A lane's role in every step: computed once per kernel, in front of the key loop
struct TfAttn16Lane { int g, li, ksw, trp, vrow, vsw; };
template <int HD32> __device__ __forceinline__ TfAttn16Lane tf_attn16_lane(int lane) {
  TfAttn16Lane r;
  r.g = lane >> 4; r.li = lane & 15;
  r.ksw = tf_tiled_kswz<HD32>(r.li);             // K-image swizzle of this lane's key row (row = 16-aligned + li)
  const int trq = r.li >> 2;                     // transposed-read role of this lane inside its 16-lane group
  r.trp = r.li & 3;
  r.vrow = r.g * 4 + trq;                        // ... its V row in a 32-key step (and vrow + 16); the swizzle sees vrow & 7
  r.vsw = tf_tiled_vswz<HD32>(r.vrow);
  return r;
}

// One 32-key step of a wave.  Ki, Vi: the K and V images; kl: the step's first row in them (a multiple of 32), kb: the key that row
// holds; qf: the wave's Q fragments; mrun, lrun, o: running maximum, running sum and unnormalised output of its 2 x 16 queries.
// CAUSAL: q0 is the wave's first query and a key also has to be <= the lane's own query q0 + qt * 16 + li, unclamped (a query past L
// is never stored).  A wave starts at step 0, which holds key 0 <= every query: the running maximum is finite before any step that
// is masked for a query tile as a whole, as above.  Which steps a wave takes is its kernel's business (tf_causal_step_taken).
// WINDOW (with CAUSAL): a key also has to be > the lane's own query - W, the unclamped query again.  The wave's first
// step is tf_window_first_step(q0, W), not 0, so a query whose window starts behind that step sees none of its keys: mx, mrun and
// mnew are all -inf, and exp2(-inf - -inf) would be NaN for good.  The step therefore subtracts msafe = (mnew == -inf ? 0 : mnew) in
// alpha and in the eight exponentials and still keeps mrun = mnew: a query that has seen nothing gets alpha = exp2(-inf) = 0 and
// eight zeros, so lrun = 0 and o = 0 exactly; the first step that holds one of its keys then is a first step (alpha = 0 on zeros);
// where mnew is finite msafe == mnew and no value changes.  Every query below L sees its own key on the diagonal, in a step its wave
// takes, so lrun > 0 at the store for every stored query.  A query at or past L is clamped for its Q rows only, its mask uses the
// unclamped index: all its visible keys may lie at or past L and it may end with lrun = 0 and 1 / lrun = inf -- it is not stored
// (tf_attn16_store's qi < L) and must stay unstored.
// MASKED (without CAUSAL and WINDOW, option mask_mfma): mw[qt] is the word of the compiled mask that belongs to the lane's
// query of tile qt and to this step -- bit j = key kb + j is allowed, kb a multiple of 32 -- and a key also has to have its bit set: the
// key of accumulator element q of S^T tile u in lane group g is kb + 16 u + 4 g + q, so its bit is 16 u + 4 g + q
// (flope_tf_plan::tf_mask_lane_bit).  Which steps a wave takes is its kernel's business again (the classes of the tile map), and as
// under WINDOW a query may see nothing in a step its wave takes, its first one included: the same msafe keeps its state at exactly 0
// until its first own key.  Every stored query has a key in a step its wave takes (the host refuses a row without one), so lrun > 0 at
// the store; a query at or past L takes the word of row L - 1 or ~0 and is not stored.
// BIASED (with MASKED, option bias_mfma): bl(qt, u)[q] is the float32 entry of the compiled bias that belongs to the lane's
// query of tile qt and to key kb + 16 u + 4 g + q (flope_tf_plan::tf_bias16_lane_index).  bl is the kernel's: values it loaded in front
// of the step, or the loads themselves, made per query tile where sixteen live values do not fit (head_dim 128).  The score of a seen key is
// fma(b, log2e, fl(s scale_log2e)) -- the scores live in the log2 domain -- ONE fma with one rounding on top of the product, which keeps the
// rounding it has in every other instantiation: product and fma stand in a block under `#pragma clang fp contract(off)`, so the compiler
// can merge the multiply into nothing (tf_attn_masked_row: the round-to-nearest intrinsics do not achieve that here).  With b = 0 the fma
// returns the product up to the sign of a zero, which reaches no output: a zero bias gives the MASKED bits.  The entry of a pair that is
// not seen may have been loaded (its -inf under a mask bit that is clear, any entry of a key at or past L); the select discards it.
template <typename T, int HD32, bool CAUSAL = false, bool WINDOW = false, bool MASKED = false, bool BIASED = false, typename BL = int>
__device__ __forceinline__ void tf_attn16_step(const char* Ki, const char* Vi, int kb, int kl, int L, int q0, float scale_log2e,
                                               const TfAttn16Lane& ln, const typename Elem<T>::frag (&qf)[2][HD32], float (&mrun)[2],
                                               float (&lrun)[2], f32x4 (&o)[2][2 * HD32], int W = 0, const uint32_t* mw = nullptr,
                                               BL bl = BL()) {
  static_assert(CAUSAL || !WINDOW, "a window without causal has no meaning");
  static_assert(!MASKED || (!CAUSAL && !WINDOW), "a compiled mask says everything itself");
  static_assert(MASKED || !BIASED, "a bias comes with its compiled mask");
  typedef typename Elem<T>::frag frag;
  constexpr int RB = 64 * HD32;
  const int g = ln.g, li = ln.li, ksw = ln.ksw, trp = ln.trp, vrow = ln.vrow, vsw = ln.vsw;
  f32x4 s[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) s[u][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int ks = 0; ks < HD32; ++ks) {
      const frag kf = *(const frag*)(Ki + (kl + u * 16 + li) * RB + (((ks * 4 + g) ^ ksw) << 4));
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) s[u][qt] = Elem<T>::mfma(kf, qf[qt][ks], s[u][qt]);
    }
  frag pf[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float v[8];
    float mx = -INFINITY;
    f32x4 bv[2];
    if constexpr (BIASED) {
      if constexpr (HD32 == 4) __builtin_amdgcn_sched_barrier(0);      // per query tile: the loads stay behind the QK MFMAs and the other tile's pass
      bv[0] = bl(qt, 0); bv[1] = bl(qt, 1);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int key = kb + u * 16 + g * 4 + q;
        bool seen = key < L;
        if constexpr (CAUSAL) seen = seen && key <= q0 + qt * 16 + li;
        if constexpr (WINDOW) seen = seen && key > q0 + qt * 16 + li - W;      // key + W > query, without the overflow of a huge W
        if constexpr (MASKED) seen = seen && ((mw[qt] >> (u * 16 + g * 4 + q)) & 1u);
        float x;
        if constexpr (BIASED) {
#pragma clang fp contract(off)
          const float a = s[u][qt][q] * scale_log2e;
          x = seen ? __builtin_fmaf(bv[u][q], 1.4426950408889634f, a) : -INFINITY;
        } else x = seen ? s[u][qt][q] * scale_log2e : -INFINITY;
        v[u * 4 + q] = x;
        mx = fmaxf(mx, x);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mnew = fmaxf(mrun[qt], mx);
    float msafe = mnew;
    if constexpr (WINDOW || MASKED) msafe = mnew == -INFINITY ? 0.f : mnew;
    const float alpha = __builtin_amdgcn_exp2f(mrun[qt] - msafe);
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = __builtin_amdgcn_exp2f(v[i] - msafe); ps += v[i]; }
    lrun[qt] = lrun[qt] * alpha + ps;
    mrun[qt] = mnew;
#pragma unroll
    for (int dt = 0; dt < 2 * HD32; ++dt) o[qt][dt] *= alpha;
    u32x4 pk;
#pragma unroll
    for (int i = 0; i < 4; ++i) pk[i] = pack2<T>(v[i * 2], v[i * 2 + 1]);
    pf[qt] = __builtin_bit_cast(frag, pk);
  }
#pragma unroll
  for (int dt = 0; dt < 2 * HD32; ++dt) {
    const int a0 = (kl + vrow) * RB + (((dt * 2 + (trp >> 1)) ^ vsw) << 4) + (trp & 1) * 8;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(Vi + a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(Vi + a0 + 16 * RB));
    const s16x8 v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    const frag vf = __builtin_bit_cast(frag, v8);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) o[qt][dt] = Elem<T>::mfma(vf, pf[qt], o[qt][dt]);
  }
}

// ... and behind the last step: o / l of the wave's queries q0 .. q0 + 31 that lie inside the sequence, to columns hcol .. of rows
// row0 + query of out [.][d]
template <typename T, int HD32>
__device__ __forceinline__ void tf_attn16_store(T* out, size_t row0, int d, int hcol, int q0, int L, int lane, const float (&lrun)[2],
                                                const f32x4 (&o)[2][2 * HD32]) {
  const int g = lane >> 4, li = lane & 15;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float lt = lrun[qt];
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
    const float inv = 1.f / lt;
    const int qi = q0 + qt * 16 + li;
    if (qi < L) {
      T* dst = out + (row0 + qi) * d + hcol + g * 4;
#pragma unroll
      for (int dt = 0; dt < 2 * HD32; ++dt) {
        u32x2 w2;
        w2[0] = pack2<T>(o[qt][dt][0] * inv, o[qt][dt][1] * inv);
        w2[1] = pack2<T>(o[qt][dt][2] * inv, o[qt][dt][3] * inv);
        *(u32x2*)(dst + dt * 16) = w2;
      }
    }
  }
}

// tf_attn_mfma: one workgroup per (batch, head); K and V of that head are staged once into LDS (128-byte rows), one __syncthreads,
// then every wave walks all keys.
// VARLEN: launched with pad32(longest) / 32 waves and that much LDS; L and Lp become the sequence's own (the V image starts behind
// its own K image), a wave whose 32 queries lie past the sequence leaves behind the one __syncthreads (a whole wave: EXEC of the
// others stays all ones for the transposed reads).
// CAUSAL: staging and the one __syncthreads as they are; a wave's step loop ends behind the step that holds its last query (the
// bound is the wave's: EXEC stays all ones).
// WINDOW (with CAUSAL, option window_mfma): staging and the one __syncthreads as they are (the image holds every key;
// its staging is shared by all waves); a wave's step loop starts at tf_window_first_step(q0, W) instead of 0, the wave's bound
// again.  Only the WINDOW instantiations read W; it sits where the argument block had four bytes of padding, so every other
// argument, the hidden ones behind them included (blockDim.x of the staging loop), keeps its offset.
template <typename T, bool VARLEN = false, bool CAUSAL = false, bool WINDOW = false>
__global__ __launch_bounds__(1024) void tf_attn_mfma(const T* __restrict__ qkv, T* __restrict__ out, int L, int d,
                                                     int H, int Lp, float scale_log2e, int W, const int* __restrict__ off) {
  static_assert(CAUSAL || !WINDOW, "a window without causal has no meaning");
  typedef typename Elem<T>::frag frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // K image [Lp][128 B] | V image [Lp][128 B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  size_t row0 = 0;
  if constexpr (VARLEN) { row0 = (size_t)off[b]; L = off[b + 1] - off[b]; Lp = (L + 31) / 32 * 32; }
  const T* base = VARLEN ? qkv + row0 * 3 * d + h * 64 : qkv + (size_t)b * L * 3 * d + h * 64;
  char* Ki = smem;
  char* Vi = smem + (size_t)Lp * 128;
  for (int idx = tid; idx < Lp * 8; idx += blockDim.x) {
    const int row = idx >> 3, ch = idx & 7;
    u32x4 kv = {0, 0, 0, 0}, vv = {0, 0, 0, 0};
    if (row < L) {
      const T* src = base + (size_t)row * 3 * d + ch * 8;
      kv = *(const u32x4*)(src + d);
      vv = *(const u32x4*)(src + 2 * d);
    }
    *(u32x4*)(Ki + row * 128 + ((ch ^ tf_tiled_kswz<2>(row)) << 4)) = kv;
    *(u32x4*)(Vi + row * 128 + ((ch ^ tf_tiled_vswz<2>(row)) << 4)) = vv;
  }
  __syncthreads();

  const int q0 = wave * 32;
  if constexpr (VARLEN) { if (q0 >= L) return; }
  frag qf[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    int qi = q0 + qt * 16 + li;
    qi = qi < L ? qi : L - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[qt][ks] = *(const frag*)(base + (size_t)qi * 3 * d + (ks * 4 + g) * 8);
  }
  float mrun[2] = {-INFINITY, -INFINITY}, lrun[2] = {0.f, 0.f};
  f32x4 o[2][4];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const TfAttn16Lane ln = tf_attn16_lane<2>(lane);
  if constexpr (CAUSAL) Lp = flope_tf_plan::tf_causal_keys(q0, 32, Lp);      // min(Lp, q0 + 32): a multiple of 32
  if constexpr (WINDOW) {
    for (int kb = flope_tf_plan::tf_window_first_step(q0, W); kb < Lp; kb += 32)
      tf_attn16_step<T, 2, true, true>(Ki + kb * 128, Vi + kb * 128, kb, 0, L, q0, scale_log2e, ln, qf, mrun, lrun, o, W);
  } else
  for (int kb = 0; kb < Lp; kb += 32) tf_attn16_step<T, 2, CAUSAL>(Ki + kb * 128, Vi + kb * 128, kb, 0, L, q0, scale_log2e, ln, qf, mrun, lrun, o);
  // tf_attn16_store's body, kept as a copy: through the call this kernel allocates 98 VGPRs instead of 96 (5 -> 4 waves per SIMD).
  // Change the expressions here and there together (test_head_dim_64_gives_the_bits_of_the_resident_kernel holds them to equal bits).
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float lt = lrun[qt];
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
    const float inv = 1.f / lt;
    const int qi = q0 + qt * 16 + li;
    if (qi < L) {
      T* dst = out + ((VARLEN ? row0 : (size_t)b * L) + qi) * d + h * 64 + g * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        u32x2 w2;
        w2[0] = pack2<T>(o[qt][dt][0] * inv, o[qt][dt][1] * inv);
        w2[1] = pack2<T>(o[qt][dt][2] * inv, o[qt][dt][3] * inv);
        *(u32x2*)(dst + dt * 16) = w2;
      }
    }
  }
}

// The staging role of a thread in the ring of tf_attn_tiled and tf_attn_tiled_masked (tf_attn16_extend: below): HD32 16-byte
// chunks of K and of V per 64-key block -- key row srow and element ssrc of the block, swizzled bytes sdk / sdv in an LDS stage
// [K block [64][RB] | V block [64][RB]] -- and the registers kr / vr a block waits in between its loads and its LDS writes.  Each kernel
// fills kr / vr in a gload of its own (where a row comes from and when it is zeros is what they differ in); lwrite is the same.
// tf_attn16_extend takes the constants from here and keeps the role written out: see there.
template <int HD32>
struct TfTiledStaging {
  static constexpr int RB = 64 * HD32, NCH = 4 * HD32;             // bytes and 16-byte chunks of a row
  static constexpr int KB = flope_tf_plan::kTfAttnTiledKB, BLK = KB * RB, STAGE = 2 * BLK;
  static_assert(flope_tf_plan::kTfAttnTiledRing == 2 && KB == 64, "the kernels' loops are written for two stages of two 32-key steps");
  int srow[HD32], ssrc[HD32], sdk[HD32], sdv[HD32];
  u32x4 kr[HD32], vr[HD32];
  __device__ __forceinline__ void init(int tid) {
#pragma unroll
    for (int i = 0; i < HD32; ++i) {
      const int idx = tid + i * 256, row = idx / NCH, ch = idx - row * NCH;
      srow[i] = row;
      ssrc[i] = ch * 8;
      sdk[i] = row * RB + ((ch ^ tf_tiled_kswz<HD32>(row)) << 4);
      sdv[i] = BLK + row * RB + ((ch ^ tf_tiled_vswz<HD32>(row)) << 4);
    }
  }
  __device__ __forceinline__ void lwrite(char* s) const {          // s: the stage
#pragma unroll
    for (int i = 0; i < HD32; ++i) {
      *(u32x4*)(s + sdk[i]) = kr[i];
      *(u32x4*)(s + sdv[i]) = vr[i];
    }
  }
};

// tf_attn_tiled (option attn_tiled): K and V streamed instead of resident.  Workgroup = 128 queries of one
// (batch, head): four waves of 32 queries; grid (B H, ceil(L / 128)).  Keys arrive in blocks of kTfAttnTiledKB = 64 (two 32-key
// steps) through a ring of kTfAttnTiledRing = 2 LDS stages (K block | V block).  Register staging: block t + 1 is loaded into VGPRs
// in front of the barrier of block t, stays in flight under block t's MFMAs and is written to the other stage behind them.  One
// barrier per block: it publishes the writes of stage t & 1 and tells that every wave is done reading stage (t + 1) & 1 (block t - 1).
// Keys at or past L: the lane loads row L - 1 instead (never a row past the sequence: the buffer may end at row B L) and writes
// zeros to LDS; a 32-key step that lies wholly past L is skipped by a branch on the step index (the same for every lane: EXEC stays
// all ones, no early return, no lane-dependent branch around the key loop).
// VARLEN: grid.y counts the query blocks of the longest sequence; a workgroup whose first query lies at or past its own sequence's
// length leaves before its first load and barrier (all four waves: the condition is per workgroup), one with some valid queries
// keeps all four waves in the barrier loop as above; nb, the step skip and the masks use the sequence's own L.
// CAUSAL: the barrier loop runs the WORKGROUP's block count, the 64-key blocks up to its last query (tf_causal_tiled_blocks: all
// four waves keep the same trips, loads, LDS writes and barriers); inside it a wave skips the 32-key steps that lie wholly above
// its own last query (tf_causal_step_taken), by the same uniform `continue` as the steps past L.
// WINDOW (with CAUSAL, option window_mfma): the barrier loop runs blocks t0 = tf_window_tiled_first_block .. nb - 1,
// the WORKGROUP's range again (one trip, load and barrier count for its four waves); the blocks below t0 are not loaded.  The loads
// in front of the loop fetch block t0 into stage t0 & 1, so a block's stage is t & 1 from the first block on, as without a window.
// Inside the loop a wave skips the steps outside tf_window_step_taken, the same uniform `continue`.  W is the last argument, behind
// every offset the other instantiations read, and only the WINDOW instantiations read it.
template <typename T, int HD32, bool VARLEN = false, bool CAUSAL = false, bool WINDOW = false>
__global__ __launch_bounds__(256, 2) void tf_attn_tiled(const T* __restrict__ qkv, T* __restrict__ out, int L, int d, int H,
                                                        float scale_log2e, const int* __restrict__ off, int W) {
  static_assert(CAUSAL || !WINDOW, "a window without causal has no meaning");
  typedef typename Elem<T>::frag frag;
  constexpr int HD = 32 * HD32, KB = TfTiledStaging<HD32>::KB, BLK = TfTiledStaging<HD32>::BLK, STAGE = TfTiledStaging<HD32>::STAGE;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [2 stages][K block [64][RB] | V block [64][RB]]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  size_t row0 = 0;
  if constexpr (VARLEN) {
    row0 = (size_t)off[b]; L = off[b + 1] - off[b];
    if ((int)blockIdx.y * flope_tf_plan::kTfAttnTiledQueries >= L) return;
  }
  const T* base = VARLEN ? qkv + row0 * 3 * d + h * HD : qkv + (size_t)b * L * 3 * d + h * HD;
  const int nb = CAUSAL ? flope_tf_plan::tf_causal_tiled_blocks((int)blockIdx.y, L) : (L + KB - 1) / KB;

  TfTiledStaging<HD32> sg;
  sg.init(tid);
  auto gload = [&](int kb0) {
#pragma unroll
    for (int i = 0; i < HD32; ++i) {
      const int row = kb0 + sg.srow[i];
      const T* src = base + (size_t)(row < L ? row : L - 1) * 3 * d + sg.ssrc[i];
      const u32x4 kv = *(const u32x4*)(src + d), vv = *(const u32x4*)(src + 2 * d);
      const u32x4 z = {0, 0, 0, 0};
      sg.kr[i] = row < L ? kv : z;
      sg.vr[i] = row < L ? vv : z;
    }
  };
  int t0 = 0;
  if constexpr (WINDOW) t0 = flope_tf_plan::tf_window_tiled_first_block((int)blockIdx.y, W);
  if constexpr (WINDOW) { gload(t0 * KB); sg.lwrite(smem + (t0 & 1) * STAGE); }
  else { gload(0); sg.lwrite(smem); }

  const int q0 = blockIdx.y * flope_tf_plan::kTfAttnTiledQueries + wave * 32;
  frag qf[2][HD32];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    int qi = q0 + qt * 16 + li;
    qi = qi < L ? qi : L - 1;
#pragma unroll
    for (int ks = 0; ks < HD32; ++ks) qf[qt][ks] = *(const frag*)(base + (size_t)qi * 3 * d + (ks * 4 + g) * 8);
  }
  float mrun[2] = {-INFINITY, -INFINITY}, lrun[2] = {0.f, 0.f};
  f32x4 o[2][2 * HD32];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 2 * HD32; ++dt) o[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const TfAttn16Lane ln = tf_attn16_lane<HD32>(lane);
  for (int t = t0; t < nb; ++t) {
    gload((t + 1) * KB);                         // (past the last block: row L - 1 again, zeros, a stage nobody reads)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BLOCK_BARRIER();
    const char* Ki = smem + (t & 1) * STAGE;
    const char* Vi = Ki + BLK;
#pragma unroll
    for (int st = 0; st < KB / 32; ++st) {
      const int kl = st * 32, kb = t * KB + kl;
      if (kb >= L) continue;                     // uniform: EXEC stays all ones
      if constexpr (CAUSAL) { if (!flope_tf_plan::tf_causal_step_taken(q0, kb)) continue; }     // per wave, uniform
      if constexpr (WINDOW) {
        if (!flope_tf_plan::tf_window_step_taken(q0, kb, W)) continue;                           // per wave, uniform
        tf_attn16_step<T, HD32, true, true>(Ki, Vi, kb, kl, L, q0, scale_log2e, ln, qf, mrun, lrun, o, W);
      } else
      tf_attn16_step<T, HD32, CAUSAL>(Ki, Vi, kb, kl, L, q0, scale_log2e, ln, qf, mrun, lrun, o);
    }
    sg.lwrite(smem + ((t + 1) & 1) * STAGE);
  }
  tf_attn16_store<T, HD32>(out, VARLEN ? row0 : (size_t)b * L, d, h * HD, q0, L, lane, lrun, o);
}

// tf_attn_tiled_masked (option mask_mfma): tf_attn_tiled under a compiled mask.  Workgroup, waves, grid, LDS ring, register
// staging, swizzles, the one barrier per trip and the store are tf_attn_tiled's; what differs is which key blocks a workgroup loads and
// which steps a wave takes, both read from the mask's tile map (tf_attn_mask.h: start, tiles).
// Trips: the barrier loop runs over the entries of the workgroup's query block, tiles[start[qb]] .. tiles[start[qb + 1] - 1] (VARLEN: the
// prefix with 64 kblock < the sequence's own length), a count every wave of the workgroup shares: one load, LDS-write and barrier count.
// The list may skip blocks, so a trip's ring stage is its trip index & 1, not its block index.  The prefetch of the trip past the end
// loads the rows of the last entry again, as zeros, into a stage nobody reads.
// Staging: the rows of entry (kblock, colany); a row at or past L is clamped to row L - 1 and staged as zeros, and so is a row whose colany
// bit is clear, in K and in V: NaN or Inf in a key that no query of the sequence allows reaches no output (0 x NaN in the PV product
// would be NaN).  The scope is the 128-row query block: a key allowed by SOME query of the block is staged as it is, and if it holds NaN
// the rows of that block that mask it get 0 x NaN.
// Steps: a wave reads its class of the step from the entry (wave-uniform).  kTfMaskNone and a step at or past L: the uniform `continue` of
// the causal skip.  kTfMaskAll: mw = ~0 without a load.  kTfMaskSome: the lane loads word kb / 32 of row min(query, L - 1) of the mask
// for its two query tiles -- query and L are the sequence's own, so no word outside the mask is read -- in front of the step's MFMAs.
// Every stored query has a key in a taken step, so lrun > 0 at the store (tf_mask_length_row under VARLEN).
// BIASED (option bias_mfma): BIAS is (const float* bias, int planes, int Lm) -- the handle's float32 planes [planes][Lm][Lm]
// (planes = 1: every head reads plane 0), Lm the mask's seq_len, the row stride whatever the sequence's own length -- and the empty pack
// otherwise: an unbiased instantiation's argument block is byte for byte what it was.  In a taken step, of class "some" or
// "all", the lane loads its sixteen entries in front of the step's MFMAs, where the mask words are loaded: row min(query, n - 1) of plane h
// or 0, columns kb + 16 u + 4 g .. + 3 for u = 0, 1 and both query tiles (flope_tf_plan::tf_bias16_lane_index's arithmetic).  A plane row
// starts on a 4-byte boundary only (Lm is arbitrary), so the 16-byte load is taken where Lm is a multiple of 4 and the step lies inside the
// row (kb + 32 <= Lm; both uniform), and four dword loads with the column clamped to Lm - 1 otherwise: no address outside [0, Lm) of that
// row is formed, whatever lies behind the planes.  An entry of a masked pair may be loaded (-inf) and is never used (tf_attn16_step).
// "none" steps and steps at or past n load nothing.  Head_dim 128 (230 VGPRs of 256 without a bias) loads per query tile inside the step,
// eight values live at a time, by dword loads alone and makes each row address anew: as built it uses all 256 VGPRs and no scratch.
struct TfBias16 { const float* bias; int planes, Lm; };
template <typename T, int HD32, bool VARLEN = false, bool BIASED = false, typename... BIAS>
__global__ __launch_bounds__(256, 2) void tf_attn_tiled_masked(const T* __restrict__ qkv, T* __restrict__ out, int L, int d, int H,
                                                               float scale_log2e, const int* __restrict__ off, int mwords,
                                                               const uint32_t* __restrict__ bits, const int* __restrict__ start,
                                                               const flope_tf_plan::TfMaskTile* __restrict__ tiles, BIAS... bias_args) {
  static_assert(sizeof...(BIAS) == (BIASED ? 3 : 0), "a BIASED instantiation takes (bias, planes, Lm), an unbiased one nothing");
  typedef typename Elem<T>::frag frag;
  constexpr int HD = 32 * HD32, KB = TfTiledStaging<HD32>::KB, BLK = TfTiledStaging<HD32>::BLK, STAGE = TfTiledStaging<HD32>::STAGE;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [2 stages][K block [64][RB] | V block [64][RB]]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, li = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  size_t row0 = 0;
  if constexpr (VARLEN) {
    row0 = (size_t)off[b]; L = off[b + 1] - off[b];
    if ((int)blockIdx.y * flope_tf_plan::kTfAttnTiledQueries >= L) return;
  }
  const T* base = VARLEN ? qkv + row0 * 3 * d + h * HD : qkv + (size_t)b * L * 3 * d + h * HD;
  const int e0 = start[blockIdx.y];
  int e1 = start[blockIdx.y + 1];
  if constexpr (VARLEN) { while (e1 - 1 > e0 && tiles[e1 - 1].kblock * KB >= L) --e1; }      // the corner's prefix; its first entry always stays

  TfTiledStaging<HD32> sg;
  sg.init(tid);
  auto gload = [&](int kb0, uint32_t clo, uint32_t chi) {
#pragma unroll
    for (int i = 0; i < HD32; ++i) {
      const int row = kb0 + sg.srow[i];
      const T* src = base + (size_t)(row < L ? row : L - 1) * 3 * d + sg.ssrc[i];
      const u32x4 kv = *(const u32x4*)(src + d), vv = *(const u32x4*)(src + 2 * d);
      const u32x4 z = {0, 0, 0, 0};
      const bool keep = row < L && (((sg.srow[i] < 32 ? clo : chi) >> (sg.srow[i] & 31)) & 1u);
      sg.kr[i] = keep ? kv : z;
      sg.vr[i] = keep ? vv : z;
    }
  };
  // the entry of a trip, the same for every lane
  auto entry = [&](int e, int& kblock, uint32_t& clo, uint32_t& chi, uint32_t& cls) {
    const flope_tf_plan::TfMaskTile t = tiles[e];
    kblock = __builtin_amdgcn_readfirstlane(t.kblock);
    clo = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.colany_lo);
    chi = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.colany_hi);
    cls = (uint32_t)__builtin_amdgcn_readfirstlane((int)t.cls);
  };
  int kblock, nkblock;
  uint32_t clo, chi, cls, nclo, nchi, ncls;
  entry(e0, kblock, clo, chi, cls);
  gload(kblock * KB, clo, chi);
  sg.lwrite(smem);

  const int q0 = blockIdx.y * flope_tf_plan::kTfAttnTiledQueries + wave * 32;
  frag qf[2][HD32];
  int mrow[2];                                   // the lane's two rows of the mask, in words
  const float* brow[2] = {nullptr, nullptr};     // BIASED, head_dim < 128: ... and of its head's bias plane
  int Lm = 0;
  if constexpr (BIASED) Lm = TfBias16{bias_args...}.Lm;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    int qi = q0 + qt * 16 + li;
    qi = qi < L ? qi : L - 1;
    mrow[qt] = qi * mwords;
    if constexpr (BIASED && HD32 < 4) {
      const TfBias16 t{bias_args...};
      brow[qt] = t.bias + ((size_t)(t.planes > 1 ? h : 0) * t.Lm + (size_t)qi) * t.Lm;
    }
#pragma unroll
    for (int ks = 0; ks < HD32; ++ks) qf[qt][ks] = *(const frag*)(base + (size_t)qi * 3 * d + (ks * 4 + g) * 8);
  }
  float mrun[2] = {-INFINITY, -INFINITY}, lrun[2] = {0.f, 0.f};
  f32x4 o[2][2 * HD32];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 2 * HD32; ++dt) o[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const TfAttn16Lane ln = tf_attn16_lane<HD32>(lane);
  for (int e = e0; e < e1; ++e) {
    const int trip = e - e0;
    if (e + 1 < e1) entry(e + 1, nkblock, nclo, nchi, ncls);
    else { nkblock = kblock; nclo = nchi = ncls = 0; }      // past the last entry: its rows again, zeros, a stage nobody reads
    gload(nkblock * KB, nclo, nchi);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BLOCK_BARRIER();
    const char* Ki = smem + (trip & 1) * STAGE;
    const char* Vi = Ki + BLK;
#pragma unroll
    for (int st = 0; st < KB / 32; ++st) {
      const int kl = st * 32, kb = kblock * KB + kl;
      const int c = flope_tf_plan::tf_mask_tile_class(cls, wave, st);      // per wave, uniform
      if (kb >= L || c == flope_tf_plan::kTfMaskNone) continue;            // uniform: EXEC stays all ones
      uint32_t mw[2] = {~0u, ~0u};
      if (c == flope_tf_plan::kTfMaskSome) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) mw[qt] = bits[mrow[qt] + (kb >> 5)];
      }
      if constexpr (BIASED) {
        // uniform: 16-byte loads where the plane rows start on 16-byte boundaries.  Not at head_dim 128: with both forms of the load in
        // the kernel that instantiation needs scratch (22 VGPRs spilled), with the dword form alone it fits its 256
        const bool vec = HD32 < 4 && flope_tf_plan::tf_bias16_step_vec(Lm, kb);
        auto bload = [&](int qt, int u) {
          const float* row = brow[qt];
          if constexpr (HD32 == 4) {               // the row's address is made anew at every load: no register holds it across the steps
            const TfBias16 t{bias_args...};
            const int qi = q0 + qt * 16 + li;
            row = t.bias + ((size_t)(t.planes > 1 ? h : 0) * t.Lm + (size_t)(qi < L ? qi : L - 1)) * t.Lm;
          }
          f32x4 r;
          if (vec) r = *(const f32x4*)(row + kb + 16 * u + 4 * g);
          else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int col = kb + 16 * u + 4 * g + q;
              r[q] = row[col < Lm ? col : Lm - 1];
            }
          }
          return r;
        };
        if constexpr (HD32 < 4) {                  // sixteen values, loaded in front of the step's MFMAs
          const f32x4 bv[4] = {bload(0, 0), bload(0, 1), bload(1, 0), bload(1, 1)};
          tf_attn16_step<T, HD32, false, false, true, true>(Ki, Vi, kb, kl, L, q0, scale_log2e, ln, qf, mrun, lrun, o, 0, mw,
                                                            [&](int qt, int u) { return bv[2 * qt + u]; });
        } else                                     // head_dim 128: eight live at a time, loaded per query tile inside the step (no scratch)
          tf_attn16_step<T, HD32, false, false, true, true>(Ki, Vi, kb, kl, L, q0, scale_log2e, ln, qf, mrun, lrun, o, 0, mw, bload);
      } else
      tf_attn16_step<T, HD32, false, false, true>(Ki, Vi, kb, kl, L, q0, scale_log2e, ln, qf, mrun, lrun, o, 0, mw);
    }
    sg.lwrite(smem + ((trip + 1) & 1) * STAGE);
    kblock = nkblock; clo = nclo; chi = nchi; cls = ncls;
  }
  tf_attn16_store<T, HD32>(out, VARLEN ? row0 : (size_t)b * L, d, h * HD, q0, L, lane, lrun, o);
}

// tf_attn16_extend (option extend_mfma): flope_tf_stream_extend's attention on tf_attn_tiled's ring and step.  Workgroup
// (sequence b, head h) x blockIdx.y = 128 chunk rows of that sequence, four waves of 32; the query at chunk row i has the ABSOLUTE
// position pos0 + i (tab: (track, pos0) per sequence; off: the packed offsets), so a wave's q0 = pos0 + 128 y + 32 wave is no multiple
// of 32.  Keys are the track's, in absolute 64-key blocks: block t = keys 64 t .. 64 t + 63, from the block that holds lo_wg (the first
// key the workgroup's first query sees; key 0 without a window) to the block that holds its last query.  Staging, swizzles, the one
// barrier per block and the step call are tf_attn_tiled's; what differs is where a key row is loaded from
// (flope_tf_plan::tf_extend_mfma_key): keys >= pos0 from the chunk's packed qkv rows (k at d, v at 2 d of a 3 d row) -- the token's own
// among them, never its cache slot --, keys lo_wg .. pos0 - 1 from the track's cache (k at 0, v at d of a 2 d row; a ring: row
// j % capacity), every other key of a block as ZEROS: a stale cache row may hold NaN, the score mask gives p = 0 there, and 0 x NaN
// in the PV product would be NaN.  The lane then loads chunk row 0, which always exists, and selects zeros, as tf_attn_tiled's gload.
// A query's state in tf_attn16_step depends on its own row alone, a step that is masked for it as a whole leaves it unchanged and
// under WINDOW it stays at exactly 0 until the query's first own key: so the same absolute steps give a chunk row the bits tf_attn_tiled
// / tf_attn_mfma give row pos0 + i of the whole track, whichever queries share its wave.
// Exits, all per workgroup and in front of the first load, store and barrier: tf_stream_entry_ok's (no track, positions that leave the
// cache, a window that is none of this cache's), positions past kTfExtendMfmaPosMax, and a query block behind the chunk.  A workgroup
// with some valid queries keeps all four waves in the barrier loop; queries behind the chunk are clamped for their Q rows and not
// stored.  Reads the cache, writes att alone: tf_cache_append stays behind it (tf_encoder_stream.h).
template <typename T, int HD32, bool WINDOW>
__global__ __launch_bounds__(256, 2) void tf_attn16_extend(const T* __restrict__ qkv, const T* __restrict__ cache, T* __restrict__ att,
                                                           const int* __restrict__ tab, const int* __restrict__ off, int n, int d, int H,
                                                           int tracks, int capacity, float scale_log2e, int W) {
  typedef typename Elem<T>::frag frag;
  typedef TfTiledStaging<HD32> Stg;                                // its constants alone: the role is written out below
  constexpr int HD = 32 * HD32, RB = Stg::RB, NCH = Stg::NCH, KB = Stg::KB, BLK = Stg::BLK, STAGE = Stg::STAGE;
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [2 stages][K block [64][RB] | V block [64][RB]]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, y = (int)blockIdx.y;
  if (b >= n) return;
  const int track = tab[2 * b], pos0 = tab[2 * b + 1];
  const int ob = off[b], len = off[b + 1] - ob;
  if (!tf_stream_entry_ok<WINDOW>(track, pos0, len, tracks, capacity, W) || !flope_tf_plan::tf_extend_mfma_positions_ok(pos0, len)) return;
  if (!flope_tf_plan::tf_extend_mfma_block_live(len, y)) return;
  const int Wk = WINDOW ? W : 0, Labs = pos0 + len;
  const T* chunk = qkv + (size_t)ob * 3 * d + h * HD;                        // chunk row i: k at + d, v at + 2 d
  const T* kv = cache + (size_t)track * capacity * 2 * d + h * HD;           // cache row r: k at + 0, v at + d
  const int t0 = flope_tf_plan::tf_extend_mfma_first_block(pos0, y, Wk), t1 = flope_tf_plan::tf_extend_mfma_last_block(pos0, len, y);

  // staging role: TfTiledStaging's, statement for statement.  Through the struct the four linear instantiations compile to other code
  // in front of and inside the block loop (head_dim 128: 3 instructions fewer, outside the +-2 this merge was held to)
  int srow[HD32], ssrc[HD32], sdk[HD32], sdv[HD32];
#pragma unroll
  for (int i = 0; i < HD32; ++i) {
    const int idx = tid + i * 256, row = idx / NCH, ch = idx - row * NCH;
    srow[i] = row;
    ssrc[i] = ch * 8;
    sdk[i] = row * RB + ((ch ^ tf_tiled_kswz<HD32>(row)) << 4);
    sdv[i] = BLK + row * RB + ((ch ^ tf_tiled_vswz<HD32>(row)) << 4);
  }
  u32x4 kr[HD32], vr[HD32];
  auto gload = [&](int kb0) {
#pragma unroll
    for (int i = 0; i < HD32; ++i) {
      const flope_tf_plan::TfExtendKey key = flope_tf_plan::tf_extend_mfma_key(kb0 + srow[i], pos0, len, capacity, Wk, y);
      const bool cached = key.kind == flope_tf_plan::kTfExtendKeyCache;
      const T* src = (cached ? kv + (size_t)key.row * 2 * d : chunk + (size_t)key.row * 3 * d + d) + ssrc[i];
      const u32x4 kv4 = *(const u32x4*)src, vv4 = *(const u32x4*)(src + d);
      const u32x4 z = {0, 0, 0, 0};
      kr[i] = key.kind == flope_tf_plan::kTfExtendKeyZero ? z : kv4;
      vr[i] = key.kind == flope_tf_plan::kTfExtendKeyZero ? z : vv4;
    }
  };
  auto lwrite = [&](int stage) {
    char* s = smem + stage * STAGE;
#pragma unroll
    for (int i = 0; i < HD32; ++i) {
      *(u32x4*)(s + sdk[i]) = kr[i];
      *(u32x4*)(s + sdv[i]) = vr[i];
    }
  };
  gload(t0 * KB);
  lwrite(t0 & 1);

  const int q0 = flope_tf_plan::tf_extend_mfma_q0(pos0, y, wave);
  frag qf[2][HD32];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    int qi = q0 - pos0 + qt * 16 + li;                                       // the chunk row
    qi = qi < len ? qi : len - 1;
#pragma unroll
    for (int ks = 0; ks < HD32; ++ks) qf[qt][ks] = *(const frag*)(chunk + (size_t)qi * 3 * d + (ks * 4 + g) * 8);
  }
  float mrun[2] = {-INFINITY, -INFINITY}, lrun[2] = {0.f, 0.f};
  f32x4 o[2][2 * HD32];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < 2 * HD32; ++dt) o[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const TfAttn16Lane ln = tf_attn16_lane<HD32>(lane);
  for (int t = t0; t <= t1; ++t) {
    gload((t + 1) * KB);                         // (behind the last block: rows nobody reads, zeros or chunk rows that exist)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BLOCK_BARRIER();
    const char* Ki = smem + (t & 1) * STAGE;
    const char* Vi = Ki + BLK;
#pragma unroll
    for (int st = 0; st < KB / 32; ++st) {
      const int kl = st * 32, kb = t * KB + kl;
      if (!flope_tf_plan::tf_extend_mfma_step_taken(q0, kb, Labs, Wk)) continue;                // per wave, uniform: EXEC stays all ones
      if constexpr (WINDOW) tf_attn16_step<T, HD32, true, true>(Ki, Vi, kb, kl, Labs, q0, scale_log2e, ln, qf, mrun, lrun, o, W);
      else tf_attn16_step<T, HD32, true>(Ki, Vi, kb, kl, Labs, q0, scale_log2e, ln, qf, mrun, lrun, o);
    }
    lwrite((t + 1) & 1);
  }
  // the store's row of query qi is row0 + qi: row0 = ob - pos0 in size_t arithmetic (flope_tf_plan::tf_extend_mfma_out_row)
  tf_attn16_store<T, HD32>(att, (size_t)ob - (size_t)pos0, d, h * HD, q0, Labs, lane, lrun, o);
}

// ---- float32 on the exact-fp32 matrix instruction (FLOPE_DT_F32 with option f32mfma = 1) ---------------------------------
// v_mfma_f32_16x16x4_f32 takes float32 operands and accumulates in float32: every product-sum is an fmaf chain, so these kernels
// differ from tf_linear_generic / tf_attn_generic (option 0, the checker) in summation order only.
//
// tf_linear_f32m: Y[M][N] = X[M][K] W^T + b (+ R) (ReLU).  Weights = A operand, 16 tokens = B operand (as conv_f32m_kernel and
// fc1_packed_kernel).  A lane's 16-byte load is four consecutive k of its weight row / its token, element s feeds MFMA s of a
// 16-deep step on BOTH operands.  K % 4 == 0; the last step of a K that is no multiple of 16 re-reads k = K - 4 .. K - 1 against
// zero weights.  Weights come packed in A-fragment order (host_pack.h pack_tf_f32m): a wave's load of one (step, feature tile)
// is one contiguous KiB.  Wave tile: MP x 16 tokens x 64 features (4 MP independent accumulator tiles); the four waves of a
// workgroup take consecutive token tiles of one 64-feature block and share its weights through L1 / L2.  The last block of an N
// that is no multiple of 64 has nct < 4 feature tiles: the wave computes tile nct - 1 again in their place and does not store it.
// Operands straight from global memory, the next step's loads in flight under this step's MFMAs; no barrier, no split-K, no
// atomics: every output is summed in one k order whatever M, MP, the grid or the batch are.
// Epilogue: accumulators start at the bias (padded to whole blocks); a lane ends with 4 nct consecutive features of its token ->
// residual by 16-byte loads, ReLU, 16-byte stores (element-wise where N % 4 != 0: out_layer); tokens past M are clamped in the
// loop and masked here, features past N masked here.
template <int MP, int ACT, bool RES>
__global__ __launch_bounds__(256) void tf_linear_f32m(const float* __restrict__ X, const float* __restrict__ Wp, const float* __restrict__ bp,
                                                      const float* __restrict__ R, float* __restrict__ Y, int M, int K, int N, int nsteps) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kq = lane >> 4, c16 = lane & 15;
  const int nblk = (N + 63) >> 6;
  const int mtile = blockIdx.x / nblk, blk = blockIdx.x - mtile * nblk;
  const int m0 = (mtile * 4 + wave) * (16 * MP);
  if (m0 >= M) return;                                     // (no barrier below)
  const int nct = min(4, ((N + 15) >> 4) - blk * 4);
  const float* xp[MP];
#pragma unroll
  for (int t = 0; t < MP; ++t) xp[t] = X + (size_t)min(m0 + t * 16 + c16, M - 1) * K;
  const f32x4* const wb = (const f32x4*)Wp + (size_t)blk * nsteps * 256 + lane;
  const int f0 = blk * 64 + kq * 4 * nct;
  int cto[4];
  f32x4 acc[MP][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    cto[ct] = min(ct, nct - 1);
    const f32x4 b = *(const f32x4*)(bp + f0 + cto[ct] * 4);
    cto[ct] *= 64;
#pragma unroll
    for (int t = 0; t < MP; ++t) acc[t][ct] = b;
  }
  auto load = [&](int ks, f32x4 (&x)[MP], f32x4 (&w)[4]) {
    const int ko = min(ks * 16 + 4 * kq, K - 4);
#pragma unroll
    for (int t = 0; t < MP; ++t) x[t] = *(const f32x4*)(xp[t] + ko);
    const f32x4* const ws = wb + ks * nct * 64;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) w[ct] = ws[cto[ct]];
  };
  auto mfma = [&](const f32x4 (&x)[MP], const f32x4 (&w)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < MP; ++t)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[ct][s], x[t][s], acc[t][ct], 0, 0, 0);
  };
  f32x4 xa[MP], wa[4], xb[MP], wc[4];
  // (no load of the loop is conditional and the tail is peeled: behind a conditional load the compiler waits for every load in
  // flight, the step just issued included -- DESIGN.md 14)
  load(0, xa, wa);
  int ks = 0;
  for (; ks + 2 < nsteps; ks += 2) {
    load(ks + 1, xb, wc);
    __builtin_amdgcn_sched_barrier(0);
    mfma(xa, wa);
    __builtin_amdgcn_sched_barrier(0);
    load(ks + 2, xa, wa);
    __builtin_amdgcn_sched_barrier(0);
    mfma(xb, wc);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (ks + 1 < nsteps) {
    load(ks + 1, xb, wc);
    mfma(xa, wa);
    mfma(xb, wc);
  } else {
    mfma(xa, wa);
  }
  // lane (kq, c16): token c16 of each tile x features 64 blk + 4 nct kq + 4 ct + q
  const bool vec = (N & 3) == 0;
#pragma unroll
  for (int t = 0; t < MP; ++t) {
    const int m = m0 + t * 16 + c16;
    if (m >= M) continue;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int f = f0 + ct * 4;
      if (ct >= nct || f >= N) continue;
      const size_t o = (size_t)m * N + f;
      f32x4 v = acc[t][ct];
      if (vec) {
        if constexpr (RES) {
          const f32x4 rv = *(const f32x4*)(R + o);
          v[0] += rv[0]; v[1] += rv[1]; v[2] += rv[2]; v[3] += rv[3];
        }
        if constexpr (ACT == FLOPE_TF_ACT_RELU) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
        if constexpr (ACT == FLOPE_TF_ACT_GELU) { v[0] = tf_gelu_f32(v[0]); v[1] = tf_gelu_f32(v[1]); v[2] = tf_gelu_f32(v[2]); v[3] = tf_gelu_f32(v[3]); }
        *(f32x4*)(Y + o) = v;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (f + q < N) {
            float s = v[q];
            if constexpr (RES) s += R[o + q];
            if constexpr (ACT == FLOPE_TF_ACT_RELU) s = fmaxf(s, 0.f);
            if constexpr (ACT == FLOPE_TF_ACT_GELU) s = tf_gelu_f32(s);
            Y[o + q] = s;
          }
      }
    }
  }
}

// tf_attn_f32m: y32m_attn_kernel (yolo_f32.hip) for any head_dim % 4 == 0 up to 16 NT.  One workgroup = 16 queries of one
// (sequence, head), four waves; q / k / v of head h are columns h dh, d + h dh, 2 d + h dh of the [M][3 d] row.
//   1. scores  S^T[key][query] = K[key][:] . Q[query][:] over head_dim (A = 16 key rows, B = the 16 queries, a lane's 16-byte load
//      = four consecutive dims, element s feeds MFMA s; dims past head_dim: the query fragment is zero and the key load re-reads
//      its last four dims); a wave takes every fourth key tile, two at a time; x scale, into LDS as S[query][key] (row pitch
//      Lp + 4 floats: the value pass reads it conflict-free); keys past L get -3e38;
//   2. softmax over the keys in float32, 16 lanes per query: max, expf, sum, one division, p = e * (1 / l); keys past L get 0;
//   3. values  O^T[dim][query] = V^T[dim][key] . P^T[key][query] (A = 16 dims of V for 4 keys, B = P from LDS; a wave takes every
//      fourth group of 4 keys; the waves' partial sums are added in wave order through LDS).
// Nothing depends on the sequence's position in the batch.  LDS: 16 (Lp + 4) + 3 NT 256 floats, at most kTfAttnLds.
using flope_tf_plan::kTfAttnLds;
// VARLEN: grid.y and the LDS are those of the longest sequence; a workgroup whose 16 queries lie past its own sequence leaves before
// the first barrier; Lp, the score pitch and the place of the partial sums behind the scores follow the sequence's own L.
// CAUSAL: a score also needs key <= its query; the score and value passes stop at the key tile that holds the workgroup's last query
// (tf_causal_f32m_tiles; which wave takes a key stays a function of the key alone), the softmax of query q runs over
// min(L, q + 1) keys and zeroes the rest of those tiles, as it does for keys past L.
template <int NT, bool VARLEN = false, bool CAUSAL = false>
__global__ __launch_bounds__(256) void tf_attn_f32m(const float* __restrict__ qkv, float* __restrict__ out, int L, int d, int H, float scale,
                                                    const int* __restrict__ off) {
  extern __shared__ __attribute__((aligned(16))) float Sm[];      // [16][pitch] scores / probabilities | [3][NT][64][4] partial outputs
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, c16 = lane & 15;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, dh = d / H, q0 = blockIdx.y * 16;
  size_t row0 = 0;
  if constexpr (VARLEN) {
    row0 = (size_t)off[b]; L = off[b + 1] - off[b];
    if (q0 >= L) return;
  }
  const int Lp = (L + 15) & ~15, pitch = Lp + 4, ld = 3 * d;
  const float* const base = VARLEN ? qkv + row0 * ld + h * dh : qkv + (size_t)b * L * ld + h * dh;
  float* const red = Sm + 16 * pitch;
  const int Lw = CAUSAL ? flope_tf_plan::tf_causal_f32m_tiles(q0, L) * 16 : Lp;       // the keys this workgroup walks, whole tiles
  // 1. scores
  {
    f32x4 qf[NT];
    int dimc[NT];
    const float* qp = base + (size_t)min(q0 + c16, L - 1) * ld;
#pragma unroll
    for (int st = 0; st < NT; ++st) {
      const int dim = st * 16 + 4 * kq;
      dimc[st] = min(dim, dh - 4);
      const f32x4 v = *(const f32x4*)(qp + dimc[st]);
      qf[st] = dim < dh ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int ntile = Lw >> 4;
    for (int kt = wave; kt < ntile; kt += 8) {
      const int kt1 = kt + 4;
      const float* kp0 = base + (size_t)min(kt * 16 + c16, L - 1) * ld + d;
      const float* kp1 = base + (size_t)min(kt1 * 16 + c16, L - 1) * ld + d;
      f32x4 k0[NT], k1[NT];
#pragma unroll
      for (int st = 0; st < NT; ++st) { k0[st] = *(const f32x4*)(kp0 + dimc[st]); k1[st] = *(const f32x4*)(kp1 + dimc[st]); }
      f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < NT; ++st)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(k0[st][s], qf[st][s], d0, 0, 0, 0);
          d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(k1[st][s], qf[st][s], d1, 0, 0, 0);
        }
      // lane (kq, c16): keys tile * 16 + 4 kq + r of query c16
      auto seen = [&](int key) { return CAUSAL ? key < L && key <= q0 + c16 : key < L; };
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = seen(kt * 16 + 4 * kq + r) ? d0[r] * scale : -3.0e38f;
      *(f32x4*)(Sm + c16 * pitch + kt * 16 + 4 * kq) = o;
      if (kt1 < ntile) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = seen(kt1 * 16 + 4 * kq + r) ? d1[r] * scale : -3.0e38f;
        *(f32x4*)(Sm + c16 * pitch + kt1 * 16 + 4 * kq) = o;
      }
    }
  }
  __syncthreads();
  // 2. softmax (thread = query tid >> 4, keys tid & 15, + 16, ...)
  {
    const int kl = tid & 15;
    float* Sq = Sm + (tid >> 4) * pitch;
    const int Lq = CAUSAL ? flope_tf_plan::tf_causal_keys(q0 + (tid >> 4), 1, L) : L;      // this query's keys: min(L, q + 1)
    float mx = -3.0e38f;
    for (int j = kl; j < Lq; j += 16) mx = fmaxf(mx, Sq[j]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 16));
    float l = 0.f;
    for (int j = kl; j < Lq; j += 16) { const float e = expf(Sq[j] - mx); Sq[j] = e; l += e; }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) l += __shfl_xor(l, o, 16);
    const float inv = 1.f / l;
    for (int j = kl; j < Lw; j += 16) Sq[j] = j < Lq ? Sq[j] * inv : 0.f;
  }
  __syncthreads();
  // 3. values: group g covers keys 4 g .. 4 g + 3; lane (kq, c16): A = V[4 g + kq][ct * 16 + c16], B = P[query c16][4 g + kq]
  f32x4 acc[NT];
  int dimv[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) { acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f}; dimv[ct] = min(ct * 16 + c16, dh - 1); }
  const int ng = Lw >> 2;
  const float* const vb = base + 2 * d;
  for (int g0 = wave; g0 < ng; g0 += 16) {                 // four groups of this wave per trip
    float av[4][NT], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = g0 + 4 * u, key = min(4 * g + kq, L - 1);
      bv[u] = g < ng ? Sm[c16 * pitch + 4 * g + kq] : 0.f;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) av[u][ct] = vb[(size_t)key * ld + dimv[ct]];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][ct], bv[u], acc[ct], 0, 0, 0);
  }
  if (wave > 0) {
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) *(f32x4*)(red + (((wave - 1) * NT + ct) * 64 + lane) * 4) = acc[ct];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 0; w < 3; ++w)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      const f32x4 r = *(const f32x4*)(red + ((w * NT + ct) * 64 + lane) * 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[ct][q] += r[q];
    }
  // lane (kq, c16): query c16, dims ct * 16 + 4 kq + r
  if (q0 + c16 < L) {
    float* o = out + ((VARLEN ? row0 : (size_t)b * L) + q0 + c16) * d + h * dh + 4 * kq;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
      if (ct * 16 + 4 * kq < dh) *(f32x4*)(o + ct * 16) = acc[ct];
  }
}

// ---- the whole float32 forward of one sequence in one workgroup (option fused) ---------------------------------
// One launch per forward: workgroup b keeps every activation of sequence b in LDS at the offsets of tf_fused_plan.h and walks the
// launch sequence of run_forward<float> phase by phase, a workgroup barrier where that sequence has a kernel boundary.  The result
// is the launch sequence's, bit for bit: every generic float32 kernel computes an element in an order that does not depend on
// which thread computes it, and each phase below calls the definition its kernel calls, float instantiation, on LDS rows --
//   linear with N > 16 or a residual   tf_linear_elem     (tf_linear_generic), elements strided over the 256 threads
//   linear with N <= 16, no residual   tf_rowwave_row     (tf_linear_rowwave), rows strided over the four waves
//   LayerNorm                          tf_layernorm_row   (tf_layernorm), rows strided over the four waves
//   attention                          tf_attn_row        (tf_attn_generic), (head, query) pairs strided over the four waves
// Weights, biases and LayerNorm parameters are read through L2 from the handle's float32 arrays; tab is the device table
// flope_tf_load_weights builds: {embedding w, b, out_layer w, b}, then per layer {in_proj w, b, out_proj w, b, linear1 w, b,
// linear2 w, b, norm1 w, b, norm2 w, b}.
constexpr int kTfFusedTabHead = 4, kTfFusedTabLayer = 12;

// the order launch_linear gives this linear in the float32 launch sequence
__device__ __forceinline__ void tf_fz_linear(const float* X, int xld, const float* W, const float* b, const float* R, int rld, float* Y,
                                             int yld, int M, int K, int N, int act) {
  if (flope_tf_plan::tf_fused_rowwave_order(N, R != nullptr)) {
    for (int m = threadIdx.x >> 6; m < M; m += 4) tf_rowwave_row<float>(X, xld, 1, W, b, Y, yld, 1, m, K, N, act, threadIdx.x & 63);
  } else {
    for (int idx = threadIdx.x; idx < M * N; idx += 256) {
      const int m = idx / N;
      tf_linear_elem<float>(X, xld, 1, W, b, R, rld, Y, yld, 1, m, idx - m * N, K, act);
    }
  }
}

__device__ __forceinline__ void tf_fz_layernorm(const float* in, float* out, const float* w, const float* b, int M, int d) {
  for (int row = threadIdx.x >> 6; row < M; row += 4) tf_layernorm_row<float>(in + row * d, out + row * d, w, b, d, threadIdx.x & 63);
}

// qkv rows of qld floats (q | k | v in the first 3 d), s: this wave's score row
template <bool CAUSAL>
__device__ __forceinline__ void tf_fz_attention(const float* qkv, int qld, float* att, float* s, int L, int d, int H) {
  const int dh = d / H;
  const float scale = 1.f / sqrtf((float)dh);
  for (int it = threadIdx.x >> 6; it < H * L; it += 4) {
    const int h = it / L, i = it - h * L;
    tf_attn_row<float, CAUSAL>(qkv + h * dh, (size_t)qld, att + i * d + h * dh, s, i, L, d, dh, scale, threadIdx.x & 63);
  }
}

// grid = batch, block = 256, dynamic LDS = lay.total (the layout of the longest sequence of the call).  x [batch][L][in_dim] ->
// y [batch][L][out_dim]; off == nullptr: every sequence has L tokens; otherwise sequence b has off[b + 1] - off[b] <= the layout's L
// tokens, rows behind it are not read and come back as out_layer.bias.  CAUSAL: the attention phase calls tf_attn_row's causal form.
template <bool CAUSAL = false>
__global__ __launch_bounds__(256) void tf_fused_f32(const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ off,
                                                    const float* const* __restrict__ tab, const flope_tf_plan::TfFusedLayout lay, int L,
                                                    int in_dim, int d, int out_dim, int H, int nl, int ff) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  const int len = off ? off[b + 1] - off[b] : L;
  float* h = (float*)(smem + lay.h);
  float* h2 = (float*)(smem + lay.h2);
  float* xs = (float*)(smem + lay.x);
  float* qkv = (float*)(smem + lay.qkv);
  float* att = (float*)(smem + lay.att);
  float* sc = (float*)(smem + lay.sc) + (threadIdx.x >> 6) * lay.sc_ld;
  float* ffb = (float*)(smem + lay.ffb);
  const int qld = (int)lay.qkv_ld;
  const float* xb = x + (size_t)b * L * in_dim;
  float* yb = y + (size_t)b * L * out_dim;
  for (int i = threadIdx.x; i < len * in_dim; i += 256) xs[i] = xb[i];
  __syncthreads();
  tf_fz_linear(xs, in_dim, tab[0], tab[1], nullptr, 0, h, d, len, in_dim, d, 0);
  __syncthreads();
  for (int l = 0; l < nl; ++l) {
    const float* const* t = tab + kTfFusedTabHead + l * kTfFusedTabLayer;
    tf_fz_linear(h, d, t[0], t[1], nullptr, 0, qkv, qld, len, d, 3 * d, 0);
    __syncthreads();
    tf_fz_attention<CAUSAL>(qkv, qld, att, sc, len, d, H);
    __syncthreads();
    tf_fz_linear(att, d, t[2], t[3], h, d, h2, d, len, d, d, 0);
    __syncthreads();
    tf_fz_layernorm(h2, h, t[8], t[9], len, d);
    __syncthreads();
    tf_fz_linear(h, d, t[4], t[5], nullptr, 0, ffb, ff, len, d, ff, 1);
    __syncthreads();
    tf_fz_linear(ffb, ff, t[6], t[7], h, d, h2, d, len, ff, d, 0);
    __syncthreads();
    tf_fz_layernorm(h2, h, t[10], t[11], len, d);
    __syncthreads();
  }
  tf_fz_linear(h, d, tab[2], tab[3], nullptr, 0, yb, out_dim, len, d, out_dim, 0);
  const float* ob = tab[3];
  float* pad = yb + (size_t)len * out_dim;
  for (size_t i = threadIdx.x; i < (size_t)(L - len) * out_dim; i += 256) pad[i] = ob[i % out_dim];
}

}  // namespace

// ---- handle ----------------------------------------------------------------------------------------------------
struct TfLinear {
  float* w = nullptr; float* b = nullptr;   // fp32 [N][K], [N]
  void* packed = nullptr;                    // MFMA image (16-bit) when eligible
  float* pk32 = nullptr; float* bpad = nullptr;   // FLOPE_DT_F32, K % 4 == 0: pack_tf_f32m image and the bias padded to whole 64-feature blocks
  int N = 0, K = 0, Kp = 0;                  // Kp: K rounded up to 64 (the packed image's K)
};
struct flope_tf_stream_s;
struct flope_tf_mask;
struct TfLayer { TfLinear in_proj, out_proj, lin1, lin2; float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr; };

struct flope_tf_encoder {
  int device = 0, in_dim = 0, d = 0, out_dim = 0, H = 0, nl = 0, ff = 0, max_tokens = 0, Mpad = 0, dtype = 0, esz = 2;
  int opt_generic = 0;                       // 1: force the generic kernels (A/B checks)
  int opt_f32m = 0;                          // 1: FLOPE_DT_F32 linears and attention on v_mfma_f32_16x16x4_f32 where eligible (stored and ignored by 16-bit handles)
  int opt_tiled = 0;                         // 16-bit handles: 1 = tf_attn_tiled where the choice would be tf_attn_generic, 2 = also in place of tf_attn_mfma (stored and ignored by float32 handles)
  int opt_fused = 0;                         // 1: a float32 forward that tf_fused_ok takes runs as one launch of tf_fused_f32 (stored and ignored by 16-bit handles and while opt_f32m)
  int opt_causal = 0;                        // 1: query i attends to keys j <= i of its own sequence, in every attention launch and in tf_fused_f32
  int opt_window = 0;                        // W > 0 (honoured with opt_causal = 1, refused without): keys i - W < j <= i, on tf_attn_generic unless opt_window_mfma, never tf_fused_f32
  int opt_window_mfma = 0;                   // 1: under causal with a window a 16-bit launch keeps tf_attn_pick's tf_attn_mfma / tf_attn_tiled, their WINDOW instantiations (stored and ignored by float32 handles)
  int opt_step_split = 0;                    // 1: flope_tf_stream_step / _extend split a token's keys over the four waves of a workgroup where tf_step_split_ok (every dtype)
  int opt_bias_mfma = 0;                     // 1: a 16-bit launch under a compiled bias is tf_attn_tiled_masked's BIASED instantiation where tf_attn_pick_biased says so (stored and ignored by float32 handles)
  int opt_mask_mfma = 0;                     // 1: a 16-bit launch under a compiled mask is tf_attn_tiled_masked where tf_attn_pick_masked says so (stored and ignored by float32 handles)
  int opt_extend_mfma = 0;                   // 1: flope_tf_stream_extend's attention is tf_attn16_extend where tf_extend_mfma_ok (stored and ignored by float32 handles); wins over opt_step_split for _extend only
  int last_masked_attn = -1;                 // FLOPE_TF_ATTN_* id of the attention launches of the last flope_tf_forward_masked that enqueued anything (flope_tf_last_forward_masked), -1: none yet
  int last_fwd = FLOPE_TF_FWD_LAUNCHES;       // what the last forward that enqueued anything ran (flope_tf_last_forward)
  const float** fused_tab = nullptr;         // device table of the float32 weight arrays tf_fused_f32 reads (FLOPE_DT_F32 handles, built by flope_tf_load_weights)
  int opt_skinny = 0;                        // 1: a linear that would run tf_gemm_mfma on 1 .. 32 rows runs tf_gemm_skinny, the same bits (stored and ignored by float32 handles)
  int opt_skinny_ln = 0;                     // 1: a LayerNorm directly in front of a skinny linear of K = model_dim <= 512 runs inside that linear's launch (tf_gemm_skinny_ln), the bits of the two launches (stored and ignored where tf_skinny_ln_ok says no, option skinny at 0 included)
  int last_ln_launched = 0, last_ln_folded = 0;   // the stand-alone LayerNorm launches of the last run_forward_with and the LayerNorms it folded (flope_tf_last_ln)
  flope_tf_plan::TfArch arch = {0, FLOPE_TF_ACT_RELU, 0};   // options norm_first / activation / final_norm, fixed once the weights are loaded (tf_arch_plan.h)
  bool arch_fixed = false;                   // set by the first flope_tf_load_weights that succeeds, never cleared
  float *fnw = nullptr, *fnb = nullptr;      // transformer_encoder.norm.weight / .bias where arch.final_norm
  int opt_f32m_lds = 0;                     // KiB of untouched LDS a tf_linear_f32m launch reserves (> 80: one workgroup per CU)
  int cus = 256;
  bool loaded = false;
  TfLinear emb, outl;
  std::vector<TfLayer> layers;
  void *h = nullptr, *h2 = nullptr, *qkv = nullptr, *att = nullptr, *ffb = nullptr;
  void* xin = nullptr;                       // 16-bit zero-padded copy of the fp32 input [Mpad][roundup(in_dim, 64)]
  // ragged batches (flope_tf_*_varlen): packed float32 input [Mpad][in_dim] and output [Mpad][out_dim], the offset table
  // [max_tokens + 1] on the device and the pageable host copy it is uploaded from; all allocated in flope_tf_create
  float *xpk = nullptr, *ypk = nullptr;
  int* vl_off = nullptr;
  std::vector<int> vl_host;
  std::vector<void*> allocs;
  std::vector<flope_tf_stream_s*> streams;   // the open stream states of this handle (flope_tf_stream_open); destroy orphans them
  std::vector<flope_tf_mask*> masks;         // the compiled masks of this handle (flope_tf_mask_create); destroy orphans them
  std::string err;
};

// A stream state (flope_tf_stream_*): the keys and values of `tracks` tracks of up to `capacity` tokens per layer,
// and how many tokens each track holds.  Positions live here, on the host; a call uploads the table of its rows.
struct flope_tf_stream_s {
  flope_tf_encoder* e = nullptr;             // nullptr once the handle is destroyed: every call but close then fails with FLOPE_ESTATE
  int tracks = 0, capacity = 0;
  int window = 0;                            // 0: a linear cache, full at capacity; W >= 1: a ring, row p % capacity, keys p - W < j <= p
  void* cache = nullptr;                     // [num_layers][tracks][capacity][2 model_dim] in the handle's dtype, a row is k | v
  int* tab = nullptr;                        // device table of one call (4 ints per track): step (track, position) per row, prefill the track per sequence, attention both and its fills' offsets
  std::vector<int> pos, tab_host;            // tokens held per track; the pageable copy tab is uploaded from
  std::vector<char> seen;                    // scratch of the argument checks
  float* rel = nullptr;                      // a biased state's distance table (flope_tf_stream_open_bias): float32 [planes][rel_d], nullptr otherwise
  int planes = 0, rel_d = 0;                 // 0 planes: no table; else 1 or num_heads, and rel_d = window ? window : capacity
  // a device-positioned state (flope_tf_stream_open_device): max_rows > 0, window > 0, `pos` stays empty and tab holds
  // 2 max_rows ints, the table tf_stream_feed_kernel writes
  int max_rows = 0;                          // 0: positions on the host, everything above
  int* pos_dev = nullptr;                    // [tracks]: tokens held per track
  float* tok = nullptr;                      // [max_rows][input_dim]: the token rows of the last call
  hipEvent_t ev = nullptr;                   // recorded behind every call that enqueues; the readers wait for it
  int feed_n = 0;                            // rows of the last _step_assoc / _step_tracker
  const void* fed_tracker = nullptr;         // the tracker and the serial number of the update fed last (_step_tracker)
  unsigned long long fed_serial = 0;
};

// A compiled attention mask (flope_tf_mask_*; tf_attn_mask.h): one device allocation bits | first | last | start |
// tiles, and the host copies the per-call checks, the FLOP count and flope_tf_mask_tiles read.
struct flope_tf_mask {
  flope_tf_encoder* e = nullptr;             // nullptr once the handle is destroyed: every call but destroy then fails with FLOPE_ESTATE
  int L = 0;
  long long pairs = 0;
  void* dev = nullptr;                       // uint32 bits [L][words] | int first [L] | int last [L] | int start [nqb + 1] | TfMaskTile tiles [start[nqb]]
  std::vector<uint32_t> bits;
  std::vector<int> first, last;
  std::vector<int> start;                    // the tile map (tf_attn_mask.h), built for every mask: option mask_mfma may be flipped between forwards
  std::vector<flope_tf_plan::TfMaskTile> tiles;
  int planes = 0;                            // 0: a plain mask.  1 or num_heads: a compiled additive bias (flope_tf_bias_create): dev is bits | first | last | float bias [planes][L][L] | start | tiles (the tile map behind the planes: option bias_mfma)
  const float* bias_dev() const { return (const float*)((const char*)dev + flope_tf_plan::tf_bias_dev_bias_at(L)); }
  const uint32_t* bits_dev() const { return (const uint32_t*)dev; }
  const int* first_dev() const { return (const int*)(bits_dev() + bits.size()); }
  const int* last_dev() const { return first_dev() + L; }
  const int* start_dev() const { return (const int*)((const char*)dev + (planes ? flope_tf_plan::tf_bias_dev_start_at(L, planes) : flope_tf_plan::tf_mask_dev_start_at(L))); }
  const flope_tf_plan::TfMaskTile* tiles_dev() const {
    return (const flope_tf_plan::TfMaskTile*)((const char*)dev + (planes ? flope_tf_plan::tf_bias_dev_tiles_at(L, planes) : flope_tf_plan::tf_mask_dev_tiles_at(L)));
  }
};

namespace {

int tf_fail(flope_tf_encoder* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  g_tf_error = msg;
  return code;
}
#define TF_HIP(e, call)                                                                          \
  do {                                                                                           \
    hipError_t _s = (call);                                                                      \
    if (_s != hipSuccess) return tf_fail(e, FLOPE_EHIP, std::string(#call) + ": " + hipGetErrorString(_s)); \
  } while (0)

// f(TfType<T>{}) for the element type T of the handle's dtype (in f: using T = typename decltype(tag)::type)
template <typename T> struct TfType { using type = T; };
template <typename F> int tf_by_dtype(const flope_tf_encoder* e, F&& f) {
  if (e->dtype == FLOPE_DT_F32) return f(TfType<float>{});
  if (e->dtype == FLOPE_DT_F16) return f(TfType<f16_t>{});
  return f(TfType<bf16_t>{});
}

// f(std::integral_constant<int, HD32>{}) for the head_dim = 32 HD32 of a launch on the 16-bit ring kernels (32 / 64 / 96 / 128: their
// picks answer for no other)
template <typename F> void tf_by_hd32(int dh, F&& f) {
  if (dh == 32) f(std::integral_constant<int, 1>{});
  else if (dh == 64) f(std::integral_constant<int, 2>{});
  else if (dh == 96) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

// [N][K] fp32 -> [N/128][K/64][128 rows][8 slots x 8 k] 16-bit, rows permuted so that MFMA row 4g+q of channel tile
// ct is feature 16g + 4ct + q of the wave's 64-feature half, slots pre-swizzled (slot j holds chunk j ^ ((r>>1)&7)).
std::vector<uint16_t> pack_linear(const float* W, int N, int K, int dtype) {
  const int nch = (K + 63) / 64;                       // K zero-padded to a multiple of 64
  std::vector<uint16_t> out((size_t)N * nch * 64);
  for (int nt = 0; nt < N / 128; ++nt)
    for (int c = 0; c < nch; ++c)
      for (int r = 0; r < 128; ++r) {
        const int half = r >> 6, rr = r & 63;
        const int n = nt * 128 + half * 64 + lds_row_to_channel(rr);
        for (int j = 0; j < 8; ++j) {
          const int chunk = j ^ ((r >> 1) & 7);
          uint16_t* dst = &out[(((size_t)nt * nch + c) * 128 + r) * 64 + j * 8];
          const float* src = W + (size_t)n * K + c * 64 + chunk * 8;
          for (int k = 0; k < 8; ++k) dst[k] = cvt16(c * 64 + chunk * 8 + k < K ? src[k] : 0.f, dtype);
        }
      }
  return out;
}

template <typename V> int tf_upload(flope_tf_encoder* e, const V* src, size_t count, void** dst) {
  void* p = nullptr;
  TF_HIP(e, hipMalloc(&p, count * sizeof(V)));
  e->allocs.push_back(p);
  TF_HIP(e, hipMemcpy(p, src, count * sizeof(V), hipMemcpyHostToDevice));
  *dst = p;
  return 0;
}

// One linear under the handle's options; returns the FLOPE_TF_LIN_* id of the kernel launched, or < 0.  The 16-bit vector paths
// (tf_gemm_mfma, tf_linear_rowwave_vec) take X, R and Y 16-byte aligned and, tf_gemm_mfma, allocated for whole 128-row tiles: true of
// the handle's own buffers, checked for a caller's by flope_tf_linear.  plan: nothing is launched and no buffer is read -- the id alone,
// by the same tests (flope_tf_linear_plan; X, R and Y are then looked at for NULL and alignment only).
template <typename T>
int launch_linear(flope_tf_encoder* e, const TfLinear& l, const void* X, int x_f32, const void* R, void* Y, int y_f32,
                  int M, int act, hipStream_t st, bool plan = false) {
  // act: 0 or FLOPE_TF_ACT_*.  GELU works on the accumulator and has no residual form in any kernel
  if (act == FLOPE_TF_ACT_GELU && R) return tf_fail(e, FLOPE_EINVAL, "linear: GELU with a residual has no kernel");
  const bool relu = act == FLOPE_TF_ACT_RELU, gelu = act == FLOPE_TF_ACT_GELU;
  if constexpr (std::is_same<T, float>::value) {
    if (e->opt_f32m && l.pk32 && !(((uintptr_t)X | (uintptr_t)Y | (uintptr_t)R) & 15)) {
      if (plan) return relu && R ? tf_fail(e, FLOPE_EINVAL, "tf_linear_f32m: no ReLU + residual form") : FLOPE_TF_LIN_F32M;
      const size_t lds = (size_t)e->opt_f32m_lds * 1024;
      const int mp = tf_f32m_mp(M, l.N, e->cus * (lds > 80 * 1024 ? 1 : 2)), nsteps = tf_f32m_steps(l.K);
      const dim3 grid((unsigned)((M + 64 * mp - 1) / (64 * mp) * ((l.N + 63) / 64)));
#define TF_GO3(MP_, RELU_, RES_)                                                                                       \
  hipLaunchKernelGGL((tf_linear_f32m<MP_, RELU_, RES_>), grid, dim3(256), lds, st, (const float*)X, l.pk32, l.bpad, \
                     (const float*)R, (float*)Y, M, l.K, l.N, nsteps)
#define TF_GO2(MP_) do { if (gelu) TF_GO3(MP_, FLOPE_TF_ACT_GELU, false); else if (relu && !R) TF_GO3(MP_, FLOPE_TF_ACT_RELU, false); else if (R && !relu) TF_GO3(MP_, 0, true); else if (!R) TF_GO3(MP_, 0, false); else return tf_fail(e, FLOPE_EINVAL, "tf_linear_f32m: no ReLU + residual form"); } while (0)
      if (mp == 4) TF_GO2(4); else if (mp == 2) TF_GO2(2); else TF_GO2(1);
#undef TF_GO2
#undef TF_GO3
      TF_HIP(e, hipGetLastError());
      return FLOPE_TF_LIN_F32M;
    }
  }
  if (l.packed && !y_f32 && !e->opt_generic) {
    if constexpr (!std::is_same<T, float>::value) {
      const bool skinny = flope_tf_plan::tf_skinny_ok(1, e->opt_skinny, e->opt_generic, l.packed != nullptr, y_f32, M);
      if (plan) return skinny ? FLOPE_TF_LIN_SKINNY : FLOPE_TF_LIN_MFMA;
      if (x_f32) {                                   // network input: fp32 [M][K] -> 16-bit [M][Kp]
        const size_t tot = (size_t)M * l.Kp;
        hipLaunchKernelGGL((tf_cast_pad<T>), dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)X, (T*)e->xin, M, l.K, l.Kp);
        X = e->xin;
      }
      if (skinny) {                                  // option "skinny", 1 .. 32 rows: a wave per 16-row feature tile, tf_gemm_mfma's bits
        const int MT = flope_tf_plan::tf_skinny_mt(M);
        const flope_tf_plan::TfSkinnyLaunch sl = flope_tf_plan::tf_skinny_launch(l.N, MT);
#define TF_SK(RELU_, RES_, MT_)                                                                                              \
  hipLaunchKernelGGL((tf_gemm_skinny<T, RELU_, RES_, MT_>), dim3(sl.grid), dim3(sl.block), 0, st, (const T*)X, l.packed, l.b, \
                     (const T*)R, (T*)Y, l.Kp, l.N)
#define TF_SK2(RELU_, RES_) do { if (MT == 1) TF_SK(RELU_, RES_, 1); else TF_SK(RELU_, RES_, 2); } while (0)
        if (gelu) TF_SK2(FLOPE_TF_ACT_GELU, false); else if (relu && R) TF_SK2(FLOPE_TF_ACT_RELU, true); else if (relu) TF_SK2(FLOPE_TF_ACT_RELU, false); else if (R) TF_SK2(0, true); else TF_SK2(0, false);
#undef TF_SK2
#undef TF_SK
        TF_HIP(e, hipGetLastError());
        return FLOPE_TF_LIN_SKINNY;
      }
      const int grid = ((M + 127) / 128) * (l.N / 128);
      const size_t lds = 65536;
#define TF_GO(RELU_, RES_)                                                                                       \
  hipLaunchKernelGGL((tf_gemm_mfma<T, RELU_, RES_>), dim3(grid), dim3(256), lds, st, (const T*)X, l.packed, l.b, \
                     (const T*)R, (T*)Y, l.Kp, l.N)
      if (gelu) TF_GO(FLOPE_TF_ACT_GELU, false); else if (relu && R) TF_GO(FLOPE_TF_ACT_RELU, true); else if (relu) TF_GO(FLOPE_TF_ACT_RELU, false); else if (R) TF_GO(0, true); else TF_GO(0, false);
#undef TF_GO
      TF_HIP(e, hipGetLastError());
      return FLOPE_TF_LIN_MFMA;
    }
  }
  if constexpr (!std::is_same<T, float>::value) {
    if (l.N <= 16 && !R && !x_f32 && l.K % 8 == 0 && (size_t)l.N * l.K * 4 <= 48 * 1024) {
      if (plan) return FLOPE_TF_LIN_ROWWAVE_VEC;
      const int blocks = (M + 7) / 8 < 2048 ? (M + 7) / 8 : 2048;
      hipLaunchKernelGGL((tf_linear_rowwave_vec<T>), dim3(blocks), dim3(256), (size_t)l.N * l.K * 4, st, (const T*)X, l.w, l.b, Y, y_f32, M, l.K, l.N, act);
      TF_HIP(e, hipGetLastError());
      return FLOPE_TF_LIN_ROWWAVE_VEC;
    }
  }
  if (l.N <= 16 && !R) {
    if (plan) return FLOPE_TF_LIN_ROWWAVE;
    const int blocks = (M + 3) / 4 < 8192 ? (M + 3) / 4 : 8192;
    hipLaunchKernelGGL((tf_linear_rowwave<T>), dim3(blocks), dim3(256), 0, st, X, x_f32, l.w, l.b, Y, y_f32, M, l.K, l.N, act);
    TF_HIP(e, hipGetLastError());
    return FLOPE_TF_LIN_ROWWAVE;
  }
  if (plan) return FLOPE_TF_LIN_GENERIC;
  const size_t total = (size_t)M * l.N;
  hipLaunchKernelGGL((tf_linear_generic<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, x_f32, l.w, l.b,
                     R, Y, y_f32, M, l.K, l.N, act);
  TF_HIP(e, hipGetLastError());
  return FLOPE_TF_LIN_GENERIC;
}

// LayerNorm over the last dimension of M rows of d (eps 1e-5, biased variance); returns the FLOPE_TF_LN_* id of the kernel, or < 0
template <typename T>
int launch_layernorm(flope_tf_encoder* e, const void* in, void* out, const float* w, const float* b, int M, hipStream_t st) {
  const int d = e->d;
  int id = FLOPE_TF_LN_SCALAR;
  if (flope_tf_plan::tf_ln_vec_ok(!std::is_same<T, float>::value, d)) id = FLOPE_TF_LN_VEC;
  if constexpr (!std::is_same<T, float>::value) {
    if (id == FLOPE_TF_LN_VEC) hipLaunchKernelGGL((tf_layernorm_vec<T>), dim3((M + 3) / 4), dim3(256), 0, st, (const T*)in, (T*)out, w, b, M, d);
  }
  if (id == FLOPE_TF_LN_SCALAR) hipLaunchKernelGGL((tf_layernorm<T>), dim3((M + 3) / 4), dim3(256), 0, st, (const T*)in, (T*)out, w, b, M, d);
  TF_HIP(e, hipGetLastError());
  return id;
}

// Whether a LayerNorm over model_dim directly in front of linear l on M rows runs inside the linear's launch (option "skinny_ln";
// tf_skinny_plan.h: tf_skinny_ln_ok).  The consumer's form has no residual and a 16-bit result.
template <typename T>
bool tf_linear_ln_ok(const flope_tf_encoder* e, const TfLinear& l, int M) {
  if (std::is_same<T, float>::value) return false;
  return flope_tf_plan::tf_skinny_ln_ok(flope_tf_plan::tf_skinny_ok(1, e->opt_skinny, e->opt_generic, l.packed != nullptr, 0, M), e->opt_skinny_ln, l.K, l.Kp, e->d);
}

// H = LayerNorm(X; gamma, beta), Y = act(H W^T + b) in the one launch of tf_gemm_skinny_ln; the caller has asked tf_linear_ln_ok.
// X, H: [roundup(M, 16)][model_dim] at least, Y the same rows of N; X aliases neither.  Returns FLOPE_TF_LIN_SKINNY_LN, or < 0.
template <typename T>
int launch_linear_ln(flope_tf_encoder* e, const TfLinear& l, const void* X, const float* gamma, const float* beta, void* H, void* Y, int M, int act,
                     hipStream_t st) {
  if constexpr (!std::is_same<T, float>::value) {
    const int MT = flope_tf_plan::tf_skinny_mt(M);
    const flope_tf_plan::TfSkinnyLaunch sl = flope_tf_plan::tf_skinny_launch(l.N, MT);
#define TF_SKL(RELU_, MT_)                                                                                                           \
  hipLaunchKernelGGL((tf_gemm_skinny_ln<T, RELU_, MT_>), dim3(sl.grid), dim3(sl.block), 0, st, (const T*)X, gamma, beta, l.packed, l.b, \
                     (T*)H, (T*)Y, l.Kp, l.N)
#define TF_SKL2(ACT_) do { if (MT == 1) TF_SKL(ACT_, 1); else TF_SKL(ACT_, 2); } while (0)
    if (act == FLOPE_TF_ACT_GELU) TF_SKL2(FLOPE_TF_ACT_GELU); else if (act == FLOPE_TF_ACT_RELU) TF_SKL2(FLOPE_TF_ACT_RELU); else TF_SKL2(0);
#undef TF_SKL2
#undef TF_SKL
    TF_HIP(e, hipGetLastError());
    return FLOPE_TF_LIN_SKINNY_LN;
  }
  return tf_fail(e, FLOPE_EINVAL, "tf_gemm_skinny_ln: 16-bit handles only");
}

// dst = LayerNorm(src; w, b), then Y = act(linear l of dst): the pair as it stands in the forward (src and dst are e->h2 and e->h, in
// the order the architecture gives them: tf_arch_plan.h) -- one launch where tf_linear_ln_ok, the two launches otherwise.  Counts into
// the handle's last_ln_*.
template <typename T>
int tf_ln_then_linear(flope_tf_encoder* e, const float* w, const float* b, const void* src, void* dst, const TfLinear& l, void* Y, int M, int act,
                      hipStream_t st) {
  int rc;
  if (tf_linear_ln_ok<T>(e, l, M)) {
    ++e->last_ln_folded;
    return launch_linear_ln<T>(e, l, src, w, b, dst, Y, M, act, st);
  }
  ++e->last_ln_launched;
  if ((rc = launch_layernorm<T>(e, src, dst, w, b, M, st)) < 0) return rc;
  return launch_linear<T>(e, l, dst, 0, nullptr, Y, 0, M, act, st);
}

// One attention launch: softmax(q k^T / sqrt(head_dim)) v per head.  off == nullptr: qkv [B][L][3 d] -> att [B][L][d].  Otherwise a
// ragged batch: packed qkv [T][3 d] -> att [T][d], sequence b = rows off[b] .. off[b + 1] - 1 (off: the handle's device table), L its
// longest length, the VARLEN instantiations.  Option causal: the CAUSAL instantiations of the same pick.  One kernel for the whole batch, the one tf_attn_plan.h picks for L; grid, block and LDS
// from tf_attn_varlen_launch in both cases.  Option window (with causal): the override sits here -- tf_attn_pick_window's answer:
// tf_attn_generic's WINDOW instantiation whatever tf_attn_pick would say, launched as the generic kernel always is, unless option
// window_mfma keeps tf_attn_pick's tf_attn_mfma / tf_attn_tiled, then their WINDOW instantiations.  Returns the kernel's FLOPE_TF_ATTN_* id, or < 0.
template <typename T>
int launch_attention(flope_tf_encoder* e, const void* qkv, void* att, int B, int L, const int* off, hipStream_t st) {
  using namespace flope_tf_plan;
  const int d = e->d, H = e->H, dh = d / H;
  const bool window = e->opt_causal && e->opt_window > 0;
  const int aligned16 = !(((uintptr_t)qkv | (uintptr_t)att) & 15);
  const int pick = window ? tf_attn_pick_window(e->dtype, dh, L, e->opt_generic, e->opt_f32m, e->opt_tiled, e->opt_window_mfma, aligned16)
                          : tf_attn_pick(e->dtype, dh, L, e->opt_generic, e->opt_f32m, e->opt_tiled, aligned16);
  const TfAttnLaunch l = tf_attn_varlen_launch(pick, dh, B, H, L);
  const dim3 grid(l.grid_x, l.grid_y), block(l.block);
  const int W = window ? e->opt_window : 0;      // kernel, grid, block and LDS of a causal launch are those of the option at 0
  auto launch = [&](auto varlen, auto causal, auto win) {
    constexpr bool VL = decltype(varlen)::value, CA = decltype(causal)::value, WIN = decltype(win)::value;
    if constexpr (!std::is_same<T, float>::value) {
      if (pick == FLOPE_TF_ATTN_MFMA64) {
        hipLaunchKernelGGL((tf_attn_mfma<T, VL, CA, WIN>), grid, block, l.lds, st, (const T*)qkv, (T*)att, L, d, H, tf_attn_pad32(L),
                           1.4426950408889634f / sqrtf(64.f), W, off);
      } else if (pick == FLOPE_TF_ATTN_TILED) {
        const float scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
        tf_by_hd32(dh, [&](auto hd32) {
          hipLaunchKernelGGL((tf_attn_tiled<T, decltype(hd32)::value, VL, CA, WIN>), grid, block, l.lds, st, (const T*)qkv, (T*)att, L, d, H, scale_log2e, off, W);
        });
      }
    }
    if constexpr (std::is_same<T, float>::value && !WIN) {       // no F32M under a window: tf_attn_pick_window never answers it
      if (pick == FLOPE_TF_ATTN_F32M) {
        const int nt = tf_attn_f32m_nt(dh);
        const float scale = 1.f / sqrtf((float)dh);
#define TF_ATT(NT_) hipLaunchKernelGGL((tf_attn_f32m<NT_, VL, CA>), grid, block, l.lds, st, (const float*)qkv, (float*)att, L, d, H, scale, off)
        if (nt == 1) TF_ATT(1); else if (nt == 2) TF_ATT(2); else if (nt == 4) TF_ATT(4); else TF_ATT(8);
#undef TF_ATT
      }
    }
    if (pick == FLOPE_TF_ATTN_GENERIC)
      hipLaunchKernelGGL((tf_attn_generic<T, VL, CA, WIN>), grid, block, l.lds, st, (const T*)qkv, (T*)att, L, d, H, W, off);
  };
  auto by_varlen = [&](auto causal, auto win) {
    if (off) launch(std::true_type{}, causal, win); else launch(std::false_type{}, causal, win);
  };
  if (window) by_varlen(std::true_type{}, std::true_type{});   // a window only under causal
  else if (e->opt_causal) by_varlen(std::true_type{}, std::false_type{});
  else by_varlen(std::false_type{}, std::false_type{});
  TF_HIP(e, hipGetLastError());
  return pick;
}

// A ragged batch as flope_tf_forward_varlen / flope_tf_attention_varlen planned it: T packed tokens, the longest length; the
// offsets are in e->vl_off by the time the first kernel runs (uploaded on the same stream).
struct TfRagged { int T, max_len; };

// Validates and plans a ragged batch into off_host (batch + 1 ints); enqueues nothing.
int tf_check_ragged(flope_tf_encoder* e, const char* who, const int* lengths, int B, int L, int* off_host, TfRagged* rg) {
  int bad = -1;
  const int rc = flope_tf_plan::tf_varlen_plan(lengths, B, L, e->max_tokens, off_host, &rg->T, &rg->max_len, &bad);
  const std::string w(who);
  switch (rc) {
    case flope_tf_plan::kTfVarlenOk: break;
    case flope_tf_plan::kTfVarlenBatch: return tf_fail(e, FLOPE_EINVAL, w + ": batch must be positive and lengths_host non-NULL");
    case flope_tf_plan::kTfVarlenLength:
      return tf_fail(e, FLOPE_EINVAL, w + ": lengths[" + std::to_string(bad) + "] = " + std::to_string(lengths[bad]) + " is outside 1 .. " + std::to_string(L) +
                                          (lengths[bad] == 0 ? " (an empty sequence has no softmax; drop it from the batch)" : ""));
    case flope_tf_plan::kTfVarlenTokens: return tf_fail(e, FLOPE_EINVAL, w + ": the sum of lengths exceeds max_tokens given to flope_tf_create");
    default: return tf_fail(e, FLOPE_EINVAL, w + ": the sum of lengths overflows int");
  }
  return 0;
}

// Validates and plans a ragged batch into e->vl_host and enqueues the upload of its batch + 1 offsets.
int tf_upload_ragged(flope_tf_encoder* e, int B, hipStream_t st) {
  // pageable source: the runtime has staged it when the call returns, so the next call may overwrite vl_host
  TF_HIP(e, hipMemcpyAsync(e->vl_off, e->vl_host.data(), (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  return 0;
}
int tf_plan_ragged(flope_tf_encoder* e, const char* who, const int* lengths, int B, int L, hipStream_t st, TfRagged* rg) {
  int rc;
  if ((rc = tf_check_ragged(e, who, lengths, B, L, e->vl_host.data(), rg))) return rc;
  return tf_upload_ragged(e, B, st);
}

// rg == nullptr: the fixed-length forward, x [B][L][in] -> y [B][L][out].  Otherwise the ragged one: the valid rows of x are gathered
// into rg->T packed rows, every linear and LayerNorm runs on those, attention per sequence, and the result is scattered into y.
// attention(li): what stands between in_proj and out_proj of layer li (qkv of the M rows in e->qkv -> e->att); < 0 ends the forward.
template <typename T, typename ATT>
int run_forward_with(flope_tf_encoder* e, const float* x, int B, int L, float* y, hipStream_t st, const TfRagged* rg, ATT&& attention) {
  using namespace flope_tf_plan;
  const int M = rg ? rg->T : B * L;
  int rc;
  e->last_ln_launched = e->last_ln_folded = 0;
  // the order, the buffers and the activation are the architecture's op list (tf_arch_plan.h), stated there alone
  const int nops = tf_arch_op_count(e->arch, e->nl);
  auto buf = [&](int b) -> void* { return b == kTfBufH ? e->h : b == kTfBufH2 ? e->h2 : b == kTfBufQkv ? e->qkv : b == kTfBufAtt ? e->att : b == kTfBufFfb ? e->ffb : nullptr; };
  auto lin = [&](const TfOp& o) -> const TfLinear& {
    const TfLayer& ly = e->layers[o.layer < 0 ? 0 : o.layer];
    return o.name == kTfLinInProj ? ly.in_proj : o.name == kTfLinOutProj ? ly.out_proj : o.name == kTfLinLinear1 ? ly.lin1 : ly.lin2;
  };
  // op 0, the embedding, from the caller's float32 rows
  if (rg) {
    const bool cast = !std::is_same<T, float>::value && e->emb.packed && !e->opt_generic;     // where launch_linear would run tf_cast_pad
    const int Kp = cast ? e->emb.Kp : e->in_dim;
    const size_t tot = (size_t)B * L * Kp;
    const dim3 grid((unsigned)((tot + 255) / 256));
    if (cast) hipLaunchKernelGGL((tf_gather_rows<T>), grid, dim3(256), 0, st, x, (T*)e->xin, e->vl_off, L, e->in_dim, Kp, tot);
    else hipLaunchKernelGGL((tf_gather_rows<float>), grid, dim3(256), 0, st, x, e->xpk, e->vl_off, L, e->in_dim, Kp, tot);
    TF_HIP(e, hipGetLastError());
    if ((rc = launch_linear<T>(e, e->emb, cast ? (const void*)e->xin : (const void*)e->xpk, cast ? 0 : 1, nullptr, e->h, 0, M, 0, st)) < 0) return rc;
  } else if ((rc = launch_linear<T>(e, e->emb, x, 1, nullptr, e->h, 0, M, 0, st)) < 0) return rc;
  // ops 1 .. nops - 2.  A LayerNorm the list marks `fold` stands directly in front of the linear that reads it: the pair option
  // skinny_ln may run as one launch (tf_ln_then_linear); every other LayerNorm is a launch of its own
  for (int i = 1; i + 1 < nops; ++i) {
    const TfOp o = tf_arch_op(e->arch, e->nl, i);
    if (o.kind == kTfOpAttention) {
      if ((rc = attention(o.layer)) < 0) return rc;
    } else if (o.kind == kTfOpLayerNorm) {
      const float* w = o.name == kTfLnFinal ? e->fnw : o.name == kTfLnNorm1 ? e->layers[o.layer].n1w : e->layers[o.layer].n2w;
      const float* b = o.name == kTfLnFinal ? e->fnb : o.name == kTfLnNorm1 ? e->layers[o.layer].n1b : e->layers[o.layer].n2b;
      if (o.fold) {
        const TfOp n = tf_arch_op(e->arch, e->nl, ++i);       // the linear behind it: in = o.out, no residual
        if ((rc = tf_ln_then_linear<T>(e, w, b, buf(o.in), buf(o.out), lin(n), buf(n.out), M, n.act, st)) < 0) return rc;
      } else {
        ++e->last_ln_launched;
        if ((rc = launch_layernorm<T>(e, buf(o.in), buf(o.out), w, b, M, st)) < 0) return rc;
      }
    } else if ((rc = launch_linear<T>(e, lin(o), buf(o.in), 0, buf(o.res), buf(o.out), 0, M, o.act, st)) < 0) return rc;
  }
  // the last op, out_layer, into the caller's float32 rows
  const void* last = buf(tf_arch_op(e->arch, e->nl, nops - 1).in);
  if (!rg) return (rc = launch_linear<T>(e, e->outl, last, 0, nullptr, y, 1, M, 0, st)) < 0 ? rc : 0;
  if ((rc = launch_linear<T>(e, e->outl, last, 0, nullptr, e->ypk, 1, M, 0, st)) < 0) return rc;
  const size_t tot = (size_t)B * L * e->out_dim;
  hipLaunchKernelGGL(tf_scatter_rows, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, (const float*)e->ypk, (const float*)e->outl.b, y, e->vl_off, L,
                     e->out_dim, tot);
  TF_HIP(e, hipGetLastError());
  return 0;
}

// ... with launch_attention there: flope_tf_forward and flope_tf_forward_varlen
template <typename T>
int run_forward(flope_tf_encoder* e, const float* x, int B, int L, float* y, hipStream_t st, const TfRagged* rg = nullptr) {
  return run_forward_with<T>(e, x, B, L, y, st, rg, [&](int) {
    return launch_attention<T>(e, e->qkv, e->att, B, rg ? rg->max_len : L, rg ? e->vl_off : nullptr, st);
  });
}

// Option fused: whether a float32 forward whose longest sequence has Lmax tokens runs as the single launch (never under option window)
bool tf_fused_pick(const flope_tf_encoder* e, int Lmax) {
  // tf_fused_f32 is the default architecture's order alone
  return e->fused_tab && e->opt_window == 0 && flope_tf_plan::tf_arch_default(e->arch) && flope_tf_plan::tf_fused_ok(e->dtype, e->opt_fused, e->opt_f32m, e->in_dim, e->d, e->ff, Lmax);
}

// ... and that launch: x [B][L][in] -> y [B][L][out], one workgroup per sequence.  off == nullptr: every sequence has L = Lmax tokens;
// otherwise the handle's device offset table of a ragged batch whose longest sequence has Lmax <= L tokens.
int launch_fused(flope_tf_encoder* e, const float* x, int B, int L, int Lmax, const int* off, float* y, hipStream_t st) {
  const flope_tf_plan::TfFusedLayout lay = flope_tf_plan::tf_fused_layout(e->in_dim, e->d, e->ff, Lmax);
#define TF_FZ(CA_) hipLaunchKernelGGL((tf_fused_f32<CA_>), dim3((unsigned)B), dim3(256), (size_t)lay.total, st, x, y, off, (const float* const*)e->fused_tab, lay, L, \
                                      e->in_dim, e->d, e->out_dim, e->H, e->nl, e->ff)
  if (e->opt_causal) TF_FZ(true); else TF_FZ(false);
#undef TF_FZ
  TF_HIP(e, hipGetLastError());
  return 0;
}

// One forward, fixed-length (rg == nullptr) or ragged: the single launch where tf_fused_pick takes it, the launch sequence otherwise;
// last_fwd records which.
int tf_forward(flope_tf_encoder* e, const float* x, int B, int L, float* y, hipStream_t st, const TfRagged* rg) {
  const int Lmax = rg ? rg->max_len : L;
  e->last_fwd = FLOPE_TF_FWD_LAUNCHES;
  if (tf_fused_pick(e, Lmax)) {
    const int rc = launch_fused(e, x, B, L, Lmax, rg ? e->vl_off : nullptr, y, st);
    if (!rc) e->last_fwd = FLOPE_TF_FWD_FUSED;
    return rc;
  }
  return tf_by_dtype(e, [&](auto tag) { return run_forward<typename decltype(tag)::type>(e, x, B, L, y, st, rg); });
}

// Option window is honoured with causal only: every entry point that runs or plans a forward or an attention of the handle's options refuses the pair (window > 0, causal = 0)
int tf_check_window(flope_tf_encoder* e, const std::string& who) {
  if (e->opt_window > 0 && !e->opt_causal)
    return tf_fail(e, FLOPE_EINVAL, who + ": option window = " + std::to_string(e->opt_window) + " needs option causal = 1 (a window without causal is refused)");
  return 0;
}

// The argument checks of a fixed-length forward under the caller's name (flope_tf_forward, and flope_tf_forward_plan, which has no
// buffers: bufs = true).  *empty: an empty batch, nothing to do.
int tf_check_forward(flope_tf_encoder* e, const std::string& who, int batch, int seq_len, bool bufs, bool* empty) {
  *empty = false;
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (!e->loaded) return tf_fail(e, FLOPE_ESTATE, who + ": weights not loaded");
  if (batch < 0 || seq_len < 0) return tf_fail(e, FLOPE_EINVAL, who + ": negative size");
  if (batch == 0 || seq_len == 0) { *empty = true; return 0; }     // buffers may be NULL
  if (!bufs) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  if ((long long)batch * seq_len > e->max_tokens)
    return tf_fail(e, FLOPE_EINVAL, who + ": batch*seq_len exceeds max_tokens given to flope_tf_create");
  return 0;
}

// ... and of a ragged one, up to the lengths (tf_check_ragged / tf_plan_ragged)
int tf_check_forward_varlen(flope_tf_encoder* e, const std::string& who, int batch, int seq_len, bool bufs) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (!e->loaded) return tf_fail(e, FLOPE_ESTATE, who + ": weights not loaded");
  if (!bufs) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  if (seq_len < 1) return tf_fail(e, FLOPE_EINVAL, who + ": non-positive seq_len");
  const size_t widest = (size_t)(e->emb.Kp > e->out_dim ? e->emb.Kp : e->out_dim);
  if (batch > 0 && (size_t)batch * seq_len > (size_t)INT32_MAX * 256 / widest)          // the row-copy kernels' grids
    return tf_fail(e, FLOPE_EINVAL, who + ": batch*seq_len too large for one launch");
  return 0;
}

}  // namespace

extern "C" const char* flope_tf_last_error(flope_tf_handle h) { return h ? h->err.c_str() : g_tf_error.c_str(); }

extern "C" int flope_tf_create(int device_id, int input_dim, int model_dim, int out_dim, int num_heads, int num_layers,
                               int ff_dim, int max_tokens, int dtype, flope_tf_handle* out) {
  if (!out) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_create: NULL out");
  *out = nullptr;
  if (input_dim < 1 || model_dim < 1 || out_dim < 1 || num_heads < 1 || num_layers < 0 || ff_dim < 1 || max_tokens < 1)
    return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_create: non-positive dimension");
  if (model_dim % num_heads)
    return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_create: model_dim must be divisible by num_heads (torch.nn.MultiheadAttention)");
  if (dtype != FLOPE_DT_BF16 && dtype != FLOPE_DT_F16 && dtype != FLOPE_DT_F32)
    return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_create: dtype must be FLOPE_DT_BF16 / F16 / F32");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: no HIP device (there is no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_create: bad device id");
  flope_tf_encoder* e = new flope_tf_encoder();
  e->device = device_id; e->in_dim = input_dim; e->d = model_dim; e->out_dim = out_dim; e->H = num_heads;
  e->nl = num_layers; e->ff = ff_dim; e->max_tokens = max_tokens; e->dtype = dtype; e->esz = dtype == FLOPE_DT_F32 ? 4 : 2;
  e->Mpad = (max_tokens + 127) / 128 * 128;
  e->layers.resize(num_layers);
  auto fin = [&](int rc) { flope_tf_destroy(e); return rc; };
  if (hipSetDevice(device_id) != hipSuccess) return fin(tf_fail(nullptr, FLOPE_EHIP, "hipSetDevice failed"));
  const size_t in_pad = (size_t)(input_dim + 63) / 64 * 64;
  struct { void** p; size_t cols; } bufs[] = {{&e->xin, in_pad}, {&e->h, (size_t)model_dim}, {&e->h2, (size_t)model_dim}, {&e->qkv, (size_t)3 * model_dim},
                                              {&e->att, (size_t)model_dim}, {&e->ffb, (size_t)ff_dim}};
  for (auto& bf : bufs) {
    const size_t bytes = (size_t)e->Mpad * bf.cols * e->esz;
    if (hipMalloc(bf.p, bytes) != hipSuccess) return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipMalloc failed"));
    e->allocs.push_back(*bf.p);
    if (hipMemset(*bf.p, 0, bytes) != hipSuccess) return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipMemset failed"));
  }
  {                                                  // ragged batches: nothing is allocated in a forward
    struct { void** p; size_t bytes; } vb[] = {{(void**)&e->xpk, (size_t)e->Mpad * input_dim * sizeof(float)}, {(void**)&e->ypk, (size_t)e->Mpad * out_dim * sizeof(float)},
                                               {(void**)&e->vl_off, ((size_t)max_tokens + 1) * sizeof(int)}};
    for (auto& bf : vb) {
      if (hipMalloc(bf.p, bf.bytes) != hipSuccess) return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipMalloc failed"));
      e->allocs.push_back(*bf.p);
      if (hipMemset(*bf.p, 0, bf.bytes) != hipSuccess) return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipMemset failed"));
    }
    e->vl_host.assign((size_t)max_tokens + 1, 0);
  }
  {                                                  // per create: the attribute is per device (a process-wide flag would leave a second GPU without it)
    hipFuncSetAttribute((const void*)tf_attn_mfma<f16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<f16_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<bf16_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<f16_t, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<bf16_t, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<f16_t, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<bf16_t, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<f16_t, false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<bf16_t, false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<f16_t, true, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    hipFuncSetAttribute((const void*)tf_attn_mfma<bf16_t, true, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072);
    // every instantiation launch_linear launches: ACT 0 / ReLU with and without a residual, GELU without one
#define TF_ATTR(T_, A_, B_) hipFuncSetAttribute((const void*)tf_gemm_mfma<T_, A_, B_>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536)
    TF_ATTR(f16_t, 0, false); TF_ATTR(f16_t, 0, true); TF_ATTR(f16_t, FLOPE_TF_ACT_RELU, false); TF_ATTR(f16_t, FLOPE_TF_ACT_RELU, true);
    TF_ATTR(bf16_t, 0, false); TF_ATTR(bf16_t, 0, true); TF_ATTR(bf16_t, FLOPE_TF_ACT_RELU, false); TF_ATTR(bf16_t, FLOPE_TF_ACT_RELU, true);
    TF_ATTR(f16_t, FLOPE_TF_ACT_GELU, false); TF_ATTR(bf16_t, FLOPE_TF_ACT_GELU, false);
#undef TF_ATTR
    // tf_linear_f32m reserves up to 160 KiB under option f32mlds: the GELU instantiations as the others
#define TF_F32M(MP_) (const void*)tf_linear_f32m<MP_, 0, false>, (const void*)tf_linear_f32m<MP_, FLOPE_TF_ACT_RELU, false>, (const void*)tf_linear_f32m<MP_, 0, true>, \
                     (const void*)tf_linear_f32m<MP_, FLOPE_TF_ACT_GELU, false>
    const void* const f32m[] = {TF_F32M(4), TF_F32M(2), TF_F32M(1),
                                (const void*)tf_attn_f32m<1>, (const void*)tf_attn_f32m<2>, (const void*)tf_attn_f32m<4>, (const void*)tf_attn_f32m<8>,
                                (const void*)tf_attn_f32m<1, true>, (const void*)tf_attn_f32m<2, true>, (const void*)tf_attn_f32m<4, true>, (const void*)tf_attn_f32m<8, true>,
                                (const void*)tf_attn_f32m<1, false, true>, (const void*)tf_attn_f32m<2, false, true>, (const void*)tf_attn_f32m<4, false, true>,
                                (const void*)tf_attn_f32m<8, false, true>, (const void*)tf_attn_f32m<1, true, true>, (const void*)tf_attn_f32m<2, true, true>,
                                (const void*)tf_attn_f32m<4, true, true>, (const void*)tf_attn_f32m<8, true, true>};
#undef TF_F32M
    for (const void* f : f32m)
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTfAttnLds) != hipSuccess)
        return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipFuncSetAttribute failed"));
    // tf_attn_tiled: 16 / 32 / 48 / 64 KiB; the widest sits at the 64 KiB a launch gets without asking
    const void* const tiled[] = {(const void*)tf_attn_tiled<f16_t, 4>, (const void*)tf_attn_tiled<bf16_t, 4>,
                                 (const void*)tf_attn_tiled<f16_t, 4, true>, (const void*)tf_attn_tiled<bf16_t, 4, true>,
                                 (const void*)tf_attn_tiled<f16_t, 4, false, true>, (const void*)tf_attn_tiled<bf16_t, 4, false, true>,
                                 (const void*)tf_attn_tiled<f16_t, 4, true, true>, (const void*)tf_attn_tiled<bf16_t, 4, true, true>,
                                 (const void*)tf_attn_tiled<f16_t, 4, false, true, true>, (const void*)tf_attn_tiled<bf16_t, 4, false, true, true>,
                                 (const void*)tf_attn_tiled<f16_t, 4, true, true, true>, (const void*)tf_attn_tiled<bf16_t, 4, true, true, true>};
    for (const void* f : tiled)
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)flope_tf_plan::tf_attn_tiled_lds(128)) != hipSuccess)
        return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipFuncSetAttribute failed"));
    const void* const ext16[] = {(const void*)tf_attn16_extend<f16_t, 4, false>, (const void*)tf_attn16_extend<bf16_t, 4, false>,
                                 (const void*)tf_attn16_extend<f16_t, 4, true>, (const void*)tf_attn16_extend<bf16_t, 4, true>};
    for (const void* f : ext16)
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)flope_tf_plan::tf_attn_tiled_lds(128)) != hipSuccess)
        return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipFuncSetAttribute failed"));
    const void* const masked16[] = {(const void*)tf_attn_tiled_masked<f16_t, 4>, (const void*)tf_attn_tiled_masked<bf16_t, 4>,
                                    (const void*)tf_attn_tiled_masked<f16_t, 4, true>, (const void*)tf_attn_tiled_masked<bf16_t, 4, true>};
    const void* const biased16[] = {(const void*)tf_attn_tiled_masked<f16_t, 4, false, true, const float*, int, int>,
                                    (const void*)tf_attn_tiled_masked<bf16_t, 4, false, true, const float*, int, int>,
                                    (const void*)tf_attn_tiled_masked<f16_t, 4, true, true, const float*, int, int>,
                                    (const void*)tf_attn_tiled_masked<bf16_t, 4, true, true, const float*, int, int>};
    for (const void* f : biased16)
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)flope_tf_plan::tf_attn_tiled_lds(128)) != hipSuccess)
        return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipFuncSetAttribute failed"));
    for (const void* f : masked16)
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)flope_tf_plan::tf_attn_tiled_lds(128)) != hipSuccess)
        return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipFuncSetAttribute failed"));
#define TF_MASKED(BI_) (const void*)tf_attn_masked<float, false, BI_>, (const void*)tf_attn_masked<float, true, BI_>, (const void*)tf_attn_masked<f16_t, false, BI_>, \
                       (const void*)tf_attn_masked<f16_t, true, BI_>, (const void*)tf_attn_masked<bf16_t, false, BI_>, (const void*)tf_attn_masked<bf16_t, true, BI_>
    const void* const masked[] = {TF_MASKED(false), TF_MASKED(true)};
#undef TF_MASKED
    for (const void* f : masked)                     // four score rows of up to max_tokens floats and the mask words behind them
      if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTfAttnLds) != hipSuccess)
        return fin(tf_fail(nullptr, FLOPE_EHIP, "flope_tf_create: hipFuncSetAttribute failed"));
    if (hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || e->cus < 1) e->cus = 256;
  }
  *out = e;
  return FLOPE_OK;
}

extern "C" int flope_tf_destroy(flope_tf_handle e) {
  if (!e) return FLOPE_OK;
  hipSetDevice(e->device);
  for (flope_tf_stream_s* s : e->streams) {      // their device memory goes with the handle; the states stay until closed and refuse every call
    hipFree(s->cache); hipFree(s->tab); hipFree(s->rel); hipFree(s->pos_dev); hipFree(s->tok);
    if (s->ev) { hipEventSynchronize(s->ev); hipEventDestroy(s->ev); }
    s->cache = nullptr; s->tab = nullptr; s->rel = nullptr; s->pos_dev = nullptr; s->tok = nullptr; s->ev = nullptr; s->e = nullptr;
  }
  for (flope_tf_mask* m : e->masks) {            // the same for the compiled masks
    hipFree(m->dev);
    m->dev = nullptr; m->e = nullptr;
  }
  for (void* p : e->allocs) hipFree(p);
  delete e;
  return FLOPE_OK;
}

extern "C" int flope_tf_set_option(flope_tf_handle e, const char* name, int value) {
  if (!e || !name) return FLOPE_EINVAL;
  if (!strcmp(name, "generic")) { const int old = e->opt_generic; e->opt_generic = value ? 1 : 0; return old; }
  if (!strcmp(name, "f32mfma")) { const int old = e->opt_f32m; e->opt_f32m = value ? 1 : 0; return old; }
  if (!strcmp(name, "attn_tiled")) {
    if (value < 0 || value > 2) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: attn_tiled is 0, 1 or 2");
    const int old = e->opt_tiled; e->opt_tiled = value; return old;
  }
  if (!strcmp(name, "fused")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: fused is 0 or 1");
    const int old = e->opt_fused; e->opt_fused = value; return old;
  }
  if (!strcmp(name, "causal")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: causal is 0 or 1");
    const int old = e->opt_causal; e->opt_causal = value; return old;
  }
  if (!strcmp(name, "window")) {
    if (value < 0) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: window is 0 (none) or a positive key count");
    const int old = e->opt_window; e->opt_window = value; return old;
  }
  if (!strcmp(name, "window_mfma")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: window_mfma is 0 or 1");
    const int old = e->opt_window_mfma; e->opt_window_mfma = value; return old;
  }
  if (!strcmp(name, "mask_mfma")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: mask_mfma is 0 or 1");
    const int old = e->opt_mask_mfma; e->opt_mask_mfma = value; return old;
  }
  if (!strcmp(name, "bias_mfma")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: bias_mfma is 0 or 1");
    const int old = e->opt_bias_mfma; e->opt_bias_mfma = value; return old;
  }
  if (!strcmp(name, "step_split")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: step_split is 0 or 1");
    const int old = e->opt_step_split; e->opt_step_split = value; return old;
  }
  if (!strcmp(name, "skinny")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: skinny is 0 or 1");
    const int old = e->opt_skinny; e->opt_skinny = value; return old;
  }
  if (!strcmp(name, "skinny_ln")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: skinny_ln is 0 or 1");
    const int old = e->opt_skinny_ln; e->opt_skinny_ln = value; return old;
  }
  if (!strcmp(name, "extend_mfma")) {
    if (value < 0 || value > 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: extend_mfma is 0 or 1");
    const int old = e->opt_extend_mfma; e->opt_extend_mfma = value; return old;
  }
  // the architecture (tf_arch_plan.h): stated before the weights are loaded, fixed afterwards
  if (!strcmp(name, "norm_first") || !strcmp(name, "activation") || !strcmp(name, "final_norm")) {
    int* field = name[0] == 'n' ? &e->arch.norm_first : name[0] == 'a' ? &e->arch.act : &e->arch.final_norm;
    const bool ok = name[0] == 'a' ? (value == FLOPE_TF_ACT_RELU || value == FLOPE_TF_ACT_GELU) : (value == 0 || value == 1);
    if (!ok) return tf_fail(e, FLOPE_EINVAL, std::string("flope_tf_set_option: ") + name + (name[0] == 'a' ? " is 1 (ReLU) or 2 (GELU, the erf form)" : " is 0 or 1"));
    if (e->arch_fixed) return tf_fail(e, FLOPE_ESTATE, std::string("flope_tf_set_option: ") + name + " is fixed once flope_tf_load_weights has succeeded");
    const int old = *field; *field = value; return old;
  }
  if (!strcmp(name, "f32mlds")) {
    if (value < 0 || value > 160) return tf_fail(e, FLOPE_EINVAL, "flope_tf_set_option: f32mlds is 0 .. 160 (KiB)");
    const int old = e->opt_f32m_lds; e->opt_f32m_lds = value; return old;
  }
  return tf_fail(e, FLOPE_EINVAL, std::string("flope_tf_set_option: unknown option ") + name);
}

extern "C" int flope_tf_load_weights(flope_tf_handle e, int n, const char* const* names, const float* const* host_ptrs,
                                     const int* ndims, const int64_t* const* shapes) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_load_weights: NULL handle");
  if (n < 0 || (n > 0 && (!names || !host_ptrs || !ndims || !shapes)))
    return tf_fail(e, FLOPE_EINVAL, "flope_tf_load_weights: NULL argument");
  TF_HIP(e, hipSetDevice(e->device));
  e->loaded = false;
  std::map<std::string, std::pair<const float*, std::vector<int64_t>>> ts;
  for (int i = 0; i < n; ++i) {
    if (!names[i] || !host_ptrs[i] || ndims[i] < 0 || ndims[i] > 8 || (ndims[i] > 0 && !shapes[i]))
      return tf_fail(e, FLOPE_EINVAL, "flope_tf_load_weights: malformed entry " + std::to_string(i));
    ts[names[i]] = std::make_pair(host_ptrs[i], std::vector<int64_t>(shapes[i], shapes[i] + ndims[i]));
  }
  auto get = [&](const std::string& name, std::vector<int64_t> want, const float** p) -> int {
    auto it = ts.find(name);
    if (it == ts.end()) return tf_fail(e, FLOPE_EWEIGHTS, "state_dict entry missing: " + name);
    if (it->second.second != want) return tf_fail(e, FLOPE_EWEIGHTS, "state_dict entry has the wrong shape: " + name);
    size_t cnt = 1;
    for (int64_t s : want) cnt *= (size_t)s;
    for (size_t i = 0; i < cnt; ++i)
      if (!std::isfinite(it->second.first[i])) return tf_fail(e, FLOPE_EWEIGHTS, "non-finite value in " + name);
    *p = it->second.first;
    return 0;
  };
  auto linear = [&](const std::string& wn, const std::string& bn, int N, int K, TfLinear* l) -> int {
    const float *w, *b;
    int rc;
    if ((rc = get(wn, {N, K}, &w)) || (rc = get(bn, {N}, &b))) return rc;
    l->N = N; l->K = K;
    if ((rc = tf_upload(e, w, (size_t)N * K, (void**)&l->w)) || (rc = tf_upload(e, b, (size_t)N, (void**)&l->b))) return rc;
    l->Kp = (K + 63) / 64 * 64;
    // 16-bit activations have row stride K, so only the fp32 network input (re-laid out by tf_cast_pad) may need padding
    if (e->dtype != FLOPE_DT_F32 && N % 128 == 0 && (K % 64 == 0 || l == &e->emb)) {
      const std::vector<uint16_t> pk = pack_linear(w, N, K, e->dtype);
      if ((rc = tf_upload(e, pk.data(), pk.size(), &l->packed))) return rc;
    }
    if (e->dtype == FLOPE_DT_F32 && K % 4 == 0) {      // both images: option f32mfma flips between forwards without a reload
      const std::vector<float> pk = pack_tf_f32m(w, N, K);
      std::vector<float> bp((size_t)(N + 63) / 64 * 64, 0.f);
      memcpy(bp.data(), b, (size_t)N * sizeof(float));
      if ((rc = tf_upload(e, pk.data(), pk.size(), (void**)&l->pk32)) || (rc = tf_upload(e, bp.data(), bp.size(), (void**)&l->bpad))) return rc;
    }
    return 0;
  };
  auto vec = [&](const std::string& name, int N, float** dst) -> int {
    const float* p;
    int rc;
    if ((rc = get(name, {N}, &p))) return rc;
    return tf_upload(e, p, (size_t)N, (void**)dst);
  };
  int rc;
  if ((rc = linear("embedding.weight", "embedding.bias", e->d, e->in_dim, &e->emb))) return rc;
  for (int i = 0; i < e->nl; ++i) {
    const std::string p = "transformer_encoder.layers." + std::to_string(i) + ".";
    TfLayer& ly = e->layers[i];
    if ((rc = linear(p + "self_attn.in_proj_weight", p + "self_attn.in_proj_bias", 3 * e->d, e->d, &ly.in_proj)) ||
        (rc = linear(p + "self_attn.out_proj.weight", p + "self_attn.out_proj.bias", e->d, e->d, &ly.out_proj)) ||
        (rc = linear(p + "linear1.weight", p + "linear1.bias", e->ff, e->d, &ly.lin1)) ||
        (rc = linear(p + "linear2.weight", p + "linear2.bias", e->d, e->ff, &ly.lin2)) ||
        (rc = vec(p + "norm1.weight", e->d, &ly.n1w)) || (rc = vec(p + "norm1.bias", e->d, &ly.n1b)) ||
        (rc = vec(p + "norm2.weight", e->d, &ly.n2w)) || (rc = vec(p + "norm2.bias", e->d, &ly.n2b)))
      return rc;
  }
  if (e->arch.final_norm &&
      ((rc = vec("transformer_encoder.norm.weight", e->d, &e->fnw)) || (rc = vec("transformer_encoder.norm.bias", e->d, &e->fnb))))
    return rc;
  if ((rc = linear("out_layer.weight", "out_layer.bias", e->out_dim, e->d, &e->outl))) return rc;
  if (e->fused_tab) {                                  // a reload replaces the table (the weight arrays themselves stay until destroy, as before)
    for (auto it = e->allocs.begin(); it != e->allocs.end(); ++it)
      if (*it == (void*)e->fused_tab) { e->allocs.erase(it); break; }
    hipFree((void*)e->fused_tab);
    e->fused_tab = nullptr;
  }
  if (e->dtype == FLOPE_DT_F32) {                      // tf_fused_f32's table: 4 + 12 num_layers device pointers
    std::vector<const float*> tab = {e->emb.w, e->emb.b, e->outl.w, e->outl.b};
    for (const TfLayer& ly : e->layers)
      for (const float* p : {(const float*)ly.in_proj.w, (const float*)ly.in_proj.b, (const float*)ly.out_proj.w, (const float*)ly.out_proj.b,
                             (const float*)ly.lin1.w, (const float*)ly.lin1.b, (const float*)ly.lin2.w, (const float*)ly.lin2.b,
                             (const float*)ly.n1w, (const float*)ly.n1b, (const float*)ly.n2w, (const float*)ly.n2b})
        tab.push_back(p);
    if ((rc = tf_upload(e, tab.data(), tab.size(), (void**)&e->fused_tab))) return rc;
  }
  TF_HIP(e, hipDeviceSynchronize());
  e->loaded = e->arch_fixed = true;
  return FLOPE_OK;
}

extern "C" int flope_tf_forward(flope_tf_handle e, const float* x_dev, int batch, int seq_len, float* y_dev, void* stream) {
  bool empty;
  int rc;
  if ((rc = tf_check_forward(e, "flope_tf_forward", batch, seq_len, x_dev && y_dev, &empty)) || empty) return rc;
  if ((rc = tf_check_window(e, "flope_tf_forward"))) return rc;
  TF_HIP(e, hipSetDevice(e->device));
  return tf_forward(e, x_dev, batch, seq_len, y_dev, (hipStream_t)stream, nullptr);
}

extern "C" int flope_tf_attention(flope_tf_handle e, const void* qkv_dev, int batch, int seq_len, void* out_dev, void* stream) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_attention: NULL handle");
  if (int rc = tf_check_window(e, "flope_tf_attention")) return rc;
  if (batch < 1 || seq_len < 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_attention: non-positive size");
  if (!qkv_dev || !out_dev) return tf_fail(e, FLOPE_EINVAL, "flope_tf_attention: NULL buffer");
  if ((long long)batch * seq_len > e->max_tokens)
    return tf_fail(e, FLOPE_EINVAL, "flope_tf_attention: batch*seq_len exceeds max_tokens given to flope_tf_create");
  if (((uintptr_t)qkv_dev | (uintptr_t)out_dev) & (uintptr_t)(e->esz - 1))
    return tf_fail(e, FLOPE_EINVAL, "flope_tf_attention: buffer not aligned to its element type");
  TF_HIP(e, hipSetDevice(e->device));
  return tf_by_dtype(e, [&](auto tag) {
    return launch_attention<typename decltype(tag)::type>(e, qkv_dev, out_dev, batch, seq_len, nullptr, (hipStream_t)stream);
  });
}

// the loaded linear a name of flope_tf_linear / flope_tf_linear_plan means, or nullptr
static const TfLinear* tf_find_linear(const flope_tf_encoder* e, const std::string& nm) {
  if (nm == "embedding") return &e->emb;
  if (nm == "out_layer") return &e->outl;
  if (nm.compare(0, 7, "layers.") != 0) return nullptr;
  const size_t dot = nm.find('.', 7);
  const std::string idx = dot == std::string::npos ? "" : nm.substr(7, dot - 7), op = dot == std::string::npos ? "" : nm.substr(dot + 1);
  if (idx.empty() || idx.size() > 6 || idx.find_first_not_of("0123456789") != std::string::npos || std::stoi(idx) >= e->nl) return nullptr;
  const TfLayer& ly = e->layers[std::stoi(idx)];
  return op == "in_proj" ? &ly.in_proj : op == "out_proj" ? &ly.out_proj : op == "linear1" ? &ly.lin1 : op == "linear2" ? &ly.lin2 : nullptr;
}

// flope_tf_linear and flope_tf_linear_act: act is 0 or FLOPE_TF_ACT_*
static int tf_linear_entry(flope_tf_handle e, const char* name, const void* x_dev, int x_f32, const void* res_dev, void* y_dev, int y_f32, int rows,
                           int act, void* stream) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_linear: NULL handle");
  if (!e->loaded) return tf_fail(e, FLOPE_ESTATE, "flope_tf_linear: weights not loaded");
  if (!name || !x_dev || !y_dev) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear: NULL argument");
  const std::string nm(name);
  const TfLinear* l = tf_find_linear(e, nm);
  if (!l) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear: unknown linear " + nm + " (embedding, out_layer, layers.<i>.in_proj / out_proj / linear1 / linear2)");
  if (rows < 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear: non-positive rows");
  if (rows > e->max_tokens) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear: rows exceeds max_tokens given to flope_tf_create");
  if (act < 0 || act > FLOPE_TF_ACT_GELU) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_act: act is 0 (none), 1 (ReLU) or 2 (GELU)");
  if (act == FLOPE_TF_ACT_GELU && res_dev) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_act: GELU with a residual has no kernel");
  const uintptr_t bits = (uintptr_t)x_dev | (uintptr_t)res_dev | (uintptr_t)y_dev;
  if (e->dtype == FLOPE_DT_F32) {
    if (bits & 3) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear: buffer not aligned to its element type");
  } else {
    if (bits & 15) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear: 16-bit handles take x, res and y 16-byte aligned");
    // tf_cast_pad writes rows of roundup(K, 64) into the handle's input copy, which is as wide as the embedding's
    if (x_f32 && l != &e->emb && l->packed && !y_f32 && !e->opt_generic)
      return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear: a float32 input to the MFMA linear is the network input (embedding only)");
    // ... and tf_gemm_mfma reads rows of roundup(K, 64): a 16-bit x_dev [rows, K] with K % 64 != 0 would be read past its rows
    if (!x_f32 && l->packed && l->K != l->Kp && !y_f32 && !e->opt_generic)
      return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear: the MFMA linear with K % 64 != 0 takes its input as float32 (x_f32), which is zero-padded to roundup(K, 64) columns");
  }
  TF_HIP(e, hipSetDevice(e->device));
  return tf_by_dtype(e, [&](auto tag) {
    using T = typename decltype(tag)::type;
    constexpr bool f32 = std::is_same<T, float>::value;                // a float32 handle's buffers are float32 whatever the flags say
    return launch_linear<T>(e, *l, x_dev, f32 || x_f32 ? 1 : 0, res_dev, y_dev, f32 || y_f32 ? 1 : 0, rows, act, (hipStream_t)stream);
  });
}

extern "C" int flope_tf_linear(flope_tf_handle e, const char* name, const void* x_dev, int x_f32, const void* res_dev, void* y_dev, int y_f32, int rows,
                               int relu, void* stream) {
  return tf_linear_entry(e, name, x_dev, x_f32, res_dev, y_dev, y_f32, rows, relu ? FLOPE_TF_ACT_RELU : 0, stream);
}

extern "C" int flope_tf_linear_act(flope_tf_handle e, const char* name, const void* x_dev, int x_f32, const void* res_dev, void* y_dev, int y_f32, int rows,
                                   int act, void* stream) {
  return tf_linear_entry(e, name, x_dev, x_f32, res_dev, y_dev, y_f32, rows, act, stream);
}

// The id flope_tf_linear returns for this linear at this row count in the form the forward runs it -- embedding: float32 in; out_layer:
// float32 out; out_proj and linear2: with a residual; linear1: with the handle's activation -- under the handle's current options; launches nothing.
extern "C" int flope_tf_linear_plan(flope_tf_handle e, const char* name, int rows) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_linear_plan: NULL handle");
  if (!e->loaded) return tf_fail(e, FLOPE_ESTATE, "flope_tf_linear_plan: weights not loaded");
  if (!name) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_plan: NULL argument");
  const std::string nm(name);
  const TfLinear* l = tf_find_linear(e, nm);
  if (!l) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_plan: unknown linear " + nm + " (embedding, out_layer, layers.<i>.in_proj / out_proj / linear1 / linear2)");
  if (rows < 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_plan: non-positive rows");
  if (rows > e->max_tokens) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_plan: rows exceeds max_tokens given to flope_tf_create");
  const bool res = nm.size() > 9 && (nm.compare(nm.size() - 9, 9, ".out_proj") == 0 || nm.compare(nm.size() - 8, 8, ".linear2") == 0);
  const int act = nm.size() > 8 && nm.compare(nm.size() - 8, 8, ".linear1") == 0 ? e->arch.act : 0;      // linear1 under the handle's activation
  void* const any = (void*)(uintptr_t)16;          // an aligned non-NULL pointer: plan mode looks at NULL and alignment only
  return tf_by_dtype(e, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return launch_linear<T>(e, *l, any, l == &e->emb ? 1 : 0, res ? any : nullptr, any, l == &e->outl ? 1 : 0, rows, act, nullptr, true);
  });
}

// the checks flope_tf_linear_ln and flope_tf_linear_ln_plan share; *l: the linear
static int tf_check_linear_ln(flope_tf_encoder* e, const char* who, const char* name, int rows, const TfLinear** l) {
  const std::string w(who);
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, w + ": NULL handle");
  if (!e->loaded) return tf_fail(e, FLOPE_ESTATE, w + ": weights not loaded");
  if (!name) return tf_fail(e, FLOPE_EINVAL, w + ": NULL argument");
  if (!(*l = tf_find_linear(e, name))) return tf_fail(e, FLOPE_EINVAL, w + ": unknown linear " + name + " (embedding, out_layer, layers.<i>.in_proj / out_proj / linear1 / linear2)");
  if (rows < 1) return tf_fail(e, FLOPE_EINVAL, w + ": non-positive rows");
  if (rows > e->max_tokens) return tf_fail(e, FLOPE_EINVAL, w + ": rows exceeds max_tokens given to flope_tf_create");
  return 0;
}

// flope_tf_linear_ln and flope_tf_linear_ln_act: act is 0 or FLOPE_TF_ACT_*
static int tf_linear_ln_entry(flope_tf_handle e, const char* name, const void* x_dev, const float* gamma_dev, const float* beta_dev, void* normed_dev,
                              void* y_dev, int rows, int act, void* stream) {
  const TfLinear* l = nullptr;
  if (int rc = tf_check_linear_ln(e, "flope_tf_linear_ln", name, rows, &l)) return rc;
  if (act < 0 || act > FLOPE_TF_ACT_GELU) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_ln_act: act is 0 (none), 1 (ReLU) or 2 (GELU)");
  if (!x_dev || !gamma_dev || !beta_dev || !normed_dev || !y_dev) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_ln: NULL argument");
  if (((uintptr_t)x_dev | (uintptr_t)normed_dev | (uintptr_t)y_dev) & 15) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_ln: x, normed and y are 16-byte aligned");
  if (((uintptr_t)gamma_dev | (uintptr_t)beta_dev) & 15) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_ln: gamma and beta are 16-byte aligned");
  const bool ok = tf_by_dtype(e, [&](auto tag) { return (int)tf_linear_ln_ok<typename decltype(tag)::type>(e, *l, rows); }) != 0;
  if (!ok) return tf_fail(e, FLOPE_EINVAL, std::string("flope_tf_linear_ln: no LayerNorm form of ") + name + " at " + std::to_string(rows) +
                                               " rows under the handle's options (16-bit handle, options skinny and skinny_ln at 1, generic at 0, 1 .. 32 rows, a packed linear of K = model_dim, model_dim % 64 == 0, model_dim <= 512)");
  // the launch reads the 16 MT rows of x while other waves write those rows of normed and y
  const uintptr_t rb = (uintptr_t)16 * flope_tf_plan::tf_skinny_mt(rows) * e->esz;
  const uintptr_t x0 = (uintptr_t)x_dev, x1 = x0 + rb * e->d, h0 = (uintptr_t)normed_dev, h1 = h0 + rb * e->d, y0 = (uintptr_t)y_dev, y1 = y0 + rb * l->N;
  if ((x0 < h1 && h0 < x1) || (x0 < y1 && y0 < x1) || (h0 < y1 && y0 < h1)) return tf_fail(e, FLOPE_EINVAL, "flope_tf_linear_ln: x, normed and y must not overlap");
  TF_HIP(e, hipSetDevice(e->device));
  return tf_by_dtype(e, [&](auto tag) {
    return launch_linear_ln<typename decltype(tag)::type>(e, *l, x_dev, gamma_dev, beta_dev, normed_dev, y_dev, rows, act, (hipStream_t)stream);
  });
}

extern "C" int flope_tf_linear_ln(flope_tf_handle e, const char* name, const void* x_dev, const float* gamma_dev, const float* beta_dev, void* normed_dev,
                                  void* y_dev, int rows, int relu, void* stream) {
  return tf_linear_ln_entry(e, name, x_dev, gamma_dev, beta_dev, normed_dev, y_dev, rows, relu ? FLOPE_TF_ACT_RELU : 0, stream);
}

extern "C" int flope_tf_linear_ln_act(flope_tf_handle e, const char* name, const void* x_dev, const float* gamma_dev, const float* beta_dev, void* normed_dev,
                                      void* y_dev, int rows, int act, void* stream) {
  return tf_linear_ln_entry(e, name, x_dev, gamma_dev, beta_dev, normed_dev, y_dev, rows, act, stream);
}

// FLOPE_TF_LIN_SKINNY_LN where flope_tf_linear_ln would launch, else the id of the separate form's linear (no residual; linear1 with
// the handle's activation); launches nothing
extern "C" int flope_tf_linear_ln_plan(flope_tf_handle e, const char* name, int rows) {
  const TfLinear* l = nullptr;
  if (int rc = tf_check_linear_ln(e, "flope_tf_linear_ln_plan", name, rows, &l)) return rc;
  const std::string nm(name);
  const int act = nm.size() > 8 && nm.compare(nm.size() - 8, 8, ".linear1") == 0 ? e->arch.act : 0;
  void* const any = (void*)(uintptr_t)16;
  return tf_by_dtype(e, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (tf_linear_ln_ok<T>(e, *l, rows)) return (int)FLOPE_TF_LIN_SKINNY_LN;
    return launch_linear<T>(e, *l, any, l == &e->emb ? 1 : 0, nullptr, any, l == &e->outl ? 1 : 0, rows, act, nullptr, true);
  });
}

extern "C" int flope_tf_last_ln(flope_tf_handle e, int* launched, int* folded) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_last_ln: NULL handle");
  if (launched) *launched = e->last_ln_launched;
  if (folded) *folded = e->last_ln_folded;
  return FLOPE_OK;
}

extern "C" int flope_tf_layernorm(flope_tf_handle e, const void* in_dev, void* out_dev, const float* gamma_dev, const float* beta_dev, int rows, void* stream) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_layernorm: NULL handle");
  if (!in_dev || !out_dev || !gamma_dev || !beta_dev) return tf_fail(e, FLOPE_EINVAL, "flope_tf_layernorm: NULL buffer");
  if (rows < 1) return tf_fail(e, FLOPE_EINVAL, "flope_tf_layernorm: non-positive rows");
  if (rows > e->max_tokens) return tf_fail(e, FLOPE_EINVAL, "flope_tf_layernorm: rows exceeds max_tokens given to flope_tf_create");
  if (((uintptr_t)gamma_dev | (uintptr_t)beta_dev) & 3) return tf_fail(e, FLOPE_EINVAL, "flope_tf_layernorm: gamma / beta not aligned to float");
  const uintptr_t bits = (uintptr_t)in_dev | (uintptr_t)out_dev;
  if (e->dtype == FLOPE_DT_F32 ? bits & 3 : bits & 15)
    return tf_fail(e, FLOPE_EINVAL, e->dtype == FLOPE_DT_F32 ? "flope_tf_layernorm: buffer not aligned to its element type"
                                                             : "flope_tf_layernorm: 16-bit handles take in and out 16-byte aligned");
  TF_HIP(e, hipSetDevice(e->device));
  return tf_by_dtype(e, [&](auto tag) {
    return launch_layernorm<typename decltype(tag)::type>(e, in_dev, out_dev, gamma_dev, beta_dev, rows, (hipStream_t)stream);
  });
}

extern "C" int flope_tf_forward_varlen(flope_tf_handle e, const float* x_dev, int batch, int seq_len, const int* lengths_host, float* y_dev, void* stream) {
  int rc;
  if ((rc = tf_check_forward_varlen(e, "flope_tf_forward_varlen", batch, seq_len, x_dev && y_dev))) return rc;
  if ((rc = tf_check_window(e, "flope_tf_forward_varlen"))) return rc;
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  TfRagged rg;
  if ((rc = tf_plan_ragged(e, "flope_tf_forward_varlen", lengths_host, batch, seq_len, st, &rg))) return rc;
  return tf_forward(e, x_dev, batch, seq_len, y_dev, st, &rg);
}

extern "C" int flope_tf_forward_plan(flope_tf_handle e, int batch, int seq_len, const int* lengths_host) {
  int rc;
  if (!lengths_host) {
    bool empty;
    if ((rc = tf_check_forward(e, "flope_tf_forward_plan", batch, seq_len, true, &empty))) return rc;
    if ((rc = tf_check_window(e, "flope_tf_forward_plan"))) return rc;
    return !empty && tf_fused_pick(e, seq_len) ? FLOPE_TF_FWD_FUSED : FLOPE_TF_FWD_LAUNCHES;
  }
  if ((rc = tf_check_forward_varlen(e, "flope_tf_forward_plan", batch, seq_len, true)) || (rc = tf_check_window(e, "flope_tf_forward_plan"))) return rc;
  std::vector<int> off((size_t)(batch > 0 ? batch : 0) + 1);         // the handle's own table stays as the last forward left it
  TfRagged rg;
  if ((rc = tf_check_ragged(e, "flope_tf_forward_plan", lengths_host, batch, seq_len, off.data(), &rg))) return rc;
  return tf_fused_pick(e, rg.max_len) ? FLOPE_TF_FWD_FUSED : FLOPE_TF_FWD_LAUNCHES;
}

extern "C" int flope_tf_last_forward(flope_tf_handle e) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_last_forward: NULL handle");
  return e->last_fwd;
}

extern "C" int flope_tf_attention_varlen(flope_tf_handle e, const void* qkv_dev, int batch, const int* lengths_host, void* out_dev, void* stream) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_attention_varlen: NULL handle");
  if (int rc = tf_check_window(e, "flope_tf_attention_varlen")) return rc;
  if (!qkv_dev || !out_dev) return tf_fail(e, FLOPE_EINVAL, "flope_tf_attention_varlen: NULL buffer");
  if (((uintptr_t)qkv_dev | (uintptr_t)out_dev) & (uintptr_t)(e->esz - 1))
    return tf_fail(e, FLOPE_EINVAL, "flope_tf_attention_varlen: buffer not aligned to its element type");
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  TfRagged rg;
  int rc;
  if ((rc = tf_plan_ragged(e, "flope_tf_attention_varlen", lengths_host, batch, e->max_tokens, st, &rg))) return rc;   // no padded length here: a length is bounded by max_tokens
  return tf_by_dtype(e, [&](auto tag) {
    return launch_attention<typename decltype(tag)::type>(e, qkv_dev, out_dev, batch, rg.max_len, e->vl_off, st);
  });
}

namespace {
// (query, key) pairs of one sequence of len tokens under the handle's options: len^2, causal len (len + 1) / 2, causal with window W
// sum_t min(t + 1, W) = W (W + 1) / 2 + (len - W) W for W < len
double tf_attn_pairs(const flope_tf_encoder* e, double len) {
  if (!e->opt_causal) return len * len;
  const double W = e->opt_window;
  if (W > 0 && W < len) return W * (W + 1.0) / 2.0 + (len - W) * W;
  return len * (len + 1.0) / 2.0;
}
}  // namespace

// algorithmic FLOPs of one forward (2*MAC: linears + QK^T + PV); option causal: a query of a sequence of len tokens meets
// (len + 1) / 2 keys on average, d len (len + 1) MACs per sequence and layer instead of 2 d len^2; with option window W query t
// meets min(t + 1, W) keys
extern "C" double flope_tf_forward_flops(flope_tf_handle e, int batch, int seq_len) {
  if (!e) return 0.0;
  const double M = (double)batch * seq_len, d = e->d;
  double mac = M * e->in_dim * d + M * d * e->out_dim;
  mac += e->nl * (M * d * 3 * d + M * d * d + 2.0 * M * d * e->ff + 2.0 * batch * tf_attn_pairs(e, seq_len) * d);
  return 2.0 * mac;
}

// algorithmic FLOPs of one ragged forward: the linears on T = sum lengths tokens, attention on sum lengths^2 (option causal: on
// sum lengths (lengths + 1) / 2, with option window on sum_t min(t + 1, W) per sequence); 0 for an invalid batch
extern "C" double flope_tf_forward_flops_varlen(flope_tf_handle e, int batch, const int* lengths_host) {
  if (!e || batch < 1 || !lengths_host) return 0.0;
  double M = 0.0, sq = 0.0;
  for (int b = 0; b < batch; ++b) {
    if (lengths_host[b] < 1) return 0.0;
    M += lengths_host[b];
    sq += tf_attn_pairs(e, lengths_host[b]);
  }
  const double d = e->d;
  double mac = M * e->in_dim * d + M * d * e->out_dim;
  mac += e->nl * (M * d * 3 * d + M * d * d + 2.0 * M * d * e->ff + 2.0 * sq * d);
  return 2.0 * mac;
}

// ---- attention under a compiled mask ------------------------------------------------------------------------------------
namespace {

// The masked attention launch, tf_attn_pick_masked's answer: tf_attn_masked for every dtype and head_dim, launched as the generic kernel
// always is plus the mask rows in LDS (tf_mask_launch), unless option mask_mfma sends a 16-bit launch to tf_attn_tiled_masked, launched
// as tf_attn_tiled is (tf_mask16_launch).  off == nullptr: qkv [B][L][3 d], L == m->L; otherwise the packed rows of a ragged batch, L
// its longest length.  Returns the kernel's FLOPE_TF_ATTN_* id, or < 0.
// A handle that carries a bias (m->planes > 0) takes tf_attn_masked's BIASED instantiation on every dtype, launched by
// tf_mask_launch as the unbiased one is, unless option bias_mfma (not mask_mfma) sends a 16-bit launch to tf_attn_tiled_masked's
// BIASED instantiation (tf_attn_pick_biased), launched by tf_mask16_launch.
int tf_masked_pick(const flope_tf_encoder* e, const flope_tf_mask* m, const void* qkv, const void* att) {
  if (m->planes) return flope_tf_plan::tf_attn_pick_biased(e->dtype, e->d / e->H, e->opt_generic, e->opt_bias_mfma, !(((uintptr_t)qkv | (uintptr_t)att) & 15));
  return flope_tf_plan::tf_attn_pick_masked(e->dtype, e->d / e->H, e->opt_generic, e->opt_mask_mfma, !(((uintptr_t)qkv | (uintptr_t)att) & 15));
}
template <typename T>
int launch_attention_masked(flope_tf_encoder* e, const flope_tf_mask* m, const void* qkv, void* att, int B, int L, const int* off, hipStream_t st) {
  const int dh = e->d / e->H, pick = tf_masked_pick(e, m, qkv, att);
  const bool tiled = pick == FLOPE_TF_ATTN_MASKED16 || pick == FLOPE_TF_ATTN_BIASED16;
  const flope_tf_plan::TfAttnLaunch l = tiled ? flope_tf_plan::tf_mask16_launch(dh, B, e->H, L) : flope_tf_plan::tf_mask_launch(dh, B, e->H, L, m->L);
  const dim3 grid(l.grid_x, l.grid_y), block(l.block);
  auto launch = [&](auto varlen, auto biased) {
    constexpr bool VL = decltype(varlen)::value, BI = decltype(biased)::value;
    if constexpr (!std::is_same<T, float>::value) {
      if (tiled) {
        const float scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
        tf_by_hd32(dh, [&](auto hd32) {
          if constexpr (BI)
            hipLaunchKernelGGL((tf_attn_tiled_masked<T, decltype(hd32)::value, VL, true, const float*, int, int>), grid, block, l.lds, st, (const T*)qkv, (T*)att, L,
                               e->d, e->H, scale_log2e, off, flope_tf_plan::tf_mask_words(m->L), m->bits_dev(), m->start_dev(), m->tiles_dev(), m->bias_dev(),
                               m->planes, m->L);
          else
            hipLaunchKernelGGL((tf_attn_tiled_masked<T, decltype(hd32)::value, VL>), grid, block, l.lds, st, (const T*)qkv, (T*)att, L, e->d, e->H, scale_log2e, off,
                               flope_tf_plan::tf_mask_words(m->L), m->bits_dev(), m->start_dev(), m->tiles_dev());
        });
        return;
      }
    }
    hipLaunchKernelGGL((tf_attn_masked<T, VL, BI>), grid, block, l.lds, st, (const T*)qkv, (T*)att, L, e->d, e->H, m->L, m->bits_dev(), m->first_dev(), m->last_dev(), off,
                       BI ? m->bias_dev() : nullptr, m->planes);
  };
  auto by_varlen = [&](auto biased) {
    if (off) launch(std::true_type{}, biased); else launch(std::false_type{}, biased);
  };
  if (m->planes) by_varlen(std::true_type{}); else by_varlen(std::false_type{});
  TF_HIP(e, hipGetLastError());
  return pick;
}

// The checks every masked call starts with, before anything is enqueued.  lengths == NULL: a fixed-length batch of `batch` sequences of
// seq_len tokens.  Otherwise the ragged batch is planned into off_host (batch + 1 ints) and *rg, and every length n is held against
// the mask's n x n corner.
int tf_masked_check(flope_tf_encoder* e, const std::string& who, const flope_tf_mask* m, int batch, int seq_len, const int* lengths, int* off_host,
                    TfRagged* rg, const void* qkv, const void* att) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (!m) return tf_fail(e, FLOPE_EINVAL, who + ": NULL mask");
  if (!m->e) return tf_fail(e, FLOPE_ESTATE, who + ": the encoder handle of this mask has been destroyed");
  if (m->e != e) return tf_fail(e, FLOPE_EINVAL, who + ": the mask was created on another handle");
  if (batch < 1) return tf_fail(e, FLOPE_EINVAL, who + ": batch must be positive");
  if (seq_len != m->L)
    return tf_fail(e, FLOPE_EINVAL, who + ": seq_len = " + std::to_string(seq_len) + " differs from the mask's seq_len = " + std::to_string(m->L));
  int max_len = seq_len;
  if (!lengths) {
    if ((long long)batch * seq_len > e->max_tokens) return tf_fail(e, FLOPE_EINVAL, who + ": batch*seq_len exceeds max_tokens given to flope_tf_create");
  } else {
    if (int rc = tf_check_ragged(e, who.c_str(), lengths, batch, seq_len, off_host, rg)) return rc;
    for (int b = 0; b < batch; ++b) {
      const int row = flope_tf_plan::tf_mask_length_row(m->first.data(), m->L, lengths[b]);
      if (row >= 0)
        return tf_fail(e, FLOPE_EINVAL, who + ": lengths[" + std::to_string(b) + "] = " + std::to_string(lengths[b]) + ": b = " + std::to_string(b) + ", row " +
                                            std::to_string(row) + " has no allowed key below " + std::to_string(lengths[b]) + " (a softmax over nothing)");
    }
    max_len = rg->max_len;
  }
  const int pick = tf_masked_pick(e, m, qkv, att);
  if (pick != FLOPE_TF_ATTN_MASKED16 && pick != FLOPE_TF_ATTN_BIASED16 &&      // tf_attn_tiled_masked keeps no row in LDS
      flope_tf_plan::tf_mask_launch(e->d / e->H, batch, e->H, max_len, m->L).lds > flope_tf_plan::kTfAttnLds)
    return tf_fail(e, FLOPE_EINVAL, who + ": seq_len too long for the score rows of one workgroup");
  return 0;
}

// What flope_tf_mask_create and flope_tf_bias_create end in once m->bits are final (m->L and m->planes set, every validator passed): the
// first / last tables, the pair count and the tile map on the host, one allocation laid out by tf_mask_dev_* / tf_bias_dev_*
// (tf_attn_mask.h) with bits | first | last and behind them the tile map, or the bias planes and then the tile map (every bias: option
// bias_mfma may be flipped between forwards), and the mask on the handle's list.  Owns m: a failure frees it.
int tf_mask_finish(flope_tf_encoder* e, const std::string& who, flope_tf_mask* m, const float* bias_host, flope_tf_mask_handle* out) {
  using namespace flope_tf_plan;
  const int L = m->L, planes = m->planes;
  m->first.resize(L);
  m->last.resize(L);
  tf_mask_first_last(m->bits.data(), L, m->first.data(), m->last.data());
  m->pairs = tf_mask_pairs(m->bits.data(), L);
  m->start.resize((size_t)tf_mask_query_blocks(L) + 1);
  m->tiles.resize((size_t)tf_mask_tiles_build(m->bits.data(), L, m->start.data(), nullptr));
  tf_mask_tiles_build(m->bits.data(), L, m->start.data(), m->tiles.data());
  const size_t nb = m->bits.size() * sizeof(uint32_t), nt = (size_t)L * sizeof(int);
  const size_t all = planes ? tf_bias_dev_bytes_tiled(L, planes, (long long)m->tiles.size()) : tf_mask_dev_bytes(L, (long long)m->tiles.size());
  auto fin = [&](const std::string& what) { hipFree(m->dev); delete m; return tf_fail(e, FLOPE_EHIP, who + ": " + what); };
  auto put = [&](size_t at, const void* src, size_t bytes) { return hipMemcpy((char*)m->dev + at, src, bytes, hipMemcpyHostToDevice) == hipSuccess; };
  if (hipSetDevice(e->device) != hipSuccess) return fin("hipSetDevice failed");
  if (hipMalloc(&m->dev, all) != hipSuccess) {
    m->dev = nullptr;
    return fin("hipMalloc of " + std::to_string(all) + " bytes failed" +
               (planes ? " (" + std::to_string(planes) + " float32 planes of " + std::to_string((size_t)L * L * 4) + " bytes)" : std::string()));
  }
  if (!put(0, m->bits.data(), nb) || !put(nb, m->first.data(), nt) || !put(nb + nt, m->last.data(), nt) ||
      (planes && !put(tf_bias_dev_bias_at(L), bias_host, (size_t)planes * L * L * sizeof(float))) ||
      !put(planes ? tf_bias_dev_start_at(L, planes) : tf_mask_dev_start_at(L), m->start.data(), m->start.size() * sizeof(int)) ||
      !put(planes ? tf_bias_dev_tiles_at(L, planes) : tf_mask_dev_tiles_at(L), m->tiles.data(), m->tiles.size() * sizeof(TfMaskTile)))
    return fin("hipMemcpy failed");
  m->e = e;
  e->masks.push_back(m);
  *out = m;
  return FLOPE_OK;
}

}  // namespace

extern "C" int flope_tf_mask_create(flope_tf_handle e, int seq_len, const uint32_t* allow_bits_host, flope_tf_mask_handle* out) {
  using namespace flope_tf_plan;
  const std::string who = "flope_tf_mask_create";
  if (out) *out = nullptr;
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (!out || !allow_bits_host) return tf_fail(e, FLOPE_EINVAL, who + ": NULL argument");
  if (seq_len < 1 || seq_len > e->max_tokens)
    return tf_fail(e, FLOPE_EINVAL, who + ": seq_len = " + std::to_string(seq_len) + " is outside 1 .. max_tokens = " + std::to_string(e->max_tokens));
  int row = -1;
  const int col = tf_mask_padding_bit(allow_bits_host, seq_len, &row);
  if (col >= 0)
    return tf_fail(e, FLOPE_EINVAL, who + ": padding bit set in row " + std::to_string(row) + ", column " + std::to_string(col) + " (columns >= seq_len must be zero)");
  row = tf_mask_empty_row(allow_bits_host, seq_len);
  if (row >= 0) return tf_fail(e, FLOPE_EINVAL, who + ": row " + std::to_string(row) + " has no allowed key (a softmax over nothing; the reference returns NaN there)");
  flope_tf_mask* m = new flope_tf_mask();
  m->L = seq_len;
  m->bits.assign(allow_bits_host, allow_bits_host + (size_t)seq_len * tf_mask_words(seq_len));
  return tf_mask_finish(e, who, m, nullptr, out);
}

// A compiled additive bias: the mask of its -inf entries plus a float32 value per allowed pair, on the same handle type
extern "C" int flope_tf_bias_create(flope_tf_handle e, int seq_len, int planes, const float* bias_host, flope_tf_mask_handle* out) {
  using namespace flope_tf_plan;
  const std::string who = "flope_tf_bias_create";
  if (out) *out = nullptr;
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (!out || !bias_host) return tf_fail(e, FLOPE_EINVAL, who + ": NULL argument");
  if (seq_len < 1 || seq_len > e->max_tokens)
    return tf_fail(e, FLOPE_EINVAL, who + ": seq_len = " + std::to_string(seq_len) + " is outside 1 .. max_tokens = " + std::to_string(e->max_tokens));
  if (planes != 1 && planes != e->H)
    return tf_fail(e, FLOPE_EINVAL, who + ": planes = " + std::to_string(planes) + " is neither 1 nor num_heads = " + std::to_string(e->H));
  int pl = -1, row = -1, col = -1;
  auto at = [&] { return "(plane " + std::to_string(pl) + ", row " + std::to_string(row) + ", col " + std::to_string(col) + ")"; };
  if (tf_bias_nonfinite(bias_host, seq_len, planes, &pl, &row, &col))
    return tf_fail(e, FLOPE_EINVAL, who + ": the entry at " + at() + " is +inf or NaN (a bias entry is finite, or -inf for a masked pair)");
  if (tf_bias_plane_differs(bias_host, seq_len, planes, &pl, &row, &col))
    return tf_fail(e, FLOPE_EINVAL, who + ": the entry at " + at() + " is masked in one of plane 0 and plane " + std::to_string(pl) +
                                        " and allowed in the other: the allowed set is one for all heads (write a per-head difference as a large negative finite value)");
  flope_tf_mask* m = new flope_tf_mask();
  m->L = seq_len;
  m->planes = planes;
  m->bits.resize((size_t)seq_len * tf_mask_words(seq_len));
  tf_bias_pack(bias_host, seq_len, m->bits.data());
  row = tf_mask_empty_row(m->bits.data(), seq_len);
  if (row >= 0) {
    delete m;
    return tf_fail(e, FLOPE_EINVAL, who + ": row " + std::to_string(row) + " has no allowed key (a softmax over nothing; the reference returns NaN there)");
  }
  return tf_mask_finish(e, who, m, bias_host, out);
}

extern "C" int flope_tf_mask_bias_planes(flope_tf_mask_handle m) {
  if (!m) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_mask_bias_planes: NULL mask");
  if (!m->e) return tf_fail(nullptr, FLOPE_ESTATE, "flope_tf_mask_bias_planes: the encoder handle of this mask has been destroyed");
  return m->planes;
}

extern "C" int flope_tf_mask_destroy(flope_tf_mask_handle m) {
  if (!m) return FLOPE_OK;
  if (flope_tf_encoder* e = m->e) {                // after flope_tf_destroy the device memory is gone already
    hipSetDevice(e->device);
    hipFree(m->dev);
    for (size_t i = 0; i < e->masks.size(); ++i)
      if (e->masks[i] == m) { e->masks.erase(e->masks.begin() + (long)i); break; }
  }
  delete m;
  return FLOPE_OK;
}

extern "C" int flope_tf_mask_info(flope_tf_mask_handle m, int* seq_len, long long* allowed_pairs) {
  if (!m) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_mask_info: NULL mask");
  if (!m->e) return tf_fail(nullptr, FLOPE_ESTATE, "flope_tf_mask_info: the encoder handle of this mask has been destroyed");
  if (seq_len) *seq_len = m->L;
  if (allowed_pairs) *allowed_pairs = m->pairs;
  return FLOPE_OK;
}

extern "C" int flope_tf_mask_tiles(flope_tf_mask_handle m, int* query_blocks, long long* blocks_listed, long long* steps_none, long long* steps_some,
                                   long long* steps_all) {
  if (!m) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_mask_tiles: NULL mask");
  if (!m->e) return tf_fail(nullptr, FLOPE_ESTATE, "flope_tf_mask_tiles: the encoder handle of this mask has been destroyed");
  const flope_tf_plan::TfMaskTileStats st = flope_tf_plan::tf_mask_tile_stats(m->L, m->start.data(), m->tiles.data());
  if (query_blocks) *query_blocks = st.query_blocks;
  if (blocks_listed) *blocks_listed = st.blocks_listed;
  if (steps_none) *steps_none = st.steps_none;
  if (steps_some) *steps_some = st.steps_some;
  if (steps_all) *steps_all = st.steps_all;
  return FLOPE_OK;
}

extern "C" int flope_tf_forward_masked(flope_tf_handle e, const float* x_dev, int batch, int seq_len, const int* lengths_host, flope_tf_mask_handle m,
                                       float* y_dev, void* stream) {
  const std::string who = "flope_tf_forward_masked";
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (!x_dev || !y_dev) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  TfRagged rg;
  int rc;
  if ((rc = tf_masked_check(e, who, m, batch, seq_len, lengths_host, e->vl_host.data(), &rg, e->qkv, e->att))) return rc;
  if (!e->loaded) return tf_fail(e, FLOPE_ESTATE, who + ": weights not loaded");
  if (lengths_host && (rc = tf_check_forward_varlen(e, who, batch, seq_len, true))) return rc;
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  if (lengths_host && (rc = tf_upload_ragged(e, batch, st))) return rc;
  e->last_fwd = FLOPE_TF_FWD_LAUNCHES;              // never the single launch
  const TfRagged* rgp = lengths_host ? &rg : nullptr;
  return tf_by_dtype(e, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return run_forward_with<T>(e, x_dev, batch, seq_len, y_dev, st, rgp, [&](int) {
      return e->last_masked_attn = launch_attention_masked<T>(e, m, e->qkv, e->att, batch, rgp ? rg.max_len : seq_len, rgp ? e->vl_off : nullptr, st);
    });
  });
}

extern "C" int flope_tf_last_forward_masked(flope_tf_handle e) {
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, "flope_tf_last_forward_masked: NULL handle");
  return e->last_masked_attn;
}

extern "C" int flope_tf_attention_masked(flope_tf_handle e, const void* qkv_dev, int batch, int seq_len, const int* lengths_host, flope_tf_mask_handle m,
                                         void* out_dev, void* stream) {
  const std::string who = "flope_tf_attention_masked";
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (!qkv_dev || !out_dev) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  if (((uintptr_t)qkv_dev | (uintptr_t)out_dev) & (uintptr_t)(e->esz - 1)) return tf_fail(e, FLOPE_EINVAL, who + ": buffer not aligned to its element type");
  TfRagged rg;
  int rc;
  if ((rc = tf_masked_check(e, who, m, batch, seq_len, lengths_host, e->vl_host.data(), &rg, qkv_dev, out_dev))) return rc;
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  if (lengths_host && (rc = tf_upload_ragged(e, batch, st))) return rc;
  return tf_by_dtype(e, [&](auto tag) {
    return launch_attention_masked<typename decltype(tag)::type>(e, m, qkv_dev, out_dev, batch, lengths_host ? rg.max_len : seq_len,
                                                                 lengths_host ? e->vl_off : nullptr, st);
  });
}

// algorithmic FLOPs of one masked forward: the linears on every token, attention on the allowed pairs (lengths: of each length's corner)
extern "C" double flope_tf_forward_flops_masked(flope_tf_handle e, int batch, const int* lengths_host, flope_tf_mask_handle m) {
  if (!e || !m || m->e != e || batch < 1) return 0.0;
  double M = 0.0, pairs = 0.0;
  for (int b = 0; b < batch; ++b) {
    const int n = lengths_host ? lengths_host[b] : m->L;
    if (n < 1 || n > m->L) return 0.0;
    M += n;
    pairs += n == m->L ? (double)m->pairs : (double)flope_tf_plan::tf_mask_pairs_len(m->bits.data(), m->L, n);
  }
  const double d = e->d;
  double mac = M * e->in_dim * d + M * d * e->out_dim;
  mac += e->nl * (M * d * 3 * d + M * d * d + 2.0 * M * d * e->ff + 2.0 * pairs * d);
  return 2.0 * mac;
}

// ---- streaming causal forward ---------------------------------------------------------------------------------------
namespace {

using flope_tf_plan::tf_stream_track;

// the checks every call on a state starts with; *e: its handle
int tf_stream_enter(flope_tf_stream_s* s, const std::string& who, flope_tf_encoder** e) {
  if (!s) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL stream state");
  if (!s->e) return tf_fail(nullptr, FLOPE_ESTATE, who + ": the encoder handle of this stream state has been destroyed");
  *e = s->e;
  return 0;
}
// ... of a call that reads or moves positions on the host: a device-positioned state has none there.  instead: the call to use
int tf_stream_enter_host(flope_tf_stream_s* s, const std::string& who, flope_tf_encoder** e, const char* instead) {
  const int rc = tf_stream_enter(s, who, e);
  if (rc) return rc;
  if (s->max_rows) return tf_fail(*e, FLOPE_ESTATE, who + ": this state keeps its positions on the device (flope_tf_stream_open_device); " + instead);
  return 0;
}
// ... and of a call that needs them there
int tf_stream_enter_device(flope_tf_stream_s* s, const std::string& who, flope_tf_encoder** e) {
  const int rc = tf_stream_enter(s, who, e);
  if (rc) return rc;
  if (!s->max_rows) return tf_fail(*e, FLOPE_ESTATE, who + ": this state keeps its positions on the host; open one with flope_tf_stream_open_device");
  return 0;
}

// the refusals of tf_encoder_stream.h in words; bad: the index they name
int tf_stream_refuse(flope_tf_stream_s* s, const std::string& who, int rc, int bad, int n, const int* rows, const int* lengths, int seq_len) {
  using namespace flope_tf_plan;
  flope_tf_encoder* e = s->e;
  const std::string i = std::to_string(bad);
  switch (rc) {
    case kTfStreamCount:
      return tf_fail(e, FLOPE_EINVAL, who + ": n = " + std::to_string(n) + " is outside 1 .. min(tracks = " + std::to_string(s->tracks) + ", max_tokens = " +
                                          std::to_string(e->max_tokens) + ")" + (rows ? "" : ", or tracks_host is NULL and n is not the state's track count"));
    case kTfStreamRange:
      return tf_fail(e, FLOPE_EINVAL, who + ": tracks[" + i + "] = " + std::to_string(rows[bad]) + " is outside 0 .. " + std::to_string(s->tracks - 1));
    case kTfStreamDuplicate:
      return tf_fail(e, FLOPE_EINVAL, who + ": tracks[" + i + "] = " + std::to_string(rows[bad]) + " names a track an earlier row names (one token per track and call)");
    case kTfStreamFull:
      if (s->window)
        return tf_fail(e, FLOPE_EINVAL, who + ": row " + i + ": track " + std::to_string(tf_stream_track(rows, bad)) + " holds INT_MAX = " + std::to_string(INT_MAX) +
                                            " tokens, the last position an int counts (a windowed state is full only there; reset the track)");
      return tf_fail(e, FLOPE_EINVAL, who + ": row " + i + ": track " + std::to_string(tf_stream_track(rows, bad)) + " already holds capacity = " + std::to_string(s->capacity) +
                                          " tokens (reset it, or open a state with more room)");
    default:
      return tf_fail(e, FLOPE_EINVAL, who + ": lengths[" + i + "] = " + std::to_string(lengths ? lengths[bad] : seq_len) + " exceeds capacity = " + std::to_string(s->capacity));
  }
}

// what the step's and the extend's launches both ask: the head_dim, and whether the row kernels move a head slice as 16-byte vectors
inline int tf_head_dim(const flope_tf_encoder* e) { return e->d / e->H; }
template <typename T> bool tf_row_vec(const flope_tf_encoder* e) { return flope_tf_plan::tf_step_vec_ok(tf_head_dim(e), (int)sizeof(T)); }

// which of FLOPE_TF_STEP_ROW / _SPLIT a step or extend of this state launches now; a state with a distance table: _BIASED, whatever
// the options say
template <typename T> int tf_step_plan(const flope_tf_encoder* e, const flope_tf_stream_s* s) {
  if (s->planes) return FLOPE_TF_STEP_BIASED;
  return e->opt_step_split && flope_tf_plan::tf_step_split_ok(tf_head_dim(e), (int)sizeof(T)) ? FLOPE_TF_STEP_SPLIT : FLOPE_TF_STEP_ROW;
}

// the attention launch of a step: n rows of qkv [n][3 d] against one layer's part of the cache -> att [n][d]; the table is s->tab.
// Returns the kernel's id or < 0
template <typename T>
int launch_step_attn(flope_tf_stream_s* s, const T* qkv, T* cache, T* att, int n, int max_pos, hipStream_t st) {
  flope_tf_encoder* e = s->e;
  const int plan = tf_step_plan<T>(e, s);
  if (plan == FLOPE_TF_STEP_SPLIT) {
    const flope_tf_plan::TfStreamLaunch l = flope_tf_plan::tf_step_split_launch(n, e->H, tf_head_dim(e));
#define TF_SPLIT(WIN_) hipLaunchKernelGGL((tf_attn_step_split<T, WIN_>), dim3(l.grid_x), dim3(l.block), l.lds, st, qkv, cache, att, (const int*)s->tab, n, e->d, \
                                          e->H, s->tracks, s->capacity, s->window)
    if (s->window) TF_SPLIT(true); else TF_SPLIT(false);
#undef TF_SPLIT
  } else {
    const flope_tf_plan::TfStreamLaunch l = flope_tf_plan::tf_step_launch(n, e->H, max_pos);
#define TF_STEP(VEC_, WIN_) hipLaunchKernelGGL((tf_attn_step<T, VEC_, WIN_>), dim3(l.grid_x), dim3(l.block), l.lds, st, qkv, cache, att, \
                                              (const int*)s->tab, n, e->d, e->H, s->tracks, s->capacity, max_pos + 1, s->window)
#define TF_STEPB(VEC_, WIN_) hipLaunchKernelGGL((tf_attn_step<T, VEC_, WIN_, true, const float*, int, int>), dim3(l.grid_x), dim3(l.block), l.lds, st, qkv, cache, \
                                               att, (const int*)s->tab, n, e->d, e->H, s->tracks, s->capacity, max_pos + 1, s->window,                      \
                                               (const float*)s->rel, s->planes, s->rel_d)
    if (plan == FLOPE_TF_STEP_BIASED) {
      if (tf_row_vec<T>(e)) { if (s->window) TF_STEPB(true, true); else TF_STEPB(true, false); }
      else { if (s->window) TF_STEPB(false, true); else TF_STEPB(false, false); }
    } else if (tf_row_vec<T>(e)) { if (s->window) TF_STEP(true, true); else TF_STEP(true, false); }
    else { if (s->window) TF_STEP(false, true); else TF_STEP(false, false); }
#undef TF_STEPB
#undef TF_STEP
  }
  TF_HIP(e, hipGetLastError());
  return plan;
}

// the forward's launch sequence at M = n rows, tf_attn_step (option step_split: tf_attn_step_split) where it has launch_attention.
// max_pos: the call's largest position; a windowed state: its largest visible key count - 1 (tf_stream_check_step_window)
template <typename T>
int run_step(flope_tf_stream_s* s, const float* x, int n, int max_pos, float* y, hipStream_t st) {
  flope_tf_encoder* e = s->e;
  const size_t layer = (size_t)s->tracks * s->capacity * 2 * e->d;
  return run_forward_with<T>(e, x, n, 1, y, st, nullptr, [&](int li) {
    const int rc = launch_step_attn<T>(s, (const T*)e->qkv, (T*)s->cache + (size_t)li * layer, (T*)e->att, n, max_pos, st);
    return rc < 0 ? rc : 0;
  });
}

// the one launch of tf_cache_append: the k | v columns of the n sequences of src_qkv (rows of 3 d; offsets `off`, at most max_len rows
// each) into one layer's part of the cache, at the (track, pos0) of `tab`.  16-byte vectors where a row's columns are whole ones.
template <typename T>
int launch_cache_copy(flope_tf_stream_s* s, const T* src_qkv, T* cache, const int* off, const int* tab, int n, int max_len, hipStream_t st) {
  flope_tf_encoder* e = s->e;
  const bool vec = flope_tf_plan::tf_cache_fill_vec_ok(e->d, (int)sizeof(T));
  const int dv = vec ? e->d / flope_tf_plan::tf_stream_vec((int)sizeof(T)) : e->d;
  const flope_tf_plan::TfStreamLaunch l = flope_tf_plan::tf_cache_append_launch(n, max_len, 2 * dv);
  const size_t total = (size_t)n * max_len * 2 * dv;
#define TF_COPY(V_, WIN_) hipLaunchKernelGGL((tf_cache_append<V_, WIN_>), dim3(l.grid_x), dim3(l.block), 0, st, (const V_*)src_qkv, (V_*)cache, off, tab, max_len, dv, \
                                            s->tracks, s->capacity, total)
  if (vec) { if (s->window) TF_COPY(u32x4, true); else TF_COPY(u32x4, false); }
  else { if (s->window) TF_COPY(T, true); else TF_COPY(T, false); }
#undef TF_COPY
  TF_HIP(e, hipGetLastError());
  return 0;
}

// the causal ragged forward's launch sequence, each layer's k | v rows copied into the cache in front of its attention (a windowed
// state: the last min(len, capacity) rows of a sequence, into the ring).  s->tab: (track, 0) per sequence.
// A state with a distance table has no compiled [L, L] bias to give launch_attention: behind the same copy it launches the biased
// tf_attn_extend with that table of (track, 0) -- at pos0 = 0 no cached key is read and a row is the biased forward's
template <typename T> int launch_extend_attn(flope_tf_stream_s* s, int plan, const T* qkv, const T* cache, T* att, int n, int max_len, int smax, hipStream_t st);
template <typename T>
int run_prefill(flope_tf_stream_s* s, const float* x, int n, int L, const TfRagged& rg, float* y, hipStream_t st) {
  flope_tf_encoder* e = s->e;
  const size_t layer = (size_t)s->tracks * s->capacity * 2 * e->d;
  return run_forward_with<T>(e, x, n, L, y, st, &rg, [&](int li) {
    const int rc = launch_cache_copy<T>(s, (const T*)e->qkv, (T*)s->cache + (size_t)li * layer, (const int*)e->vl_off, (const int*)s->tab, n, rg.max_len, st);
    if (rc) return rc;
    if (s->planes) {
      const int ra = launch_extend_attn<T>(s, FLOPE_TF_EXTEND_BIASED, (const T*)e->qkv, (const T*)s->cache + (size_t)li * layer, (T*)e->att, n, rg.max_len,
                                           flope_tf_plan::tf_extend_keys(0, rg.max_len, s->window), st);
      return ra < 0 ? ra : 0;
    }
    return launch_attention<T>(e, e->qkv, e->att, n, rg.max_len, e->vl_off, st);
  });
}

// the ragged forward's launch sequence over the packed chunks, tf_attn_extend where it has launch_attention and each layer's k | v rows
// appended to the cache BEHIND that attention (on a ring the append takes rows whose keys the chunk's earlier queries still read;
// tf_encoder_stream.h).  smax: the call's largest visible key count (tf_stream_check_extend)
// which of FLOPE_TF_EXTEND_ROW / _SPLIT / _MFMA an extend of this state launches now: option extend_mfma where tf_extend_mfma_ok, in
// front of option step_split.  pos_ok: every chunk of the call stays below kTfExtendMfmaPosMax (a plan without a call: true)
template <typename T> int tf_extend_plan(const flope_tf_encoder* e, const flope_tf_stream_s* s, bool pos_ok = true) {
  if (s->planes) return FLOPE_TF_EXTEND_BIASED;              // a state with a distance table: the options do not reach it
  if (e->opt_extend_mfma && pos_ok && flope_tf_plan::tf_extend_mfma_ok(e->dtype, tf_head_dim(e), e->d)) return FLOPE_TF_EXTEND_MFMA;
  return tf_step_plan<T>(e, s) == FLOPE_TF_STEP_SPLIT ? FLOPE_TF_EXTEND_SPLIT : FLOPE_TF_EXTEND_ROW;
}

// the attention launch of an extend: the packed chunks in qkv [T][3 d] (offsets e->vl_off, table s->tab) against one layer's part of
// the cache -> att [T][d].  plan: tf_extend_plan's answer for the call.  Returns it, or < 0
template <typename T>
int launch_extend_attn(flope_tf_stream_s* s, int plan, const T* qkv, const T* cache, T* att, int n, int max_len, int smax, hipStream_t st) {
  flope_tf_encoder* e = s->e;
  if (plan == FLOPE_TF_EXTEND_MFMA) {
    if constexpr (!std::is_same<T, float>::value) {
      const int dh = tf_head_dim(e);
      const flope_tf_plan::TfExtendLaunch lm = flope_tf_plan::tf_extend_mfma_launch(n, e->H, max_len, dh);
      const float scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
      auto launch = [&](auto hd32, auto win) {
        hipLaunchKernelGGL((tf_attn16_extend<T, decltype(hd32)::value, decltype(win)::value>), dim3(lm.grid_x, lm.grid_y), dim3(lm.block), lm.lds, st, qkv, cache, att,
                           (const int*)s->tab, (const int*)e->vl_off, n, e->d, e->H, s->tracks, s->capacity, scale_log2e, s->window);
      };
      tf_by_hd32(dh, [&](auto hd32) {
        if (s->window) launch(hd32, std::true_type{}); else launch(hd32, std::false_type{});
      });
    } else {
      return tf_fail(e, FLOPE_EINVAL, "tf_attn16_extend has no float32 form");
    }
    TF_HIP(e, hipGetLastError());
    return plan;
  }
  const flope_tf_plan::TfExtendLaunch la = flope_tf_plan::tf_extend_launch(n, e->H, max_len, smax);
  const flope_tf_plan::TfExtendLaunch ls = flope_tf_plan::tf_extend_split_launch(n, e->H, max_len, tf_head_dim(e));
#define TF_EXT(VEC_, WIN_) hipLaunchKernelGGL((tf_attn_extend<T, VEC_, WIN_>), dim3(la.grid_x, la.grid_y), dim3(la.block), la.lds, st, qkv, cache, \
                                             att, (const int*)s->tab, (const int*)e->vl_off, n, e->d, e->H, s->tracks, s->capacity, smax, s->window)
#define TF_EXTB(VEC_, WIN_) hipLaunchKernelGGL((tf_attn_extend<T, VEC_, WIN_, true, const float*, int, int>), dim3(la.grid_x, la.grid_y), dim3(la.block), la.lds, st, \
                                              qkv, cache, att, (const int*)s->tab, (const int*)e->vl_off, n, e->d, e->H, s->tracks, s->capacity, smax, s->window,     \
                                              (const float*)s->rel, s->planes, s->rel_d)
#define TF_EXTS(WIN_) hipLaunchKernelGGL((tf_attn_extend_split<T, WIN_>), dim3(ls.grid_x, ls.grid_y), dim3(ls.block), ls.lds, st, qkv, cache, \
                                        att, (const int*)s->tab, (const int*)e->vl_off, n, e->d, e->H, s->tracks, s->capacity, s->window)
  if (plan == FLOPE_TF_EXTEND_SPLIT) { if (s->window) TF_EXTS(true); else TF_EXTS(false); }   // option step_split: tf_attn_extend_split, the bits of the split steps
  else if (plan == FLOPE_TF_EXTEND_BIASED) {
    if (!s->planes) return tf_fail(e, FLOPE_ESTATE, "tf_attn_extend's biased form needs a state with a distance table");
    if (tf_row_vec<T>(e)) { if (s->window) TF_EXTB(true, true); else TF_EXTB(true, false); }
    else { if (s->window) TF_EXTB(false, true); else TF_EXTB(false, false); }
  } else if (tf_row_vec<T>(e)) { if (s->window) TF_EXT(true, true); else TF_EXT(true, false); }
  else { if (s->window) TF_EXT(false, true); else TF_EXT(false, false); }
#undef TF_EXTB
#undef TF_EXTS
#undef TF_EXT
  TF_HIP(e, hipGetLastError());
  return plan;
}

// whether every chunk of the call whose table is in s->tab_host stays where tf_attn16_extend's int arithmetic holds
inline bool tf_extend_positions_ok(const flope_tf_stream_s* s, int n, const int* lengths) {
  for (int b = 0; b < n; ++b)
    if (!flope_tf_plan::tf_extend_mfma_positions_ok(s->tab_host[(size_t)2 * b + 1], lengths[b])) return false;
  return true;
}

template <typename T>
int run_extend(flope_tf_stream_s* s, const float* x, int n, int L, const TfRagged& rg, const int* lengths, int smax, float* y, hipStream_t st) {
  flope_tf_encoder* e = s->e;
  const size_t layer = (size_t)s->tracks * s->capacity * 2 * e->d;
  const int plan = tf_extend_plan<T>(e, s, tf_extend_positions_ok(s, n, lengths));
  return run_forward_with<T>(e, x, n, L, y, st, &rg, [&](int li) {
    T* cache = (T*)s->cache + (size_t)li * layer;
    const int rc = launch_extend_attn<T>(s, plan, (const T*)e->qkv, (const T*)cache, (T*)e->att, n, rg.max_len, smax, st);
    if (rc < 0) return rc;
    return launch_cache_copy<T>(s, (const T*)e->qkv, cache, (const int*)e->vl_off, (const int*)s->tab, n, rg.max_len, st);
  });
}

}  // namespace

namespace {
// window = 0: flope_tf_stream_open, the linear cache; window >= 1: flope_tf_stream_open_window, the ring.
// planes >= 1: flope_tf_stream_open_bias -- the state's distance table rel [planes][rel_d], already checked, is uploaded here, once and
// synchronously, into an allocation of the state's own
int tf_stream_open(flope_tf_handle e, const std::string& who, int tracks, int capacity, int window, flope_tf_stream* out, int planes = 0, int rel_d = 0,
                   const float* rel_host = nullptr, int max_rows = 0) {
  if (!out) return tf_fail(e, FLOPE_EINVAL, who + ": NULL out");
  *out = nullptr;
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (flope_tf_plan::tf_stream_check_open(tracks, capacity))
    return tf_fail(e, FLOPE_EINVAL, who + ": tracks must be positive and capacity 1 .. " + std::to_string(flope_tf_plan::kTfStreamMaxCapacity) +
                                        " (the score rows of tf_attn_step live in 64 KiB of LDS)");
  if (window && flope_tf_plan::tf_stream_check_open_window(tracks, capacity, window))
    return tf_fail(e, FLOPE_EINVAL, who + ": window = " + std::to_string(window) + " is outside 1 .. capacity = " + std::to_string(capacity) +
                                        " (the ring must hold every key of a window)");
  TF_HIP(e, hipSetDevice(e->device));
  const size_t bytes = (size_t)e->nl * tracks * capacity * 2 * e->d * e->esz;
  flope_tf_stream_s* s = new flope_tf_stream_s();
  s->e = e; s->tracks = tracks; s->capacity = capacity; s->window = window;
  // num_layers = 0 has no cache; the allocation keeps one row so that the pointer is a pointer.  The table: 5 ints per track, or the 2
  // per row of a device-positioned state
  const size_t tab_ints = max_rows ? (size_t)2 * max_rows : (size_t)5 * tracks;
  if (hipMalloc(&s->cache, bytes ? bytes : 16) != hipSuccess || hipMalloc((void**)&s->tab, tab_ints * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(s->cache); hipFree(s->tab);
    delete s;
    return tf_fail(e, FLOPE_EHIP, who + ": hipMalloc failed for a cache of " + std::to_string(bytes) + " bytes (num_layers x tracks x capacity x 2 model_dim)");
  }
  if (max_rows) {                                  // positions, zeroed; the token rows; the table starts as "no row" (feed_n = 0)
    const size_t tb = (size_t)max_rows * e->in_dim * sizeof(float);
    if (hipMalloc((void**)&s->pos_dev, (size_t)tracks * sizeof(int)) != hipSuccess || hipMalloc((void**)&s->tok, tb) != hipSuccess ||
        hipMemset(s->pos_dev, 0, (size_t)tracks * sizeof(int)) != hipSuccess || hipMemset(s->tok, 0, tb) != hipSuccess ||
        hipMemset(s->tab, 0, tab_ints * sizeof(int)) != hipSuccess || hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      hipFree(s->cache); hipFree(s->tab); hipFree(s->pos_dev); hipFree(s->tok);
      if (s->ev) hipEventDestroy(s->ev);
      delete s;
      return tf_fail(e, FLOPE_EHIP, who + ": allocating " + std::to_string(tracks) + " positions and " + std::to_string(tb) + " bytes of token rows failed");
    }
    s->max_rows = max_rows;
  }
  if (planes) {
    const size_t rb = flope_tf_plan::tf_stream_bias_bytes(planes, rel_d);
    hipError_t err = hipMalloc((void**)&s->rel, rb);
    const bool alloc_failed = err != hipSuccess;
    if (!alloc_failed) err = hipMemcpy(s->rel, rel_host, rb, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
      (void)hipGetLastError();
      hipFree(s->cache); hipFree(s->tab); hipFree(s->rel); hipFree(s->pos_dev); hipFree(s->tok);
      if (s->ev) hipEventDestroy(s->ev);
      delete s;
      return tf_fail(e, FLOPE_EHIP, who + (alloc_failed ? ": hipMalloc failed for" : ": the upload failed of") + " a distance table of " + std::to_string(rb) +
                                        " bytes (planes x distances x 4): " + hipGetErrorString(err));
    }
    s->planes = planes; s->rel_d = rel_d;
  }
  if (!max_rows) {
    s->pos.assign((size_t)tracks, 0);
    s->tab_host.assign((size_t)5 * tracks, 0);
    s->seen.assign((size_t)tracks, 0);
  }
  e->streams.push_back(s);
  *out = s;
  return FLOPE_OK;
}
}  // namespace

extern "C" int flope_tf_stream_open(flope_tf_handle e, int tracks, int capacity, flope_tf_stream* out) {
  return tf_stream_open(e, "flope_tf_stream_open", tracks, capacity, 0, out);
}

extern "C" int flope_tf_stream_open_window(flope_tf_handle e, int tracks, int capacity, int window, flope_tf_stream* out) {
  if (out && e && window < 1) {
    *out = nullptr;
    return tf_fail(e, FLOPE_EINVAL, "flope_tf_stream_open_window: window = " + std::to_string(window) + " is outside 1 .. capacity (flope_tf_stream_open is the state without a window)");
  }
  return tf_stream_open(e, "flope_tf_stream_open_window", tracks, capacity, window, out);
}

namespace {
// a state with a distance table, host- or device-positioned (max_rows > 0): the table's refusals, then the open
int tf_stream_open_biased(flope_tf_handle e, const std::string& who, int tracks, int capacity, int window, int planes, int distances, const float* table_host,
                          flope_tf_stream* out, int max_rows) {
  using namespace flope_tf_plan;
  // the state's own refusals first: a table is judged against a capacity and a window that are ones
  if (tf_stream_check_open(tracks, capacity) == kTfStreamOk && (!window || tf_stream_check_open_window(tracks, capacity, window) == kTfStreamOk)) {
    int bp = -1, bd = -1;
    switch (tf_stream_check_open_bias(capacity, window, e->H, planes, distances, table_host, &bp, &bd)) {
      case kTfStreamBiasPlanes:
        return tf_fail(e, FLOPE_EINVAL, who + ": planes = " + std::to_string(planes) + " is neither 1 nor num_heads = " + std::to_string(e->H));
      case kTfStreamBiasDistances:
        return tf_fail(e, FLOPE_EINVAL, who + ": distances = " + std::to_string(distances) + ", but this state needs " +
                                            std::to_string(tf_stream_bias_distances(capacity, window)) + (window ? " (its window)" : " (its capacity)"));
      case kTfStreamBiasNull:
        return tf_fail(e, FLOPE_EINVAL, who + ": NULL table");
      case kTfStreamBiasValue:
        return tf_fail(e, FLOPE_EINVAL, who + ": table[" + std::to_string(bp) + "][" + std::to_string(bd) + "] = " + std::to_string(table_host[(size_t)bp * distances + bd]) +
                                            " (plane, distance) is not finite (-inf is no way to mask here: visibility stays with the window)");
      default: break;
    }
  }
  return tf_stream_open(e, who, tracks, capacity, window, out, planes, distances, table_host, max_rows);
}
}  // namespace

extern "C" int flope_tf_stream_open_bias(flope_tf_handle e, int tracks, int capacity, int window, int planes, int distances, const float* table_host,
                                         flope_tf_stream* out) {
  const std::string who = "flope_tf_stream_open_bias";
  if (!out) return tf_fail(e, FLOPE_EINVAL, who + ": NULL out");
  *out = nullptr;
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (window < 0) return tf_fail(e, FLOPE_EINVAL, who + ": window = " + std::to_string(window) + " is negative (0: the linear state; 1 .. capacity: the ring)");
  return tf_stream_open_biased(e, who, tracks, capacity, window, planes, distances, table_host, out, 0);
}

extern "C" int flope_tf_stream_open_device(flope_tf_handle e, int tracks, int capacity, int window, int max_rows, int planes, int distances,
                                           const float* table_host, flope_tf_stream* out) {
  const std::string who = "flope_tf_stream_open_device";
  if (!out) return tf_fail(e, FLOPE_EINVAL, who + ": NULL out");
  *out = nullptr;
  if (!e) return tf_fail(nullptr, FLOPE_EINVAL, who + ": NULL handle");
  if (window < 1)
    return tf_fail(e, FLOPE_EINVAL, who + ": window = " + std::to_string(window) + " is outside 1 .. capacity (a device-positioned state is windowed: its launches are sized by the window, not by a position)");
  if (max_rows < 1 || max_rows > e->max_tokens)
    return tf_fail(e, FLOPE_EINVAL, who + ": max_rows = " + std::to_string(max_rows) + " is outside 1 .. max_tokens = " + std::to_string(e->max_tokens));
  if (planes == 0 && !table_host) return tf_stream_open(e, who, tracks, capacity, window, out, 0, 0, nullptr, max_rows);
  return tf_stream_open_biased(e, who, tracks, capacity, window, planes, distances, table_host, out, max_rows);
}

extern "C" int flope_tf_stream_bias_planes(flope_tf_stream s) {
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_stream_enter(s, "flope_tf_stream_bias_planes", &e))) return rc;
  return s->planes;
}

extern "C" int flope_tf_stream_close(flope_tf_stream s) {
  if (!s) return FLOPE_OK;
  if (flope_tf_encoder* e = s->e) {
    hipSetDevice(e->device);
    if (s->ev) { hipEventSynchronize(s->ev); hipEventDestroy(s->ev); }
    hipFree(s->cache); hipFree(s->tab); hipFree(s->rel); hipFree(s->pos_dev); hipFree(s->tok);
    for (auto it = e->streams.begin(); it != e->streams.end(); ++it)
      if (*it == s) { e->streams.erase(it); break; }
  }
  delete s;
  return FLOPE_OK;
}

extern "C" int flope_tf_stream_reset(flope_tf_stream s, int n, const int* tracks_host) {
  flope_tf_encoder* e;
  int rc, bad = -1;
  if ((rc = tf_stream_enter_host(s, "flope_tf_stream_reset", &e, "use flope_tf_stream_reset_device"))) return rc;
  if ((rc = flope_tf_plan::tf_stream_check_reset(s->tracks, n, tracks_host, &bad)))
    return tf_stream_refuse(s, "flope_tf_stream_reset", rc, bad, n, tracks_host, nullptr, 0);
  if (!tracks_host) s->pos.assign((size_t)s->tracks, 0);
  else for (int r = 0; r < n; ++r) s->pos[(size_t)tracks_host[r]] = 0;
  return FLOPE_OK;
}

extern "C" int flope_tf_stream_position(flope_tf_stream s, int track) {
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_stream_enter_host(s, "flope_tf_stream_position", &e, "use flope_tf_stream_read_positions"))) return rc;
  if (track < 0 || track >= s->tracks)
    return tf_fail(e, FLOPE_EINVAL, "flope_tf_stream_position: track " + std::to_string(track) + " is outside 0 .. " + std::to_string(s->tracks - 1));
  return s->pos[(size_t)track];
}

extern "C" int flope_tf_stream_step(flope_tf_stream s, const float* x_dev, int n, const int* tracks_host, float* y_dev, void* stream) {
  const std::string who = "flope_tf_stream_step";
  flope_tf_encoder* e;
  int rc, bad = -1, max_pos = 0;
  if ((rc = tf_stream_enter_host(s, who, &e, "use flope_tf_stream_step_assoc or flope_tf_stream_step_tracker"))) return rc;
  if (!e->loaded) return tf_fail(e, FLOPE_ESTATE, who + ": weights not loaded");
  rc = s->window ? flope_tf_plan::tf_stream_check_step_window(s->pos.data(), s->tracks, s->window, e->max_tokens, n, tracks_host, s->seen.data(), &bad, &max_pos)
                 : flope_tf_plan::tf_stream_check_step(s->pos.data(), s->tracks, s->capacity, e->max_tokens, n, tracks_host, s->seen.data(), &bad, &max_pos);
  if (rc)
    return tf_stream_refuse(s, who, rc, bad, n, tracks_host, nullptr, 0);
  if (!x_dev || !y_dev) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  flope_tf_plan::tf_stream_step_table(s->pos.data(), n, tracks_host, s->tab_host.data());
  // pageable source, as the offsets of a ragged batch: staged when the call returns, so the next call may overwrite tab_host
  TF_HIP(e, hipMemcpyAsync(s->tab, s->tab_host.data(), (size_t)2 * n * sizeof(int), hipMemcpyHostToDevice, st));
  flope_tf_plan::tf_stream_advance(s->pos.data(), n, tracks_host);
  return tf_by_dtype(e, [&](auto tag) { return run_step<typename decltype(tag)::type>(s, x_dev, n, max_pos, y_dev, st); });
}

extern "C" int flope_tf_stream_prefill(flope_tf_stream s, const float* x_dev, int n, int seq_len, const int* lengths_host, const int* tracks_host, float* y_dev,
                                       void* stream) {
  const std::string who = "flope_tf_stream_prefill";
  flope_tf_encoder* e;
  int rc, bad = -1;
  if ((rc = tf_stream_enter_host(s, who, &e, "a device-positioned state has no prefill: feed it with flope_tf_stream_step_assoc or flope_tf_stream_step_tracker"))) return rc;
  if ((rc = tf_check_forward_varlen(e, who, n, seq_len, x_dev && y_dev))) return rc;
  std::vector<int> full;                            // lengths_host NULL: every sequence has seq_len tokens
  if (!lengths_host && n > 0) full.assign((size_t)n, seq_len);
  const int* lengths = lengths_host ? lengths_host : full.data();
  TfRagged rg;
  if ((rc = tf_check_ragged(e, who.c_str(), lengths, n, seq_len, e->vl_host.data(), &rg))) return rc;
  rc = s->window ? flope_tf_plan::tf_stream_check_prefill_window(s->tracks, n, tracks_host, s->seen.data(), &bad)
                 : flope_tf_plan::tf_stream_check_prefill(s->tracks, s->capacity, n, seq_len, lengths, tracks_host, s->seen.data(), &bad);
  if (rc)
    return tf_stream_refuse(s, who, rc, bad, n, tracks_host, lengths, seq_len);
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  if ((rc = tf_upload_ragged(e, n, st))) return rc;
  for (int b = 0; b < n; ++b) { s->tab_host[(size_t)2 * b] = tf_stream_track(tracks_host, b); s->tab_host[(size_t)2 * b + 1] = 0; }   // every sequence starts its track
  TF_HIP(e, hipMemcpyAsync(s->tab, s->tab_host.data(), (size_t)2 * n * sizeof(int), hipMemcpyHostToDevice, st));
  flope_tf_plan::tf_stream_set_lengths(s->pos.data(), n, seq_len, lengths, tracks_host);
  const int causal = e->opt_causal, window = e->opt_window;       // causal and the state's window for these launches only; last_fwd is tf_forward's and stays
  e->opt_causal = 1;
  e->opt_window = s->window;
  rc = tf_by_dtype(e, [&](auto tag) { return run_prefill<typename decltype(tag)::type>(s, x_dev, n, seq_len, rg, y_dev, st); });
  e->opt_causal = causal;
  e->opt_window = window;
  return rc;
}

extern "C" int flope_tf_stream_extend(flope_tf_stream s, const float* x_dev, int n, int seq_len, const int* lengths_host, const int* tracks_host, float* y_dev,
                                      void* stream) {
  const std::string who = "flope_tf_stream_extend";
  flope_tf_encoder* e;
  int rc, bad = -1, smax = 0;
  if ((rc = tf_stream_enter_host(s, who, &e, "a device-positioned state has no extend: use flope_tf_stream_step_assoc or flope_tf_stream_step_tracker"))) return rc;
  if ((rc = tf_check_forward_varlen(e, who, n, seq_len, x_dev && y_dev))) return rc;
  std::vector<int> full;                            // lengths_host NULL: every chunk has seq_len tokens
  if (!lengths_host && n > 0) full.assign((size_t)n, seq_len);
  const int* lengths = lengths_host ? lengths_host : full.data();
  TfRagged rg;
  if ((rc = tf_check_ragged(e, who.c_str(), lengths, n, seq_len, e->vl_host.data(), &rg))) return rc;
  if ((rc = flope_tf_plan::tf_stream_check_extend(s->pos.data(), s->tracks, s->capacity, s->window, n, lengths, tracks_host, s->seen.data(), &bad, &smax))) {
    if (rc == flope_tf_plan::kTfStreamRoom || rc == flope_tf_plan::kTfStreamFull) {
      const int t = tf_stream_track(tracks_host, bad);
      const std::string head = who + ": lengths[" + std::to_string(bad) + "] = " + std::to_string(lengths[bad]) + ": track " + std::to_string(t) + " holds " +
                               std::to_string(s->pos[(size_t)t]) + " tokens, ";
      if (rc == flope_tf_plan::kTfStreamRoom)
        return tf_fail(e, FLOPE_EINVAL, head + "and the chunk would pass capacity = " + std::to_string(s->capacity) + " (reset the track, or open a state with more room)");
      return tf_fail(e, FLOPE_EINVAL, head + "and the chunk would pass INT_MAX = " + std::to_string(INT_MAX) + ", the last position an int counts (reset the track)");
    }
    if (rc == flope_tf_plan::kTfStreamDuplicate)
      return tf_fail(e, FLOPE_EINVAL, who + ": tracks[" + std::to_string(bad) + "] = " + std::to_string(tracks_host[bad]) +
                                          " names a track an earlier sequence names (one sequence per track and call)");
    return tf_stream_refuse(s, who, rc, bad, n, tracks_host, lengths, seq_len);
  }
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  if ((rc = tf_upload_ragged(e, n, st))) return rc;
  flope_tf_plan::tf_stream_step_table(s->pos.data(), n, tracks_host, s->tab_host.data());
  TF_HIP(e, hipMemcpyAsync(s->tab, s->tab_host.data(), (size_t)2 * n * sizeof(int), hipMemcpyHostToDevice, st));
  // the positions move only once every launch is enqueued: a call that fails on the way (FLOPE_EHIP) leaves the tracks where they were.
  // On a linear state the rows it may have written lie behind the positions, where nothing reads them; on a ring they may have taken
  // the rows of keys a later window still holds, so reset the call's tracks after such a failure
  if ((rc = tf_by_dtype(e, [&](auto tag) { return run_extend<typename decltype(tag)::type>(s, x_dev, n, seq_len, rg, lengths, smax, y_dev, st); }))) return rc;
  flope_tf_plan::tf_stream_extend_advance(s->pos.data(), n, lengths, tracks_host);
  return FLOPE_OK;
}

extern "C" int flope_tf_stream_step_plan(flope_tf_stream s) {
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_stream_enter(s, "flope_tf_stream_step_plan", &e))) return rc;
  return tf_by_dtype(e, [&](auto tag) { return tf_step_plan<typename decltype(tag)::type>(e, s); });
}

// ---- a device-positioned state stepped by an association ----------------------------------------------------------------
namespace {
// What _step_assoc and _step_tracker share behind their checks: tf_stream_feed_kernel (the table, the positions, the token rows),
// _step's launch sequence for all n rows over the token buffer at smax = window, tf_feed_fill_bias.  SOURCE and its arrays as the
// kernel takes them.
int run_step_feed(flope_tf_stream_s* s, int source, const int* assoc, const int* overflow, int n, const double* vec7, int vec_rows, const float* x, float* y,
                  hipStream_t st) {
  flope_tf_encoder* e = s->e;
  const dim3 grid((unsigned)((n + kTfFeedBlock - 1) / kTfFeedBlock)), block(kTfFeedBlock);
#define TF_FEED(SRC_) hipLaunchKernelGGL((tf_stream_feed_kernel<SRC_>), grid, block, 0, st, assoc, overflow, n, s->tracks, s->pos_dev, s->tab, vec7, vec_rows, x, \
                                         e->in_dim, s->tok)
  if (source == kTfFeedRows) TF_FEED(kTfFeedRows);
  else if (source == FLOPE_TF_FEED_MEAN) TF_FEED(FLOPE_TF_FEED_MEAN);
  else TF_FEED(FLOPE_TF_FEED_MEAS);
#undef TF_FEED
  TF_HIP(e, hipGetLastError());
  s->feed_n = n;
  // no position is known here: a score row holds at most `window` keys (tf_window_keys <= W), which is what the launch is sized for
  int rc = tf_by_dtype(e, [&](auto tag) { return run_step<typename decltype(tag)::type>(s, s->tok, n, s->window - 1, y, st); });
  if (rc < 0) return rc;
  const size_t total = (size_t)n * e->out_dim;
  hipLaunchKernelGGL(tf_feed_fill_bias, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const int*)s->tab, (const float*)e->outl.b, y, e->out_dim, total);
  TF_HIP(e, hipGetLastError());
  TF_HIP(e, hipEventRecord(s->ev, st));
  return 0;
}

// the checks both start with; n: the call's rows
int tf_feed_enter(flope_tf_stream_s* s, const std::string& who, flope_tf_encoder** e) {
  int rc;
  if ((rc = tf_stream_enter_device(s, who, e))) return rc;
  if (!(*e)->loaded) return tf_fail(*e, FLOPE_ESTATE, who + ": weights not loaded");
  return 0;
}
int tf_feed_rows_ok(flope_tf_stream_s* s, const std::string& who, int n) {
  if (n < 0 || n > s->max_rows)
    return tf_fail(s->e, FLOPE_EINVAL, who + ": n = " + std::to_string(n) + " is outside 0 .. max_rows = " + std::to_string(s->max_rows));
  return 0;
}
}  // namespace

extern "C" int flope_tf_stream_step_assoc(flope_tf_stream s, const float* x_dev, const int32_t* assoc_dev, const int32_t* overflow_dev, int n, float* y_dev,
                                          void* stream) {
  const std::string who = "flope_tf_stream_step_assoc";
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_feed_enter(s, who, &e))) return rc;
  if ((rc = tf_feed_rows_ok(s, who, n))) return rc;
  if (n == 0) return FLOPE_OK;
  if (!x_dev || !assoc_dev || !y_dev) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  TF_HIP(e, hipSetDevice(e->device));
  return run_step_feed(s, kTfFeedRows, assoc_dev, overflow_dev, n, nullptr, 0, x_dev, y_dev, (hipStream_t)stream);
}

extern "C" int flope_tf_stream_step_tracker(flope_tf_stream s, flope_track_handle t, int source, float* y_dev, void* stream) {
  const std::string who = "flope_tf_stream_step_tracker";
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_feed_enter(s, who, &e))) return rc;
  flope_track_view v;
  if (!t || flope_track_device_view(t, &v) != FLOPE_OK) return tf_fail(e, FLOPE_EINVAL, who + ": NULL tracker");
  if (source != FLOPE_TF_FEED_MEAS && source != FLOPE_TF_FEED_MEAN)
    return tf_fail(e, FLOPE_EINVAL, who + ": source = " + std::to_string(source) + " is neither FLOPE_TF_FEED_MEAS nor FLOPE_TF_FEED_MEAN");
  if (e->in_dim < flope_tf_plan::kTfFeedDim)
    return tf_fail(e, FLOPE_EINVAL, who + ": input_dim = " + std::to_string(e->in_dim) + " is below 7, the tracker's vector (world position, quaternion x y z w)");
  if (v.device != e->device) return tf_fail(e, FLOPE_EINVAL, who + ": the tracker lives on device " + std::to_string(v.device) + ", the encoder on " + std::to_string(e->device));
  if (v.n < 0) return tf_fail(e, FLOPE_ESTATE, who + ": the tracker has had no update since flope_track_create / flope_track_reset");
  if (s->fed_tracker == (const void*)t && s->fed_serial == v.serial)
    return tf_fail(e, FLOPE_ESTATE, who + ": update " + std::to_string(v.serial) + " of this tracker has been fed to this state already (one token per track and update)");
  if ((rc = tf_feed_rows_ok(s, who, v.n))) return rc;
  if (!y_dev) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  TF_HIP(e, hipStreamWaitEvent(st, (hipEvent_t)v.event, 0));
  s->fed_tracker = (const void*)t;
  s->fed_serial = v.serial;
  const bool mean = source == FLOPE_TF_FEED_MEAN;
  if ((rc = run_step_feed(s, source, v.assoc, v.count + 1, v.n, mean ? v.means : v.meas, mean ? v.max_tracks : v.n, nullptr, y_dev, st))) return rc;
  return v.n;
}

extern "C" int flope_tf_stream_reset_device(flope_tf_stream s, void* stream) {
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_stream_enter_device(s, "flope_tf_stream_reset_device", &e))) return rc;
  TF_HIP(e, hipSetDevice(e->device));
  TF_HIP(e, hipMemsetAsync(s->pos_dev, 0, (size_t)s->tracks * sizeof(int), (hipStream_t)stream));
  TF_HIP(e, hipEventRecord(s->ev, (hipStream_t)stream));
  s->fed_tracker = nullptr;                        // (a tracker that was reset too starts a new run of updates: none of them has been fed)
  return FLOPE_OK;
}

extern "C" int flope_tf_stream_read_positions(flope_tf_stream s, int32_t* pos_host, int cap) {
  const std::string who = "flope_tf_stream_read_positions";
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_stream_enter_device(s, who, &e))) return rc;
  if (!pos_host || cap < s->tracks) return tf_fail(e, FLOPE_EINVAL, who + ": pos_host is NULL or holds fewer than tracks = " + std::to_string(s->tracks) + " ints");
  TF_HIP(e, hipSetDevice(e->device));
  TF_HIP(e, hipEventSynchronize(s->ev));
  TF_HIP(e, hipMemcpy(pos_host, s->pos_dev, (size_t)s->tracks * sizeof(int), hipMemcpyDeviceToHost));
  return s->tracks;
}

extern "C" int flope_tf_stream_read_feed(flope_tf_stream s, int32_t* track_host, int32_t* pos_host, int cap) {
  const std::string who = "flope_tf_stream_read_feed";
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_stream_enter_device(s, who, &e))) return rc;
  const int n = s->feed_n;
  if (n == 0) return 0;
  if (!track_host || !pos_host || cap < n) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer, or room for fewer than the last call's " + std::to_string(n) + " rows");
  TF_HIP(e, hipSetDevice(e->device));
  TF_HIP(e, hipEventSynchronize(s->ev));
  std::vector<int> tab((size_t)2 * n);
  TF_HIP(e, hipMemcpy(tab.data(), s->tab, tab.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int m = 0; m < n; ++m) { track_host[m] = tab[(size_t)2 * m]; pos_host[m] = tab[(size_t)2 * m + 1]; }
  return n;
}

extern "C" int flope_tf_stream_read_tokens(flope_tf_stream s, float* tok_host, int cap_rows) {
  const std::string who = "flope_tf_stream_read_tokens";
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_stream_enter_device(s, who, &e))) return rc;
  const int n = s->feed_n;
  if (n == 0) return 0;
  if (!tok_host || cap_rows < n) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer, or room for fewer than the last call's " + std::to_string(n) + " rows");
  TF_HIP(e, hipSetDevice(e->device));
  TF_HIP(e, hipEventSynchronize(s->ev));
  TF_HIP(e, hipMemcpy(tok_host, s->tok, (size_t)n * e->in_dim * sizeof(float), hipMemcpyDeviceToHost));
  return n;
}

namespace {
// What the two test hooks (flope_tf_stream_attention, flope_tf_stream_attention_extend) share.  Sequence b of their padded batch
// [n][seq_len] is for track b: its first `hist` rows are the track's history, the `own` rows behind them the step's token or the
// extend's chunk.  The table (s->tab, 5 n ints): (b, hist) per sequence -- the table of the attention launch -- then (b, 0, hist) per
// sequence: (b, 0) is the one-entry table of that sequence's cache copy and (0, hist) its offsets.
void tf_hook_table_entry(flope_tf_stream_s* s, int n, int b, int hist) {
  int* t = s->tab_host.data();
  t[2 * b] = b; t[2 * b + 1] = hist;
  t[2 * n + 3 * b] = b; t[2 * n + 3 * b + 1] = 0; t[2 * n + 3 * b + 2] = hist;
  s->pos[(size_t)b] = 0;                               // a test hook: the rows it loads are no history of the track
}
// ... and the staging of sequence b (seq: its first row): the k | v columns of the history into layer 0's part of track b
// (tf_cache_append, one launch per sequence: the batch is padded, not packed), the own rows into the handle's qkv buffer from row dst on
template <typename T>
int tf_hook_stage(flope_tf_stream_s* s, const T* seq, int n, int b, int hist, int own, int dst, hipStream_t st) {
  flope_tf_encoder* e = s->e;
  const size_t row = (size_t)3 * e->d;
  TF_HIP(e, hipMemcpyAsync((T*)e->qkv + (size_t)dst * row, seq + (size_t)hist * row, (size_t)own * row * sizeof(T), hipMemcpyDeviceToDevice, st));
  if (hist < 1) return 0;
  const int* tab = (const int*)s->tab + 2 * n + 3 * b;
  return launch_cache_copy<T>(s, seq, (T*)s->cache, tab + 1, tab, 1, hist, st);
}
// ... and the refusals both make in the same words
int tf_hook_refuse(flope_tf_stream_s* s, const std::string& who, int rc, int bad, int n, int seq_len, const int* lengths, const char* or_else) {
  flope_tf_encoder* e = s->e;
  if (rc == flope_tf_plan::kTfStreamLength)
    return tf_fail(e, FLOPE_EINVAL, who + ": lengths[" + std::to_string(bad) + "] = " + std::to_string(lengths ? lengths[bad] : seq_len) + " is outside 1 .. seq_len = " +
                                        std::to_string(seq_len) + (s->window ? "" : ", or above capacity = " + std::to_string(s->capacity)));
  return tf_fail(e, FLOPE_EINVAL, who + ": n = " + std::to_string(n) + " is outside 1 .. min(tracks = " + std::to_string(s->tracks) + ", max_tokens = " +
                                      std::to_string(e->max_tokens) + ")" + or_else);
}

// flope_tf_stream_attention behind its checks: per sequence rows 0 .. len - 2 are the history and row len - 1 the token (row b of the
// handle's qkv buffer), then the step's attention launch
template <typename T>
int run_stream_attention(flope_tf_stream_s* s, const T* qkv, int n, int L, const int* lengths, T* att, int max_pos, hipStream_t st) {
  flope_tf_encoder* e = s->e;
  for (int b = 0; b < n; ++b) {
    const int rc = tf_hook_stage<T>(s, qkv + (size_t)b * L * 3 * e->d, n, b, (lengths ? lengths[b] : L) - 1, 1, b, st);
    if (rc) return rc;
  }
  return launch_step_attn<T>(s, (const T*)e->qkv, (T*)s->cache, att, n, max_pos, st);
}
}  // namespace

extern "C" int flope_tf_stream_attention(flope_tf_stream s, const void* qkv_dev, int n, int seq_len, const int* lengths_host, void* att_dev, void* stream) {
  const std::string who = "flope_tf_stream_attention";
  flope_tf_encoder* e;
  int rc, bad = -1, max_pos = 0;
  if ((rc = tf_stream_enter_host(s, who, &e, "the hook moves positions on the host: use a state of flope_tf_stream_open_window"))) return rc;
  if (e->nl < 1) return tf_fail(e, FLOPE_EINVAL, who + ": an encoder without layers has no cache");
  if ((rc = flope_tf_plan::tf_stream_check_attention(s->tracks, s->capacity, s->window, e->max_tokens, n, seq_len, lengths_host, &bad, &max_pos)))
    return tf_hook_refuse(s, who, rc, bad, n, seq_len, lengths_host, ", or seq_len < 1");
  if (!qkv_dev || !att_dev) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  if (((uintptr_t)qkv_dev | (uintptr_t)att_dev) & 15) return tf_fail(e, FLOPE_EINVAL, who + ": buffer not aligned to 16 bytes");
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  for (int b = 0; b < n; ++b) tf_hook_table_entry(s, n, b, (lengths_host ? lengths_host[b] : seq_len) - 1);
  TF_HIP(e, hipMemcpyAsync(s->tab, s->tab_host.data(), (size_t)5 * n * sizeof(int), hipMemcpyHostToDevice, st));
  return tf_by_dtype(e, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return run_stream_attention<T>(s, (const T*)qkv_dev, n, seq_len, lengths_host, (T*)att_dev, max_pos, st);
  });
}

extern "C" int flope_tf_stream_extend_plan(flope_tf_stream s) {
  flope_tf_encoder* e;
  int rc;
  if ((rc = tf_stream_enter(s, "flope_tf_stream_extend_plan", &e))) return rc;
  return tf_by_dtype(e, [&](auto tag) { return tf_extend_plan<typename decltype(tag)::type>(e, s); });
}

namespace {
// flope_tf_stream_attention_extend behind its checks: per sequence rows 0 .. cached - 1 are the history and rows cached .. len - 1 the
// chunk, packed into the handle's qkv buffer; the extend's attention launch over them, and the packed rows of the handle's att buffer
// back to their places in att
template <typename T>
int run_stream_attention_extend(flope_tf_stream_s* s, const T* qkv, int n, int L, const int* lengths, const int* cached, T* att, int smax, int max_len,
                                hipStream_t st) {
  flope_tf_encoder* e = s->e;
  const int d = e->d;
  for (int b = 0; b < n; ++b) {
    const int rc = tf_hook_stage<T>(s, qkv + (size_t)b * L * 3 * d, n, b, cached[b], lengths[b] - cached[b], e->vl_host[(size_t)b], st);
    if (rc) return rc;
  }
  std::vector<int> chunk((size_t)n);
  for (int b = 0; b < n; ++b) chunk[(size_t)b] = lengths[b] - cached[b];
  const int plan = tf_extend_plan<T>(e, s, tf_extend_positions_ok(s, n, chunk.data()));
  const int rc = launch_extend_attn<T>(s, plan, (const T*)e->qkv, (const T*)s->cache, (T*)e->att, n, max_len, smax, st);
  if (rc < 0) return rc;
  for (int b = 0; b < n; ++b)
    TF_HIP(e, hipMemcpyAsync(att + ((size_t)b * L + cached[b]) * d, (const T*)e->att + (size_t)e->vl_host[(size_t)b] * d, (size_t)chunk[(size_t)b] * d * sizeof(T),
                             hipMemcpyDeviceToDevice, st));
  return rc;
}
}  // namespace

extern "C" int flope_tf_stream_attention_extend(flope_tf_stream s, const void* qkv_dev, int n, int seq_len, const int* lengths_host, const int* cached_host,
                                                void* att_dev, void* stream) {
  using namespace flope_tf_plan;
  const std::string who = "flope_tf_stream_attention_extend";
  flope_tf_encoder* e;
  int rc, bad = -1, smax = 0, max_len = 0, total = 0;
  if ((rc = tf_stream_enter_host(s, who, &e, "the hook moves positions on the host: use a state of flope_tf_stream_open_window"))) return rc;
  if (e->nl < 1) return tf_fail(e, FLOPE_EINVAL, who + ": an encoder without layers has no cache");
  if ((rc = tf_stream_check_attention_extend(s->tracks, s->capacity, s->window, e->max_tokens, n, seq_len, lengths_host, cached_host, &bad, &smax, &max_len, &total))) {
    if (rc == kTfStreamCached)
      return tf_fail(e, FLOPE_EINVAL, who + ": cached[" + std::to_string(bad) + "] = " + std::to_string(cached_host[bad]) + " is outside 0 .. lengths[" + std::to_string(bad) +
                                          "] - 1 = " + std::to_string(lengths_host[bad] - 1));
    if (rc == kTfStreamTokens) return tf_fail(e, FLOPE_EINVAL, who + ": the chunks together exceed max_tokens given to flope_tf_create");
    return tf_hook_refuse(s, who, rc, bad, n, seq_len, lengths_host, ", seq_len < 1, or lengths_host / cached_host is NULL");
  }
  if (!qkv_dev || !att_dev) return tf_fail(e, FLOPE_EINVAL, who + ": NULL buffer");
  if (((uintptr_t)qkv_dev | (uintptr_t)att_dev) & 15) return tf_fail(e, FLOPE_EINVAL, who + ": buffer not aligned to 16 bytes");
  TF_HIP(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  int run = 0;
  for (int b = 0; b < n; ++b) {
    e->vl_host[(size_t)b] = run;
    run += lengths_host[b] - cached_host[b];
    tf_hook_table_entry(s, n, b, cached_host[b]);
  }
  e->vl_host[(size_t)n] = run;
  if ((rc = tf_upload_ragged(e, n, st))) return rc;
  TF_HIP(e, hipMemcpyAsync(s->tab, s->tab_host.data(), (size_t)5 * n * sizeof(int), hipMemcpyHostToDevice, st));
  return tf_by_dtype(e, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return run_stream_attention_extend<T>(s, (const T*)qkv_dev, n, seq_len, lengths_host, cached_host, (T*)att_dev, smax, max_len, st);
  });
}

#ifdef FLOPE_STAG_DBG
extern "C" int flope_tfdbg_read(unsigned long long* dst_host, int cap_records) {
  unsigned n = 0;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_tfdbg_n), sizeof(n)) != hipSuccess) return -1;
  const int m0 = (int)(n < 512u ? n : 512u), m = m0 < cap_records ? m0 : cap_records;
  if (m > 0 && hipMemcpyFromSymbol(dst_host, HIP_SYMBOL(g_tfdbg), (size_t)m * 64) != hipSuccess) return -1;
  n = 0;
  hipMemcpyToSymbol(HIP_SYMBOL(g_tfdbg_n), &n, sizeof(n));
  return m;
}
#endif
