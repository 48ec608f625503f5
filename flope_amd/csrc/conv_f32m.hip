// Float32 trunk on the matrix cores (FLOPE_DT_F32 with option f32mfma = 1): implicit-GEMM convolution on
// v_mfma_f32_16x16x4_f32, which takes float32 operands and accumulates in float32 -- every product-sum is an fmaf chain, so the
// result differs from naive_conv_kernel (naive.hip, the checker: f32mfma = 0) only in summation order.
//   D[channel][pixel] += W[channel][k] X[k][pixel]: weights = A operand (16 rows x 4 k per instruction), 16 output pixels = B.
//   A lane's 16-byte load is four consecutive k of its weight row / of its pixel, and element s feeds MFMA s of a 16-deep K step
//   on BOTH operands (the k order inside a step is permuted identically for A and B).  k = tap * Cin + ci on NHWC, Cin % 16 == 0:
//   a step lies inside one tap, so the tap offset is scalar arithmetic; the zero ring makes 3x3 taps pure addressing.
//   Stem (7x7 stride 2, 4 stored input channels): one tap is one lane's 16-byte load, k = 4 tap + c, K = 196 padded to 13 steps
//   with zero weights (the padding taps re-read tap 48).
//   Wave tile: MP x 16 pixels x 64 channels (4 MP independent accumulator tiles); the four waves of a workgroup take consecutive
//   pixel tiles of one 64-channel block and share its weights (packed in A-fragment order, host_pack.h pack_f32m: a wave's load of
//   one (step, channel tile) is one contiguous KiB) through L1 / L2.  Operands come straight from global memory, the next step's
//   loads in flight under this step's MFMAs (16 MP MFMAs = 512 MP cycles per step).  No barrier, no atomics: every output is summed
//   in one fixed order whatever MP, the grid or the batch are.
//   One workgroup per CU, i.e. one wave per SIMD: the launch reserves plan.h kF32mLds bytes of LDS it never touches.  Measured
//   (profiles/f32m_workgroups_per_cu_ab.txt): at B = 256 x 224^2 the 3x3 convs run at 34 - 46 % of the instruction's
//   peak with two workgroups per CU and at 67 - 74 % with one.
//   Epilogue: accumulators start at the folded-BN bias; a lane ends with 16 consecutive channels of its pixel -> residual in by
//   16-byte loads, ReLU, 16-byte NHWC stores into the interior only; pixels past B Ho Wo are clamped in the loop and masked here.
//   Split-K (engine option f32m_ksplit, plan.h f32m_ksplit(); small batches): the SPLIT variant of the same kernel runs
//   S workgroups per tile.  Workgroup (tile, share) walks the K steps [floor(share n / S), floor((share + 1) n / S)) of the n steps
//   (plan.h f32m_share_begin) with accumulators that start at +0.0f, and stores its raw float32 sums to a workspace laid out
//   [share][m][Cout].  conv_f32m_finalize_kernel, a second launch ordered behind it on the stream, computes per output element
//       v = bias;  v += part[0];  v += part[1];  ...  v += part[S - 1];  v += residual;  v = max(v, 0)
//   with plain float adds in exactly this order.  THAT ORDER IS THE DEFINITION OF THE MODE'S ARITHMETIC (the host walk of
//   tests/host_harness/harness_f32m_ksplit.cpp restates it): a result depends on S -- which the planner derives from the batch --
//   and on nothing else: not on MP, the grid, the pixel's position or what else is in the batch.  No atomics, no protocol between
//   workgroups.
#include "../../include/flope_amd.h"
#include "common.h"
#include "plan.h"

template <int MP, bool STEM, bool SPLIT = false>
__global__ __launch_bounds__(256) void conv_f32m_kernel(const F32mConvP p) {
  static_assert(!(STEM && SPLIT), "the stem (13 steps) is never split");
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kq = lane >> 4, c16 = lane & 15;
  const int nblk = p.Cout >> 6;
  unsigned tile = blockIdx.x;
  int share = 0;
  if (SPLIT) { tile = blockIdx.x / (unsigned)p.ksplit; share = blockIdx.x - tile * p.ksplit; }
  const int mtile = tile / nblk, blk = tile - mtile * nblk;
  const int m0 = (mtile * 4 + wave) * (16 * MP);
  if (m0 >= p.M) return;                                   // (no barrier below)
  const int HoWo = p.Ho * p.Wo;
  // this lane's pixel of each of the MP pixel tiles: pointer to channel 4 kq of tap (0, 0)
  const float* xp[MP];
#pragma unroll
  for (int t = 0; t < MP; ++t) {
    const int m = min(m0 + t * 16 + c16, p.M - 1);
    const int b = fastdiv(m, p.mg_hw, p.sh_hw), r = m - b * HoWo;
    const int ho = fastdiv(r, p.mg_w, p.sh_w), wo = r - ho * p.Wo;
    xp[t] = p.in + (((size_t)b * p.Hip + ho * p.stride + p.in_off) * p.Wip + wo * p.stride + p.in_off) * p.Cin_stored + (STEM ? 0 : 4 * kq);
  }
  const f32x4* const wb = (const f32x4*)p.w + (size_t)blk * p.nsteps * 256 + lane;
  f32x4 acc[MP][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const f32x4 b = SPLIT ? f32x4{0.f, 0.f, 0.f, 0.f} : *(const f32x4*)(p.bias + blk * 64 + kq * 16 + ct * 4);
#pragma unroll
    for (int t = 0; t < MP; ++t) acc[t][ct] = b;
  }
  // this workgroup's K steps [k0, nsteps): all of them, or its share
  const int k0 = SPLIT ? flope_plan::f32m_share_begin(p.nsteps, p.ksplit, share) : 0;
  const int nsteps = SPLIT ? flope_plan::f32m_share_begin(p.nsteps, p.ksplit, share + 1) : p.nsteps;
  // operand loads of the K steps in order (the tap walk is wave-uniform; a share enters it at its first step)
  int ky = 0, kx = 0, cs = 0;
  if (SPLIT) {
    const int tap = k0 / p.csteps;
    cs = k0 - tap * p.csteps; ky = tap / p.KW; kx = tap - ky * p.KW;
  }
  auto load = [&](int ks, f32x4 (&x)[MP], f32x4 (&w)[4]) {
    int off;
    if (STEM) {
      const int tap = min(ks * 4 + kq, p.KH * p.KW - 1), ty = tap / 7;
      off = (ty * p.Wip + tap - ty * 7) * 4;
    } else {
      off = (ky * p.Wip + kx) * p.Cin_stored + cs * 16;
      if (++cs == p.csteps) { cs = 0; if (++kx == p.KW) { kx = 0; ++ky; } }
    }
#pragma unroll
    for (int t = 0; t < MP; ++t) x[t] = *(const f32x4*)(xp[t] + off);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) w[ct] = wb[(ks * 4 + ct) * 64];
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
  // (no load of the loop is conditional: the compiler then counts the loads in flight and waits for the older step's only --
  // behind a conditional load it waits for every load, the step just issued included)
  load(k0, xa, wa);
  int ks = k0;
  for (; ks + 2 < nsteps; ks += 2) {
    load(ks + 1, xb, wc);
    __builtin_amdgcn_sched_barrier(0);                     // (the scheduler otherwise sinks the loads behind the MFMAs they are meant to run under)
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
  // lane (kq, c16): pixel c16 of each tile x channels 64 blk + 16 kq + 4 ct + q
#pragma unroll
  for (int t = 0; t < MP; ++t) {
    const int m = m0 + t * 16 + c16;
    if (m >= p.M) continue;
    if (SPLIT) {                                           // raw partial sums -> split_ws[share][m][Cout]
      float* const wp = p.split_ws + ((size_t)share * p.M + m) * p.Cout + blk * 64 + kq * 16;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) *(f32x4*)(wp + ct * 4) = acc[t][ct];
      continue;
    }
    const int b = fastdiv(m, p.mg_hw, p.sh_hw), r = m - b * HoWo;
    const int ho = fastdiv(r, p.mg_w, p.sh_w), wo = r - ho * p.Wo;
    const size_t o = (((size_t)b * p.Hop + ho + 1) * p.Wop + wo + 1) * p.Cout + blk * 64 + kq * 16;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      f32x4 v = acc[t][ct];
      if (p.res) {
        const f32x4 rv = *(const f32x4*)(p.res + o + ct * 4);
        v[0] += rv[0]; v[1] += rv[1]; v[2] += rv[2]; v[3] += rv[3];
      }
      if (p.relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
      *(f32x4*)(p.out + o + ct * 4) = v;
    }
  }
}

// split-K, second launch: one thread = four consecutive channels of one pixel.  v = bias, + the S partial sums in ascending share
// order, + residual, ReLU -- plain float adds in this order (the file header); 16-byte loads, 16-byte NHWC stores into the interior
// only (m < M: the zero ring is never written).
__global__ __launch_bounds__(256) void conv_f32m_finalize_kernel(const F32mConvP p) {
  const int c4 = p.Cout >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int m = idx / c4, c = (idx - m * c4) * 4;
  if (m >= p.M) return;
  f32x4 v = *(const f32x4*)(p.bias + c);
  const float* part = p.split_ws + (size_t)m * p.Cout + c;
  const size_t pitch = (size_t)p.M * p.Cout;
  for (int s = 0; s < p.ksplit; ++s) {
    const f32x4 a = *(const f32x4*)(part + s * pitch);
    v[0] += a[0]; v[1] += a[1]; v[2] += a[2]; v[3] += a[3];
  }
  const int b = fastdiv(m, p.mg_hw, p.sh_hw), r = m - b * p.Ho * p.Wo;
  const int ho = fastdiv(r, p.mg_w, p.sh_w), wo = r - ho * p.Wo;
  const size_t o = (((size_t)b * p.Hop + ho + 1) * p.Wop + wo + 1) * p.Cout + c;
  if (p.res) {
    const f32x4 rv = *(const f32x4*)(p.res + o);
    v[0] += rv[0]; v[1] += rv[1]; v[2] += rv[2]; v[3] += rv[3];
  }
  if (p.relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
  *(f32x4*)(p.out + o) = v;
}

extern "C" int flope_conv_f32m_init() {
  const void* const k[9] = {(const void*)conv_f32m_kernel<4, true>,  (const void*)conv_f32m_kernel<2, true>,  (const void*)conv_f32m_kernel<1, true>,
                            (const void*)conv_f32m_kernel<4, false>, (const void*)conv_f32m_kernel<2, false>, (const void*)conv_f32m_kernel<1, false>,
                            (const void*)conv_f32m_kernel<4, false, true>, (const void*)conv_f32m_kernel<2, false, true>,
                            (const void*)conv_f32m_kernel<1, false, true>};
  for (const void* f : k) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// mp: pixel tiles per wave (1, 2 or 4; plan.h f32m_mp), lds: bytes reserved.  p->ksplit <= 1: grid = tiles = ceil(M / (64 mp)) * Cout / 64
// workgroups.  p->ksplit = S in 2..32 (never the stem): grid = tiles * S workgroups of the split variant, then the finalize launch on
// the same stream; p->split_ws holds ws_bytes >= S * M * Cout floats and every share has at least one step.
extern "C" int flope_conv_f32m_launch(const F32mConvP* p, int mp, int stem, int grid, size_t lds, size_t ws_bytes, void* stream) {
  const bool shape_ok = p->Cout % 64 == 0 && p->M == p->B * p->Ho * p->Wo && p->M >= 1 &&
                        (stem ? (p->Cin_stored == 4 && p->KH == 7 && p->KW == 7 && p->nsteps == 13 && p->Cout == 64)
                              : (p->Cin_stored == p->Cin && p->Cin % 16 == 0 && p->csteps == p->Cin / 16 && p->nsteps == p->KH * p->KW * p->csteps));
  const int S = p->ksplit > 1 ? p->ksplit : 1;
  const int tiles = (p->M + 64 * mp - 1) / (64 * mp) * (p->Cout / 64);
  if (!shape_ok || lds > 160 * 1024 || (mp != 1 && mp != 2 && mp != 4) || grid != tiles * S) return (int)hipErrorInvalidValue;
  if (S > 1 && (stem || S > flope_plan::kF32mMaxSplit || p->nsteps / S < 1 || !p->split_ws ||
                (size_t)S * p->M * p->Cout * sizeof(float) > ws_bytes))
    return (int)hipErrorInvalidValue;
  const dim3 g(grid), b(256);
  hipStream_t st = (hipStream_t)stream;
  if (S > 1) {
    if (mp == 4) hipLaunchKernelGGL((conv_f32m_kernel<4, false, true>), g, b, lds, st, *p);
    else if (mp == 2) hipLaunchKernelGGL((conv_f32m_kernel<2, false, true>), g, b, lds, st, *p);
    else hipLaunchKernelGGL((conv_f32m_kernel<1, false, true>), g, b, lds, st, *p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const long quads = (long)p->M * (p->Cout / 4);
    hipLaunchKernelGGL(conv_f32m_finalize_kernel, dim3((unsigned)((quads + 255) / 256)), b, 0, st, *p);
    return (int)hipGetLastError();
  }
  if (stem) {    if (mp == 4) hipLaunchKernelGGL((conv_f32m_kernel<4, true>), g, b, lds, st, *p);
    else if (mp == 2) hipLaunchKernelGGL((conv_f32m_kernel<2, true>), g, b, lds, st, *p);
    else hipLaunchKernelGGL((conv_f32m_kernel<1, true>), g, b, lds, st, *p);
  } else {
    if (mp == 4) hipLaunchKernelGGL((conv_f32m_kernel<4, false>), g, b, lds, st, *p);
    else if (mp == 2) hipLaunchKernelGGL((conv_f32m_kernel<2, false>), g, b, lds, st, *p);
    else hipLaunchKernelGGL((conv_f32m_kernel<1, false>), g, b, lds, st, *p);
  }
  return (int)hipGetLastError();
}
