// CPU-only test harness of the split-K form of the float32 MFMA trunk (engine option f32m_ksplit; flope_amd/csrc/conv_f32m.hip,
// plan.h f32m_ksplit): the planner's helpers, and a scalar walk of the split kernel plus conv_f32m_finalize_kernel over the packed
// weight image -- every share an fmaf chain from +0 over its own K steps in the kernel's operand order, raw sums to a workspace
// laid out [share][m][Cout], then bias + share 0 + share 1 + ... + residual, ReLU (tests/test_f32m_ksplit_host.py).  Linked with
// harness_f32m.cpp, whose f32m_walk is the unsplit kernel: S = 1 IS that walk.  Not part of the product.
#include "host_pack.h"
#include "plan.h"

#include <math.h>

#include <algorithm>

extern "C" {

int f32m_walk(const float* in, const float* wimg, const float* bias, const float* res, float* out, int B, int Hip, int Wip, int cin_stored,
              int cin, int Ho, int Wo, int cout, int k, int stride, int in_off, int relu, int stem, int mp);

int f32m_ksplit_plan(int option, int total_tiles, int mp, int nsteps, int plan_slices, int cus) {
  return flope_plan::f32m_ksplit(option, total_tiles, mp, nsteps, plan_slices, cus);
}
int f32m_ksplit_share_begin(int nsteps, int S, int share) { return flope_plan::f32m_share_begin(nsteps, S, share); }
int f32m_ksplit_min_share_steps() { return flope_plan::kF32mMinShareSteps; }
long f32m_ksplit_ws_bytes(int cus) { return (long)flope_plan::f32m_ws_bytes(cus); }

// One conv as a split launch of S shares + the finalize launch compute it.  Tensors as f32m_walk (harness_f32m.cpp); ws: ws_floats
// floats of workspace, filled with the caller's pattern (elements no share owns stay as they were).  Returns 0, or a positive code
// when an index leaves its buffer (1 weights, 2 input, 3 workspace written, 4 workspace read) or a share is empty (5).
int f32m_ksplit_walk(const float* in, const float* wimg, const float* bias, const float* res, float* out, float* ws, long ws_floats, int B,
                     int Hip, int Wip, int cin, int Ho, int Wo, int cout, int k, int stride, int in_off, int relu, int mp, int S) {
  if (S <= 1) return f32m_walk(in, wimg, bias, res, out, B, Hip, Wip, cin, cin, Ho, Wo, cout, k, stride, in_off, relu, 0, mp);
  const int M = B * Ho * Wo, HoWo = Ho * Wo, Hop = Ho + 2, Wop = Wo + 2, nblk = cout / 64;
  const int n = flope_host::f32m_steps(cin, k), csteps = cin / 16;
  const long in_n = (long)B * Hip * Wip * cin, w_n = (long)cout * n * 16;
  const int mtiles = (M + 64 * mp - 1) / (64 * mp);
  // ---- the split launch: workgroup = (tile, share), tile = (mtile, blk) ----
  for (int wg = 0; wg < mtiles * nblk * S; ++wg) {
    const int tile = wg / S, share = wg - tile * S, mtile = tile / nblk, blk = tile - mtile * nblk;
    const int k0 = flope_plan::f32m_share_begin(n, S, share), k1 = flope_plan::f32m_share_begin(n, S, share + 1);
    if (k1 <= k0) return 5;
    for (int wave = 0; wave < 4; ++wave) {
      const int m0 = (mtile * 4 + wave) * 16 * mp;
      if (m0 >= M) continue;
      for (int t = 0; t < mp; ++t) {
        long xp[16];
        for (int j = 0; j < 16; ++j) {
          const int m = std::min(m0 + t * 16 + j, M - 1), b = m / HoWo, r = m % HoWo, ho = r / Wo, wo = r % Wo;
          xp[j] = (((long)b * Hip + ho * stride + in_off) * Wip + wo * stride + in_off) * cin;
        }
        for (int ct = 0; ct < 4; ++ct) {
          float acc[16][16];                               // [row i][pixel j], from +0
          for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j) acc[i][j] = 0.f;
          // the share enters the tap walk at its first step by scalar arithmetic
          const int tap0 = k0 / csteps;
          int cs = k0 % csteps, ky = tap0 / k, kx = tap0 % k;
          for (int ks = k0; ks < k1; ++ks) {
            long off[4];
            for (int kq = 0; kq < 4; ++kq) off[kq] = ((long)ky * Wip + kx) * cin + cs * 16 + 4 * kq;
            if (++cs == csteps) { cs = 0; if (++kx == k) { kx = 0; ++ky; } }
            for (int s = 0; s < 4; ++s)
              for (int i = 0; i < 16; ++i)
                for (int j = 0; j < 16; ++j)
                  for (int kq = 0; kq < 4; ++kq) {
                    const long wi = ((((long)blk * n + ks) * 4 + ct) * 64 + kq * 16 + i) * 4 + s, xi = xp[j] + off[kq] + s;
                    if (wi < 0 || wi >= w_n) return 1;
                    if (xi < 0 || xi >= in_n) return 2;
                    acc[i][j] = fmaf(wimg[wi], in[xi], acc[i][j]);
                  }
          }
          for (int j = 0; j < 16; ++j) {
            const int m = m0 + t * 16 + j;
            if (m >= M) continue;
            for (int i = 0; i < 16; ++i) {
              const long o = ((long)share * M + m) * cout + blk * 64 + (i >> 2) * 16 + ct * 4 + (i & 3);
              if (o < 0 || o >= ws_floats) return 3;
              ws[o] = acc[i][j];
            }
          }
        }
      }
    }
  }
  // ---- the finalize launch: one thread = four channels of one pixel; the adds in this order define the mode ----
  for (long idx = 0; idx < (long)M * (cout / 4); ++idx) {
    const int m = (int)(idx / (cout / 4)), c = (int)(idx % (cout / 4)) * 4;
    const int b = m / HoWo, r = m % HoWo, ho = r / Wo, wo = r % Wo;
    const long o = (((long)b * Hop + ho + 1) * Wop + wo + 1) * cout + c;
    for (int q = 0; q < 4; ++q) {
      float v = bias[c + q];
      for (int s = 0; s < S; ++s) {
        const long wi = ((long)s * M + m) * cout + c + q;
        if (wi >= ws_floats) return 4;
        v += ws[wi];
      }
      if (res) v += res[o + q];
      if (relu) v = fmaxf(v, 0.f);
      out[o + q] = v;
    }
  }
  return 0;
}

}  // extern "C"
