// CPU-only test harness of the float32 MFMA trunk (flope_amd/csrc/conv_f32m.hip): the weight packers of host_pack.h and a scalar
// walk of the kernel's operand feed -- which float every lane loads for which MFMA of which K step, from the packed image and a
// zero-bordered NHWC input -- so that packer, tap walk, row permutation and epilogue addressing are checked against the fp64
// oracle without a GPU (tests/test_f32m_host.py).  Not part of the product.
#include "host_pack.h"
#include "plan.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

extern "C" {

long f32m_image_floats(int cout, int cin, int k) { return (long)cout * flope_host::f32m_steps(cin, k) * 16; }
long f32m_stem_image_floats() { return (long)64 * flope_host::kF32mStemSteps * 16; }

void f32m_pack(const float* w, int cout, int cin, int k, float* dst) {
  const std::vector<float> wf(w, w + (size_t)cout * cin * k * k);
  const std::vector<float> p = flope_host::pack_f32m(wf, cout, cin, k);
  memcpy(dst, p.data(), p.size() * sizeof(float));
}

void f32m_pack_stem(const float* w, float* dst) {
  const std::vector<float> wf(w, w + (size_t)64 * 3 * 7 * 7);
  const std::vector<float> p = flope_host::pack_f32m_stem(wf);
  memcpy(dst, p.data(), p.size() * sizeof(float));
}

// the tile height the planner picks (plan.h f32m_mp)
int f32m_plan_mp(int M, int cout, int cus) { return flope_plan::f32m_mp(M, cout, cus); }

// One conv as the kernel computes it, lane by lane.  in: [B][Hip][Wip][cin_stored], res / out: [B][Ho + 2][Wo + 2][cout] (out's ring
// is left as the caller filled it), wimg: the packed image, mp: pixel tiles per wave.  stem != 0: 7 x 7, 4 stored channels.
// Per workgroup (pixel tile of 64 mp, channel block), wave, K step ks, MFMA s, pixel tile t, channel tile ct:
//   D[i][j] += sum over kq of A[i][kq] B[kq][j],  A = float s of lane (kq, i)'s weight load, B = float s of lane (kq, j)'s input load,
// accumulated as an fmaf chain over kq = 0..3 in float.  Returns 0, or a positive code when an index leaves its buffer.
int f32m_walk(const float* in, const float* wimg, const float* bias, const float* res, float* out, int B, int Hip, int Wip, int cin_stored,
              int cin, int Ho, int Wo, int cout, int k, int stride, int in_off, int relu, int stem, int mp) {
  const int M = B * Ho * Wo, HoWo = Ho * Wo, Hop = Ho + 2, Wop = Wo + 2, nblk = cout / 64;
  const int nsteps = stem ? flope_host::kF32mStemSteps : flope_host::f32m_steps(cin, k), csteps = cin / 16;
  const long in_n = (long)B * Hip * Wip * cin_stored, w_n = (long)cout * nsteps * 16;
  const int mtiles = (M + 64 * mp - 1) / (64 * mp);
  for (int mtile = 0; mtile < mtiles; ++mtile)
    for (int blk = 0; blk < nblk; ++blk)
      for (int wave = 0; wave < 4; ++wave) {
        const int m0 = (mtile * 4 + wave) * 16 * mp;
        if (m0 >= M) continue;
        for (int t = 0; t < mp; ++t) {
          // per lane column j: the pixel's base offset (clamped past the end, as the kernel does)
          long xp[16];
          for (int j = 0; j < 16; ++j) {
            const int m = std::min(m0 + t * 16 + j, M - 1), b = m / HoWo, r = m % HoWo, ho = r / Wo, wo = r % Wo;
            xp[j] = (((long)b * Hip + ho * stride + in_off) * Wip + wo * stride + in_off) * cin_stored;
          }
          for (int ct = 0; ct < 4; ++ct) {
            float acc[16][16];                             // [row i][pixel j]
            for (int i = 0; i < 16; ++i)
              for (int j = 0; j < 16; ++j) acc[i][j] = bias[blk * 64 + (i >> 2) * 16 + ct * 4 + (i & 3)];
            int ky = 0, kx = 0, cs = 0;
            for (int ks = 0; ks < nsteps; ++ks) {
              long off[4];                                 // per kq: offset of the lane's 16-byte load from its pixel base
              for (int kq = 0; kq < 4; ++kq) {
                if (stem) {
                  const int tap = std::min(ks * 4 + kq, 48);
                  off[kq] = ((long)(tap / 7) * Wip + tap % 7) * 4;
                } else {
                  off[kq] = ((long)ky * Wip + kx) * cin_stored + cs * 16 + 4 * kq;
                }
              }
              if (!stem && ++cs == csteps) { cs = 0; if (++kx == k) { kx = 0; ++ky; } }
              for (int s = 0; s < 4; ++s)
                for (int i = 0; i < 16; ++i)
                  for (int j = 0; j < 16; ++j)
                    for (int kq = 0; kq < 4; ++kq) {
                      const long wi = ((((long)blk * nsteps + ks) * 4 + ct) * 64 + kq * 16 + i) * 4 + s, xi = xp[j] + off[kq] + s;
                      if (wi < 0 || wi >= w_n) return 1;
                      if (xi < 0 || xi >= in_n) return 2;
                      acc[i][j] = fmaf(wimg[wi], in[xi], acc[i][j]);
                    }
            }
            for (int j = 0; j < 16; ++j) {
              const int m = m0 + t * 16 + j;
              if (m >= M) continue;
              const int b = m / HoWo, r = m % HoWo, ho = r / Wo, wo = r % Wo;
              for (int i = 0; i < 16; ++i) {
                const long o = (((long)b * Hop + ho + 1) * Wop + wo + 1) * cout + blk * 64 + (i >> 2) * 16 + ct * 4 + (i & 3);
                float v = acc[i][j];
                if (res) v += res[o];
                if (relu) v = fmaxf(v, 0.f);
                out[o] = v;
              }
            }
          }
        }
      }
  return 0;
}

}  // extern "C"
