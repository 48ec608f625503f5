// CPU-only test harness of the float32 MFMA encoder linear (tf_linear_f32m, flope_amd/csrc/tf_encoder.hip): the weight packer of
// host_pack.h and a scalar walk of the kernel's operand feed -- which float every lane loads for which MFMA of which K step, from
// the packed image and the row-major tokens -- so that packer, row permutation, padding and epilogue masking are checked against
// fp64 without a GPU (tests/test_tf_f32m_host.py), and the device output against this walk bit for bit
// (tests/test_gpu_tf_f32m.py).  Not part of the product.
#include "host_pack.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

extern "C" {

long tf_f32m_image_floats(int N, int K) { return (long)flope_host::tf_f32m_floats(N, K); }

void tf_f32m_pack(const float* w, int N, int K, float* dst) {
  const std::vector<float> p = flope_host::pack_tf_f32m(w, N, K);
  memcpy(dst, p.data(), p.size() * sizeof(float));
}

// the tile height a launch picks (host_pack.h tf_f32m_mp)
int tf_f32m_plan_mp(int M, int N, int slots) { return flope_host::tf_f32m_mp(M, N, slots); }

// One linear as the kernel computes it, lane by lane.  X [M][K] (K % 4 == 0), wimg: the packed image, bias [N], R / Y [M][N], mp: token
// tiles per wave.  Per workgroup (token tile of 64 mp, feature block), wave, token tile t, feature tile ct, K step ks, MFMA s:
//   D[i][j] += sum over kq of A[i][kq] B[kq][j],  A = float s of lane (kq, i)'s weight load, B = float s of lane (kq, j)'s token load,
// an fmaf chain over kq = 0..3 in float, started at the bias; then residual, then ReLU.  Returns 0, or a positive code when an index
// leaves its buffer.
int tf_f32m_walk(const float* X, const float* wimg, const float* bias, const float* R, float* Y, int M, int K, int N, int relu, int mp) {
  if (K < 4 || K % 4 || M < 1 || N < 1) return 9;
  const int nsteps = flope_host::tf_f32m_steps(K), nblk = (N + 63) / 64;
  const long w_n = (long)flope_host::tf_f32m_floats(N, K), x_n = (long)M * K, y_n = (long)M * N;
  std::vector<float> bp((size_t)nblk * 64, 0.f);
  memcpy(bp.data(), bias, (size_t)N * sizeof(float));
  const int mtiles = (M + 64 * mp - 1) / (64 * mp);
  for (int mtile = 0; mtile < mtiles; ++mtile)
    for (int blk = 0; blk < nblk; ++blk)
      for (int wave = 0; wave < 4; ++wave) {
        const int m0 = (mtile * 4 + wave) * 16 * mp;
        if (m0 >= M) continue;
        const int nct = std::min(4, (N + 15) / 16 - blk * 4);
        for (int t = 0; t < mp; ++t)
          for (int ct = 0; ct < nct; ++ct) {                // (tiles nct .. 3 of the kernel repeat tile nct - 1 and are not stored)
            float acc[16][16];                             // [row i][token j]
            for (int i = 0; i < 16; ++i)
              for (int j = 0; j < 16; ++j) acc[i][j] = bp[flope_host::tf_f32m_feature(blk, nct, ct, i)];
            for (int ks = 0; ks < nsteps; ++ks)
              for (int s = 0; s < 4; ++s)
                for (int i = 0; i < 16; ++i)
                  for (int j = 0; j < 16; ++j)
                    for (int kq = 0; kq < 4; ++kq) {
                      const long wi = ((((long)blk * nsteps * 4 + (long)ks * nct + ct) * 64) + kq * 16 + i) * 4 + s;
                      const long xi = (long)std::min(m0 + t * 16 + j, M - 1) * K + std::min(ks * 16 + 4 * kq, K - 4) + s;
                      if (wi < 0 || wi >= w_n) return 1;
                      if (xi < 0 || xi >= x_n) return 2;
                      acc[i][j] = fmaf(wimg[wi], X[xi], acc[i][j]);
                    }
            for (int j = 0; j < 16; ++j) {
              const int m = m0 + t * 16 + j;
              if (m >= M) continue;
              for (int i = 0; i < 16; ++i) {
                const int f = flope_host::tf_f32m_feature(blk, nct, ct, i);
                if (f >= N) continue;
                const long o = (long)m * N + f;
                if (o < 0 || o >= y_n) return 3;
                float v = acc[i][j];
                if (R) v += R[o];
                if (relu) v = fmaxf(v, 0.f);
                Y[o] = v;
              }
            }
          }
      }
  return 0;
}

}  // extern "C"
