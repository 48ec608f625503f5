// CPU-only test harness of the encoder's single-launch forward (option fused; flope_amd/csrc/tf_fused_plan.h): the
// planner functions as tf_encoder.hip calls them, the buffers that are live in each phase of tf_fused_f32, and a scalar walk of that
// kernel over an emulated LDS -- the same phase order, the same offsets and aliasing, the same summation orders (fmaf chains, 64 lanes
// with an xor butterfly), std::exp for the device's expf.  Every LDS access is checked against layout.total and every global access
// against its array; the walk counts violations instead of aborting.  A rehearsal that catches a wrong alias or offset before a GPU
// run, not a bit oracle.  tests/test_tf_fused_host.py.  Not part of the product.
#include "tf_fused_plan.h"

#include <cmath>
#include <limits>
#include <vector>

using flope_tf_plan::TfFusedLayout;

namespace {

enum { B_H, B_H2, B_X, B_QKV, B_ATT, B_SC, B_FFB, B_COUNT };
// phases of one forward: load, embedding, then per layer in_proj, attention, out_proj, norm1, linear1, linear2, norm2, then out_layer
enum { P_LOAD, P_EMB, P_INPROJ, P_ATTN, P_OUTPROJ, P_LN1, P_LIN1, P_LIN2, P_LN2, P_OUT, P_COUNT };
#define M_(b) (1 << (b))
// WRITTEN BY HAND from the phases of tf_fused_f32 (tf_encoder.hip), not derived from the walk below: keep it in step with the kernel.
// buffers whose contents a phase reads, writes, or must find unchanged afterwards (h carries the residual across the attention
// and the feed-forward halves)
const int kLive[P_COUNT] = {
    M_(B_X),                                        // load
    M_(B_X) | M_(B_H),                              // embedding
    M_(B_H) | M_(B_QKV),                            // in_proj
    M_(B_H) | M_(B_QKV) | M_(B_ATT) | M_(B_SC),     // attention
    M_(B_H) | M_(B_ATT) | M_(B_H2),                 // out_proj + residual
    M_(B_H2) | M_(B_H),                             // norm1
    M_(B_H) | M_(B_FFB),                            // linear1
    M_(B_H) | M_(B_FFB) | M_(B_H2),                 // linear2 + residual
    M_(B_H2) | M_(B_H),                             // norm2
    M_(B_H),                                        // out_layer
};

struct Walk {
  std::vector<float> lds;
  long bad = 0;
  float dummy = 0.f;
  float& at(uint32_t base, long idx) {              // float idx of the buffer at byte offset base
    const long byte = (long)base + idx * 4;
    if (idx < 0 || byte < 0 || byte + 4 > (long)lds.size() * 4) { ++bad; dummy = std::numeric_limits<float>::quiet_NaN(); return dummy; }
    return lds[byte / 4];
  }
};
struct Arr {                                        // a global array with its element count
  const float* p; long n; long* bad;
  float operator[](long i) const { if (i < 0 || i >= n) { ++*bad; return std::numeric_limits<float>::quiet_NaN(); } return p[i]; }
};

float butterfly_sum(float* v) {                     // wave_sum: every lane ends with the same value; lane 0's is returned
  for (int o = 32; o > 0; o >>= 1) { float t[64]; for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ o]; for (int l = 0; l < 64; ++l) v[l] = t[l]; }
  return v[0];
}
float butterfly_max(float* v) {
  for (int o = 32; o > 0; o >>= 1) { float t[64]; for (int l = 0; l < 64; ++l) t[l] = std::fmax(v[l], v[l ^ o]); for (int l = 0; l < 64; ++l) v[l] = t[l]; }
  return v[0];
}

// Y = act(X W^T + b (+ R)); X, R in LDS; Y in LDS (yg == nullptr) or from float y0 on in the global array yg of yn floats
void linear(Walk& w, uint32_t X, int xld, const Arr& W, const Arr& b, bool has_r, uint32_t R, int rld, uint32_t Y, int yld, float* yg, long yn,
            long y0, int M, int K, int N, int relu) {
  auto store = [&](long i, float v) {
    if (!yg) { w.at(Y, i) = v; return; }
    if (i < 0 || y0 + i < 0 || y0 + i >= yn) { ++w.bad; return; }
    yg[y0 + i] = v;
  };
  const bool rowwave = flope_tf_plan::tf_fused_rowwave_order(N, has_r);
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) {
      float acc;
      if (rowwave) {
        float lane[64];
        for (int l = 0; l < 64; ++l) {
          lane[l] = 0.f;
          for (int k = l; k < K; k += 64) lane[l] = std::fmaf(w.at(X, (long)m * xld + k), W[(long)n * K + k], lane[l]);
        }
        acc = butterfly_sum(lane) + b[n];
      } else {
        acc = 0.f;
        for (int k = 0; k < K; ++k) acc = std::fmaf(w.at(X, (long)m * xld + k), W[(long)n * K + k], acc);
        acc += b[n];
        if (has_r) acc += w.at(R, (long)m * rld + n);
      }
      if (relu) acc = std::fmax(acc, 0.f);
      store((long)m * yld + n, acc);
    }
}

void layernorm(Walk& w, uint32_t in, uint32_t out, const Arr& g, const Arr& be, int M, int d) {
  for (int row = 0; row < M; ++row) {
    float lane[64];
    for (int l = 0; l < 64; ++l) { lane[l] = 0.f; for (int c = l; c < d; c += 64) lane[l] += w.at(in, (long)row * d + c); }
    const float mean = butterfly_sum(lane) / d;
    for (int l = 0; l < 64; ++l) {
      lane[l] = 0.f;
      for (int c = l; c < d; c += 64) { const float t = w.at(in, (long)row * d + c) - mean; lane[l] = std::fmaf(t, t, lane[l]); }
    }
    const float rstd = 1.f / std::sqrt(butterfly_sum(lane) / d + 1e-5f);
    for (int c = 0; c < d; ++c) w.at(out, (long)row * d + c) = (w.at(in, (long)row * d + c) - mean) * rstd * g[c] + be[c];
  }
}

void attention(Walk& w, const TfFusedLayout& lay, int L, int d, int H) {
  const int dh = d / H, qld = (int)lay.qkv_ld;
  const float scale = 1.f / std::sqrt((float)dh);
  for (int it = 0; it < H * L; ++it) {
    const int wave = it % flope_tf_plan::kTfFusedWaves, h = it / L, i = it - h * L;
    const long s = (long)wave * lay.sc_ld, base = (long)h * dh;
    float lane[64];
    for (int l = 0; l < 64; ++l) {
      lane[l] = -std::numeric_limits<float>::infinity();
      for (int j = l; j < L; j += 64) {
        float a = 0.f;
        for (int c = 0; c < dh; ++c) a = std::fmaf(w.at(lay.qkv, base + (long)i * qld + c), w.at(lay.qkv, base + (long)j * qld + d + c), a);
        a *= scale;
        w.at(lay.sc, s + j) = a;
        lane[l] = std::fmax(lane[l], a);
      }
    }
    const float mx = butterfly_max(lane);
    for (int l = 0; l < 64; ++l) {
      lane[l] = 0.f;
      for (int j = l; j < L; j += 64) { const float p = std::exp(w.at(lay.sc, s + j) - mx); w.at(lay.sc, s + j) = p; lane[l] += p; }
    }
    const float inv = 1.f / butterfly_sum(lane);
    for (int c = 0; c < dh; ++c) {
      float o = 0.f;
      for (int j = 0; j < L; ++j) o = std::fmaf(w.at(lay.sc, s + j), w.at(lay.qkv, base + (long)j * qld + 2 * d + c), o);
      w.at(lay.att, (long)i * d + h * dh + c) = o * inv;
    }
  }
}

}  // namespace

extern "C" {

long tf_fused_lds_limit() { return (long)flope_tf_plan::kTfFusedLds; }
int tf_fused_waves() { return flope_tf_plan::kTfFusedWaves; }

// out10: {h, h2, x, qkv, att, sc, ffb (byte offsets), qkv_ld, sc_ld (floats), total (bytes)}
void tf_fused_layout(int in_dim, int d, int ff, int L, long* out10) {
  const TfFusedLayout l = flope_tf_plan::tf_fused_layout(in_dim, d, ff, L);
  const long v[10] = {l.h, l.h2, l.x, l.qkv, l.att, l.sc, l.ffb, l.qkv_ld, l.sc_ld, (long)l.total};
  for (int i = 0; i < 10; ++i) out10[i] = v[i];
}

// out7: bytes the kernel uses of each buffer, in the order of the offsets above
void tf_fused_buffer_bytes(int in_dim, int d, int ff, int L, long* out7) {
  const TfFusedLayout l = flope_tf_plan::tf_fused_layout(in_dim, d, ff, L);
  const long v[7] = {(long)L * d, (long)L * d, (long)L * in_dim, (long)L * l.qkv_ld, (long)L * d, (long)flope_tf_plan::kTfFusedWaves * l.sc_ld, (long)L * ff};
  for (int i = 0; i < 7; ++i) out7[i] = v[i] * 4;
}

int tf_fused_phases() { return P_COUNT; }
// bit i set: buffer i (the order above) is live in this phase
int tf_fused_live(int phase) { return phase >= 0 && phase < P_COUNT ? kLive[phase] : -1; }

int tf_fused_rowwave_order(int N, int has_residual) { return flope_tf_plan::tf_fused_rowwave_order(N, has_residual) ? 1 : 0; }
int tf_fused_ok(int dtype, int opt_fused, int opt_f32m, int in_dim, int d, int ff, int L) {
  return flope_tf_plan::tf_fused_ok(dtype, opt_fused, opt_f32m, in_dim, d, ff, L) ? 1 : 0;
}

// The fused forward of x [B][L][in_dim] -> y [B][L][out_dim].  lengths: B ints or NULL (every sequence has L tokens).
// tab / tab_n: the kernel's pointer table (4 + 12 nl host arrays) and the element count of each.  Returns the number of index
// violations (0 = clean), -1 for a shape that is not eligible, -2 for a bad length.
long tf_fused_walk(const float* x, float* y, const int* lengths, int B, int L, int in_dim, int d, int out_dim, int H, int nl, int ff,
                   const float* const* tab, const long* tab_n) {
  int Lmax = L;
  std::vector<int> off((size_t)B + 1, 0);
  if (lengths) {
    Lmax = 0;
    for (int b = 0; b < B; ++b) {
      if (lengths[b] < 1 || lengths[b] > L) return -2;
      off[b + 1] = off[b] + lengths[b];
      if (lengths[b] > Lmax) Lmax = lengths[b];
    }
  }
  if (!flope_tf_plan::tf_fused_ok(FLOPE_DT_F32, 1, 0, in_dim, d, ff, Lmax)) return -1;
  const TfFusedLayout lay = flope_tf_plan::tf_fused_layout(in_dim, d, ff, Lmax);
  Walk w;
  auto arr = [&](int i) { return Arr{tab[i], tab_n[i], &w.bad}; };
  const long xn = (long)B * L * in_dim, yn = (long)B * L * out_dim;
  const Arr X{x, xn, &w.bad};
  for (int b = 0; b < B; ++b) {                          // one workgroup each: fresh LDS, nothing carried over
    w.lds.assign((size_t)(lay.total / 4), std::numeric_limits<float>::quiet_NaN());
    const int len = lengths ? off[b + 1] - off[b] : L;
    const long xb = (long)b * L * in_dim, yb = (long)b * L * out_dim;
    for (long i = 0; i < (long)len * in_dim; ++i) w.at(lay.x, i) = X[xb + i];
    linear(w, lay.x, in_dim, arr(0), arr(1), false, 0, 0, lay.h, d, nullptr, 0, 0, len, in_dim, d, 0);
    for (int l = 0; l < nl; ++l) {
      const int t = 4 + 12 * l;
      linear(w, lay.h, d, arr(t), arr(t + 1), false, 0, 0, lay.qkv, (int)lay.qkv_ld, nullptr, 0, 0, len, d, 3 * d, 0);
      attention(w, lay, len, d, H);
      linear(w, lay.att, d, arr(t + 2), arr(t + 3), true, lay.h, d, lay.h2, d, nullptr, 0, 0, len, d, d, 0);
      layernorm(w, lay.h2, lay.h, arr(t + 8), arr(t + 9), len, d);
      linear(w, lay.h, d, arr(t + 4), arr(t + 5), false, 0, 0, lay.ffb, ff, nullptr, 0, 0, len, d, ff, 1);
      linear(w, lay.ffb, ff, arr(t + 6), arr(t + 7), true, lay.h, d, lay.h2, d, nullptr, 0, 0, len, ff, d, 0);
      layernorm(w, lay.h2, lay.h, arr(t + 10), arr(t + 11), len, d);
    }
    {                                                    // out_layer straight to y, then the rows behind the sequence
      const Arr bo = arr(3);
      linear(w, lay.h, d, arr(2), bo, false, 0, 0, 0, out_dim, y, yn, yb, len, d, out_dim, 0);
      for (long i = 0; i < (long)(L - len) * out_dim; ++i) {
        const long g = yb + (long)len * out_dim + i;
        if (g < 0 || g >= yn) ++w.bad; else y[g] = bo[i % out_dim];
      }
    }
  }
  return w.bad;
}

}  // extern "C"
