// CPU-only test harness of the planner of option "skinny_ln" (flope_amd/csrc/tf_skinny_plan.h, which tf_gemm_skinny_ln calls per lane;
// DESIGN.md 49): the eligibility rule, the summation order and the store of the post-norm rows.
//   rule    tf_skinny_ln_ok and tf_ln_vec_ok as they are;
//   order   one row of d 16-bit values, its sum and the sum of its squared deviations two ways, both in float32 from the same per-vector
//           partials (tf_layernorm_vec's: s from 0.f, s += lo + hi for q = 0 .. 3; v from 0.f, v = fmaf(a, a, fmaf(c, c, v))):
//             wave   tf_layernorm_vec's: lane c of 64 holds vector c (0.f past d / 8), wave_sum = += the lane at xor 32, 16, 8, 4, 2, 1;
//             lane   tf_gemm_skinny_ln's: lane group g holds vector tf_skinny_ln_vec(slot, g) in ring slot `slot`, the planner's in-lane tree
//                    (tf_skinny_ln_lane_tree), then += the lane group at xor tf_skinny_ln_lane_xor(0) >> 4 and (1) >> 4;
//           the caller compares the bit patterns.  Build with -ffp-contract=off: every product and sum rounds on its own, fmaf is fused;
//   cover   a walk of a whole launch (every wave, lane, token tile, ks): every 16 bytes of rows 0 .. 16 MT - 1 of H are stored exactly
//           once, nothing outside them (the stores are made, into a buffer of exactly that size, so a sanitizer build sees one that is
//           not), a lane stores where it loaded, its vector index and gamma / beta column are those of that load.
// Not part of the product.  With -DTF_SKINNY_LN_MAIN the file is a program of its own (built under -fsanitize=address,undefined by the
// test and run as a child process) that runs every shape of the test.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "tf_skinny_plan.h"

using namespace flope_tf_plan;

namespace {

float f16_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000) << 16, em = h & 0x7fff;
  uint32_t bits;
  if (em >= 0x7c00) bits = sign | 0x7f800000u | ((em & 0x3ff) << 13);          // inf / NaN
  else if (em >= 0x0400) bits = sign | ((em << 13) + (112u << 23));             // normal
  else {                                                                        // zero / subnormal: em 2^-24, exact in float32
    const float v = (float)em * 5.9604644775390625e-8f;
    uint32_t b;
    memcpy(&b, &v, 4);
    bits = sign | b;
  }
  float f;
  memcpy(&f, &bits, 4);
  return f;
}
float bf16_to_f32(uint16_t h) {
  const uint32_t bits = (uint32_t)h << 16;
  float f;
  memcpy(&f, &bits, 4);
  return f;
}
uint32_t bits_of(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

// the per-vector partials of tf_layernorm_vec (tf_ln_vec_sum / tf_ln_vec_sq of tf_encoder.hip, restated: element 2 q is lo, 2 q + 1 hi)
float vec_sum(const float* e) {
  float s = 0.f;
  for (int q = 0; q < 4; ++q) s += e[2 * q] + e[2 * q + 1];
  return s;
}
float vec_sq(const float* e, float mean) {
  float v = 0.f;
  for (int q = 0; q < 4; ++q) {
    const float a = e[2 * q] - mean, c = e[2 * q + 1] - mean;
    v = fmaf(a, a, fmaf(c, c, v));
  }
  return v;
}

// wave_sum over 64 lanes: every lane ends with the same value; lane 0's
float wave_sum64(const float* lane_val) {
  float v[64], t[64];
  memcpy(v, lane_val, sizeof v);
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ o];
    memcpy(v, t, sizeof v);
  }
  return v[0];
}

// the four lane groups of one token: per group the partial of each ring slot (0.f where the slot is empty) -> the planner's order.
// broken 1: the tree in ascending bit order (in the lane 1, 2, 4, 8, across lanes 16 then 32); broken 2: the empty slots skipped -- a tree
// over the 2 nch slots that are there (halving while the count is even, the rest in sequence) instead of over the full ring
float lane_sum4(const float part[4][kTfSkinnyLnSlots], int nslots, int broken) {
  float g[4], t[4];
  for (int gi = 0; gi < 4; ++gi) {
    float p[kTfSkinnyLnSlots];
    memcpy(p, part[gi], sizeof p);
    if (broken == 1) {
      for (int o = 1; o < kTfSkinnyLnSlots; o <<= 1)
        for (int s = 0; s < kTfSkinnyLnSlots; s += 2 * o) p[s] = p[s] + p[s + o];
      g[gi] = p[0];
    } else if (broken == 2) {
      int n = nslots;
      while (n > 1 && n % 2 == 0) {
        n /= 2;
        for (int s = 0; s < n; ++s) p[s] = p[s] + p[s + n];
      }
      for (int s = 1; s < n; ++s) p[0] = p[0] + p[s];
      g[gi] = p[0];
    } else {
      g[gi] = tf_skinny_ln_lane_tree(p);
    }
  }
  for (int st = 0; st < 2; ++st) {
    const int x = (broken == 1 ? tf_skinny_ln_lane_xor(1 - st) : tf_skinny_ln_lane_xor(st)) >> 4;      // lane xor 32 / 16 is group xor 2 / 1
    for (int gi = 0; gi < 4; ++gi) t[gi] = g[gi] + g[gi ^ x];
    memcpy(g, t, sizeof g);
  }
  return g[0];
}

}  // namespace

extern "C" {

int tf_skinny_ln_h_ok(int skinny_ok, int opt_skinny_ln, int K, int Kp, int N_of_ln) {
  return tf_skinny_ln_ok(skinny_ok != 0, opt_skinny_ln, K, Kp, N_of_ln) ? 1 : 0;
}
int tf_skinny_ln_h_vec_ok(int dtype16, int d) { return tf_ln_vec_ok(dtype16, d) ? 1 : 0; }
int tf_skinny_ln_h_consts(int* out4) {
  out4[0] = kTfSkinnyLnSlots; out4[1] = kTfSkinnyLnTreeSteps; out4[2] = tf_skinny_ln_lane_xor(0); out4[3] = tf_skinny_ln_lane_xor(1);
  return 0;
}

// One row: d % 64 == 0, 64 <= d <= 512, `row` its d 16-bit patterns (bf16 != 0: bfloat16, else float16).  out[0 .. 3] = the bit patterns
// of (wave sum, lane sum, wave square sum, lane square sum); each square sum is taken about its own side's mean.  Returns 0, or -1 on a
// bad d.
int tf_skinny_ln_h_order(int d, const uint16_t* row, int bf16, int broken, uint32_t* out) {
  if (d % 64 || d < 64 || d > 64 * kTfSkinnyDepth) return -1;
  const int nv = d / 8, nch = d / 64;
  std::vector<float> x((size_t)d);
  for (int i = 0; i < d; ++i) x[i] = bf16 ? bf16_to_f32(row[i]) : f16_to_f32(row[i]);
  float lane[64], part[4][kTfSkinnyLnSlots];
  float mean[2];
  for (int pass = 0; pass < 2; ++pass) {
    // tf_layernorm_vec: lane c holds vector c
    for (int c = 0; c < 64; ++c) lane[c] = c < nv ? (pass ? vec_sq(&x[(size_t)c * 8], mean[0]) : vec_sum(&x[(size_t)c * 8])) : 0.f;
    const float w = wave_sum64(lane);
    // tf_gemm_skinny_ln: group g holds vector tf_skinny_ln_vec(slot, g) in slot (chunk, ks)
    for (int g = 0; g < 4; ++g)
      for (int sl = 0; sl < kTfSkinnyLnSlots; ++sl) {
        const int v = tf_skinny_ln_vec(sl, g);
        part[g][sl] = (sl >> 1) < nch ? (pass ? vec_sq(&x[(size_t)v * 8], mean[1]) : vec_sum(&x[(size_t)v * 8])) : 0.f;
      }
    const float l = lane_sum4(part, 2 * nch, broken);
    if (!pass) { mean[0] = w / d; mean[1] = l / d; }
    out[2 * pass] = bits_of(w); out[2 * pass + 1] = bits_of(l);
  }
  return 0;
}

// One launch: d % 64 == 0 <= 512, N % 128 == 0, MT 1 or 2.  fails[0 .. 2] = cover, bounds, meaning; returns whether any is non-zero.
// broken 1: wave ft stores chunk ft % nch; 2: ks ignored in the store offset; 4: token tile 1 stored 16 rows further
int tf_skinny_ln_h_cover(int d, int N, int MT, int broken, long long* fails) {
  const int nch = d / 64;
  const size_t hbytes = (size_t)16 * MT * d * 2;
  std::vector<uint8_t> h(hbytes, 0);                                  // exactly as large as what the launch may write
  std::vector<int> count(hbytes / 16, 0);
  long long cover = 0, bounds = 0, meaning = 0;
  const TfSkinnyLaunch l = tf_skinny_launch(N, MT);
  for (unsigned b = 0; b < l.grid; ++b)
    for (unsigned wv = 0; wv < l.block / 64; ++wv) {
      const int ft = tf_skinny_tile((int)b, (int)wv);
      int hc = tf_skinny_ln_h_chunk(ft, nch);
      if (broken & 1) hc = ft % nch;
      if (hc >= nch || hc < -1) { ++bounds; continue; }
      if (hc < 0) continue;
      for (int lane = 0; lane < 64; ++lane)
        for (int tt = 0; tt < MT; ++tt)
          for (int ks = 0; ks < 2; ++ks) {
            size_t off = tf_skinny_ln_h_off(tt, hc, (broken & 2) ? 0 : ks, lane, d);
            if ((broken & 4) && tt == 1) off += (size_t)16 * d * 2;
            if (off + 16 > hbytes || off % 16) { ++bounds; continue; }
            memset(h.data() + off, 0xff, 16);                             // the store itself
            ++count[off / 16];
            if (broken) continue;
            // where it loaded: vector tf_skinny_ln_vec of row tf_skinny_x_row, and the columns of gamma / beta of that vector
            const int v = tf_skinny_ln_vec(tf_skinny_ln_slot(hc, ks), lane >> 4);
            if (off != tf_skinny_x_off(tt, hc, ks, lane, d)) ++meaning;
            if (off != (size_t)tf_skinny_x_row(tt, lane) * d * 2 + (size_t)v * 16) ++meaning;
            if (v != 8 * hc + 4 * ks + (lane >> 4) || v < 0 || v >= d / 8) ++meaning;
            if (tf_skinny_ln_col(hc, ks, lane) != v * 8 || v * 8 + 8 > d) ++meaning;
          }
    }
  for (int c : count) cover += c != 1;
  for (uint8_t v : h) cover += v != 0xff;
  fails[0] = cover; fails[1] = bounds; fails[2] = meaning;
  return (int)((cover + bounds + meaning) != 0);
}

}  // extern "C"

#ifdef TF_SKINNY_LN_MAIN
#include <stdio.h>
int main() {
  int shapes = 0, rows = 0, failures = 0;
  const int ds[] = {128, 256, 384, 512};
  for (int d : ds)
    for (int N : {128, 384, 1536})
      for (int MT = 1; MT <= 2; ++MT) {
        long long f[3];
        failures += tf_skinny_ln_h_cover(d, N, MT, 0, f);
        if (N / 16 > d / 64) failures += !tf_skinny_ln_h_cover(d, N, MT, 1, f);      // (ft % nch repeats only where there are more waves than chunks)
        failures += !tf_skinny_ln_h_cover(d, N, MT, 2, f);
        ++shapes;
      }
  uint32_t seed = 12345u;
  for (int d : ds)
    for (int r = 0; r < 64; ++r) {
      std::vector<uint16_t> row((size_t)d);
      for (int bf = 0; bf < 2; ++bf) {
        for (int i = 0; i < d; ++i) {
          seed = seed * 1664525u + 1013904223u;
          // float16 / bfloat16 patterns of finite values of mixed sign and magnitude (exponent field kept below the top)
          const uint16_t v = (uint16_t)(seed >> 16);
          row[i] = bf ? (uint16_t)((v & 0x8000) | (((v >> 7) & 0x0f) + 120) << 7 | (v & 0x7f)) : (uint16_t)((v & 0x8000) | (((v >> 10) & 0x0f) + 8) << 10 | (v & 0x3ff));
        }
        uint32_t o[4];
        failures += tf_skinny_ln_h_order(d, row.data(), bf, 0, o) != 0 || o[0] != o[1] || o[2] != o[3];
        ++rows;
      }
    }
  for (int M = 0; M <= 40; ++M)
    for (int d : {64, 128, 384, 512, 576, 640})
      for (int bits = 0; bits < 8; ++bits) {
        const int sk = bits & 1, opt = (bits >> 1) & 1, same = (bits >> 2) & 1;
        const bool skinny_ok = tf_skinny_ok(1, sk, 0, 1, 0, M);
        const bool want = sk && opt && same && M >= 1 && M <= 32 && d <= 512;
        failures += (tf_skinny_ln_h_ok(skinny_ok, opt, same ? d : 4 * d, same ? d : 4 * d, d) != 0) != want;
      }
  printf("%d shapes, %d rows, %d failures\n", shapes, rows, failures);
  return failures ? 1 : 0;
}
#endif
