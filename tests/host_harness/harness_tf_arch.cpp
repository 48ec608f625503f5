// CPU harness of the encoder's architecture list (flope_amd/csrc/tf_arch_plan.h, which run_forward_with walks) and of its GELU
// (flope_amd/csrc/tf_act.h, which every linear kernel applies): tests/test_tf_arch_host.py; DESIGN.md 50.  Built with
// -ffp-contract=off, so every product and sum of tf_gelu_f32 is rounded on its own unless the text says fmaf.
// With -DTF_ARCH_MAIN the file is a stand-alone program (run under AddressSanitizer + UBSan by the test).
#include "tf_arch_plan.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

using namespace flope_tf_plan;

namespace {

float bits_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
uint32_t f_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

double gelu64(double x) { return 0.5 * x * (1.0 + erf(x * 0.70710678118654752440)); }

// |tf_gelu_f32(x) - gelu64(x)| in units of 2^-23 |x|, one smallest subnormal forgiven (the `tiny` of the bound)
double gelu_err(float x) {
  const double e = fabs((double)tf_gelu_f32(x) - gelu64((double)x)) - ldexp(1.0, -149);
  return e <= 0 ? 0.0 : e / (ldexp(1.0, -23) * fabs((double)x));
}

// The op list with one defect, for the checks that must notice it
//   1  pre-norm: out_proj and linear2 take their residual from the normed buffer
//   2  LN2 moved in front of linear2 (normalises the hidden rows' source instead of linear1's)
//   3  the final norm skipped: out_layer reads the un-normed stream
int ops_of(const TfArch& a, int nl, int broken, TfOp* out, int cap) {
  int n = 0;
  const int cnt = tf_arch_op_count(a, nl);
  std::vector<TfOp> v;
  for (int i = 0; i < cnt; ++i) v.push_back(tf_arch_op(a, nl, i));
  if (broken == 1 && a.norm_first) {
    for (TfOp& o : v)
      if (o.kind == kTfOpLinear && o.res != kTfBufNone) o.res = o.res == kTfBufH ? kTfBufH2 : kTfBufH;
  }
  if (broken == 2) {
    for (size_t i = 0; i + 1 < v.size(); ++i)
      if (v[i].kind == kTfOpLayerNorm && v[i].name == kTfLnNorm2 && v[i + 1].name == kTfLinLinear1) { TfOp t = v[i]; v[i] = v[i + 1]; v[i + 1] = t; ++i; }
  }
  if (broken == 3 && a.final_norm) {
    v.erase(v.end() - 2);
    v.back().in = kTfBufH;
  }
  for (const TfOp& o : v) {
    if (n < cap) out[n] = o;
    ++n;
  }
  return n;
}

}  // namespace

extern "C" {

int tf_arch_h_valid(int nf, int act, int fn) { const TfArch a = {nf, act, fn}; return tf_arch_valid(a); }
int tf_arch_h_default(int nf, int act, int fn) { const TfArch a = {nf, act, fn}; return tf_arch_default(a); }
int tf_arch_h_count(int nf, int act, int fn, int nl) { const TfArch a = {nf, act, fn}; return tf_arch_op_count(a, nl); }
// out: 8 ints per op {kind, name, layer, in, res, out, act, fold}; returns the op count (which may exceed cap: nothing is written past it)
int tf_arch_h_ops(int nf, int act, int fn, int nl, int broken, int* out, int cap) {
  const TfArch a = {nf, act, fn};
  std::vector<TfOp> v((size_t)(cap > 0 ? cap : 0));
  const int n = ops_of(a, nl, broken, v.data(), cap);
  for (int i = 0; i < n && i < cap; ++i) {
    const TfOp& o = v[i];
    const int f[8] = {o.kind, o.name, o.layer, o.in, o.res, o.out, o.act, o.fold};
    memcpy(out + 8 * i, f, sizeof f);
  }
  return n;
}
void tf_arch_h_ln(int nf, int act, int fn, int nl, int* folded, int* launched) {
  const TfArch a = {nf, act, fn};
  *folded = tf_arch_ln_folded(a, nl);
  *launched = tf_arch_ln_launched(a, nl);
}

void tf_arch_h_gelu(const float* x, float* y, long long n) {
  for (long long i = 0; i < n; ++i) y[i] = tf_gelu_f32(x[i]);
}
double tf_arch_h_gelu64(double x) { return gelu64(x); }

// Every float32 of both signs whose magnitude's bit pattern is lo_bits + k stride <= hi_bits: the worst gelu_err, where, and how many
double tf_arch_h_gelu_walk(uint32_t lo_bits, uint32_t hi_bits, uint32_t stride, long long* count, float* worst_x) {
  double worst = 0;
  long long n = 0;
  for (uint64_t u = lo_bits; u <= hi_bits; u += stride) {
    for (int sgn = 0; sgn < 2; ++sgn) {
      const float x = bits_f((uint32_t)u | (sgn ? 0x80000000u : 0u));
      if (x == 0.f) continue;
      const double e = gelu_err(x);
      if (e > worst) { worst = e; if (worst_x) *worst_x = x; }
      ++n;
    }
  }
  if (count) *count = n;
  return worst;
}

}  // extern "C"

#ifdef TF_ARCH_MAIN
int main() {
  long long fails = 0, lists = 0;
  for (int nf = 0; nf < 2; ++nf)
    for (int act = 1; act <= 2; ++act)
      for (int fn = 0; fn < 2; ++fn)
        for (int nl = 0; nl <= 3; ++nl)
          for (int broken = 0; broken <= 3; ++broken) {
            const int cnt = tf_arch_h_count(nf, act, fn, nl);
            std::vector<int> out((size_t)8 * cnt);              // exactly the ops of the list: a write past it is reported
            const int n = tf_arch_h_ops(nf, act, fn, nl, broken, out.data(), cnt);
            if (broken == 0 && n != cnt) ++fails;
            int folded, launched;
            tf_arch_h_ln(nf, act, fn, nl, &folded, &launched);
            if (folded + launched != 2 * nl + fn) ++fails;
            ++lists;
          }
  const float xs[] = {0.f, -0.f, 1.f, -1.f, 1e-30f, 17.f, -17.f, 1e30f, -1e30f, INFINITY, -INFINITY, NAN};
  float ys[sizeof xs / sizeof xs[0]];
  tf_arch_h_gelu(xs, ys, (long long)(sizeof xs / sizeof xs[0]));
  if (ys[0] != 0.f || ys[2] <= 0.84f || ys[2] >= 0.85f || !(ys[9] == INFINITY) || ys[11] == ys[11]) ++fails;
  long long count = 0;
  float wx = 0;
  const double worst = tf_arch_h_gelu_walk(1, 0x41800000u, 1u << 14, &count, &wx);
  printf("%lld lists, %lld gelu points, worst %.3f at %g, %lld failures\n", lists, count, worst, (double)wx, fails);
  return fails ? 1 : 0;
}
#endif
