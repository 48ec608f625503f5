// The encoder's GELU (torch's activation="gelu": the exact erf form 0.5 x (1 + erf(x / sqrt 2)), not the tanh form), in ONE place and
// without HIP or libm: every linear kernel of tf_encoder.hip applies it to its float32 accumulator, and
// tests/host_harness/harness_tf_arch.cpp compiles the same text for the CPU, where its error against fp64 is measured
// (tests/test_tf_arch_host.py).  Only +, x, fmaf, fabsf, copysignf and one IEEE division.
//
// erf by Abramowitz & Stegun 7.1.28: for t >= 0, erfc t = (1 + a1 t + .. + a6 t^6)^-16 with |error| <= 3e-7.  With q = erfc(|x| / sqrt 2)
// the normal distribution is Phi(x) = q / 2 for x < 0 and 1 - q / 2 for x >= 0, written without a branch as 0.5 + copysign(0.5 - q / 2, x);
// the small side is never 1 - (1 - small) of two rounded values of different size, and what counts for x Phi(x) is Phi's ABSOLUTE error
// (the bound of tests/tf_act_bound.py is G 2^-23 |x|).
//   NaN            every step is arithmetic on x: NaN
//   +inf           p = inf, q = 0, Phi = 1: +inf;  -inf: Phi = 0, -inf x 0 = NaN -- never a finite non-zero value
//   |x| large      p^16 overflows to inf, q = 0: x or -0
//   0              p = 1, q = 1, Phi = 0.5: 0 (the sign of x)
#pragma once
#include <math.h>

#ifndef TF_ACT_HD
#if defined(__HIPCC__)
#define TF_ACT_HD __host__ __device__
#else
#define TF_ACT_HD
#endif
#endif

#define FLOPE_TF_ACT_NONE 0
#define FLOPE_TF_ACT_RELU 1
#define FLOPE_TF_ACT_GELU 2

TF_ACT_HD inline float tf_gelu_f32(float x) {
  const float t = fabsf(x) * 0.70710678118654752f;
  float p = 0.0000430638f;
  p = fmaf(p, t, 0.0002765672f);
  p = fmaf(p, t, 0.0001520143f);
  p = fmaf(p, t, 0.0092705272f);
  p = fmaf(p, t, 0.0422820123f);
  p = fmaf(p, t, 0.0705230784f);
  p = fmaf(p, t, 1.0f);
  p = p * p;
  p = p * p;
  p = p * p;
  p = p * p;
  const float hq = 0.5f / p;                          // erfc(|x| / sqrt 2) / 2
  const float phi = 0.5f + copysignf(0.5f - hq, x);
  return x * phi;
}
