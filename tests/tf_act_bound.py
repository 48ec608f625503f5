"""The element-wise bound of a GELU'd encoder linear, on top of tests/tf_linear_bound.py, which it imports unchanged.

    acc = x W^T + b in fp64,  ref = gelu64(acc) = 0.5 acc (1 + erf(acc / sqrt 2))
    bound = u |ref| + 1.13 (K + 2) 2^-23 mag + G 2^-23 |acc| + tiny

  u |ref|, mag, tiny        as in tf_linear_bound.py: the one rounding of the store, the float32 sum of K products and the bias
  1.13                      >= sup |gelu'| = 1.1290 at x = sqrt 2: the error of the pre-activation passes through at most that much larger
  G 2^-23 |acc|             the float32 evaluation error of tf_gelu_f32 (flope_amd/csrc/tf_act.h).  G is measured, not chosen:
                            tests/test_tf_arch_host.py walks the header's function, compiled with every product and sum rounded on its own,
                            against fp64 over 2^24 float32 values of [-16, 16] and the neighbourhoods of 0, and asserts that its worst
                            error in units of 2^-23 |x| is at most G_WORST below; G = 2 ceil(G_WORST), the factor 2 being this file's
                            convention of one ulp where half would do per rounding (it covers a device compiler contracting a * b + c).
GELU has no residual form in any kernel.
"""
import math

import torch

import tf_linear_bound as LB

G_WORST = 8.01                        # measured 8.002 (at x = 0.0505); tests/test_tf_arch_host.py keeps it honest
G = 2 * math.ceil(G_WORST)            # 18
GELU_SLOPE = 1.13


def gelu64(t):
    t = t.double()
    return 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))


def gelu_linear_reference(x, W, b, out):
    """-> (ref, bound) in fp64 [rows, N].  x: as fed; W: as multiplied; out: "f16" / "bf16" / "f32", the type stored."""
    xd, Wd, bd = x.double(), W.double(), b.double()
    acc = xd @ Wd.t() + bd
    mag = xd.abs() @ Wd.abs().t() + bd.abs()
    ref = gelu64(acc)
    return ref, LB.U[out] * ref.abs() + GELU_SLOPE * (W.shape[1] + 2) * LB.ACC * mag + G * LB.ACC * acc.abs() + LB.TINY[out]


def _fma(a, b, c):
    """float32 fmaf: the product of two float32 is exact in fp64; the sum is rounded there and once more to float32"""
    return (a.double() * b.double() + c.double()).float()


def gelu_f32(x):
    """tf_gelu_f32 of flope_amd/csrc/tf_act.h step by step in float32"""
    x = x.float()
    t = x.abs() * torch.tensor(0.70710678118654752, dtype=torch.float32)
    p = torch.full_like(t, 0.0000430638)
    for a in (0.0002765672, 0.0001520143, 0.0092705272, 0.0422820123, 0.0705230784, 1.0):
        p = _fma(p, t, torch.tensor(a, dtype=torch.float32))
    for _ in range(4):
        p = p * p
    hq = 0.5 / p
    return x * (0.5 + torch.copysign(0.5 - hq, x))


GELU_MUTATIONS = ["tanh", "sigmoid", "relu", "nohalf", "after_res"]


def emulate_gelu_linear(x, W, b, out, order="seq", mutation=None, r=None):
    """gelu(x W^T + b) with float32 products and partial sums (tf_linear_bound.fsum), tf_gelu_f32 in float32, stored once to `out`.
    mutation: None, or one defect
         tanh        the tanh form 0.5 a (1 + tanh(sqrt(2 / pi) (a + 0.044715 a^3)))
         sigmoid     a sigmoid(1.702 a)                     relu       ReLU in GELU's place
         nohalf      the factor 1/2 missing                  after_res  GELU applied behind a residual add (r, standard normal)"""
    p = x.float()[:, None, :] * W.float()[None, :, :]
    acc = LB.fsum(p, order) + b.float()
    if mutation == "tanh":
        y = 0.5 * acc * (1.0 + torch.tanh(0.7978845608028654 * (acc + 0.044715 * acc * acc * acc)))
    elif mutation == "sigmoid":
        y = acc * torch.sigmoid(1.702 * acc)
    elif mutation == "relu":
        y = torch.relu(acc)
    elif mutation == "nohalf":
        y = 2.0 * gelu_f32(acc)
    elif mutation == "after_res":
        y = gelu_f32(acc + r.float())
    else:
        y = gelu_f32(acc)
    return y.to(LB.TDT[out])
