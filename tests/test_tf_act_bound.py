"""The element-wise checker of a GELU'd encoder linear (tests/tf_act_bound.py) must bite: it passes an honest float32
emulation -- float32 products and partial sums in the three summation orders of tests/tf_linear_bound.py, tf_gelu_f32 step by step in
float32 -- and fails copies broken the way an activation epilogue breaks, one defect at a time, at float32 output, where the bound is
tightest, on at least one of the cases (the convention of tests/test_tf_linear_bound.py): the bound's float32 term grows with K mag,
while the tanh form is a fixed 4.7e-4 at most from the erf form, which the K = 128 case resolves and the K = 384 case cannot.  CPU only; the same reference and bound judge the device in tests/test_gpu_tf_arch.py.  Every test prints its figures (-s).
"""
import pytest
import torch

import tf_act_bound as AB
import tf_linear_bound as LB

# linear1 of the GPU test's shapes: (rows, K, N) with the weights of the shapes' state dicts
CASES = [((16, 128, 9, 2, 2, 256), 33), ((24, 384, 9, 6, 2, 1536), 5), ((16, 192, 5, 3, 1, 320), 17)]
OUTS = ["f32", "f16", "bf16"]


def _case(dims, rows, out):
    sd = LB.state_dict(dims)
    W, b = sd["transformer_encoder.layers.0.linear1.weight"], sd["transformer_encoder.layers.0.linear1.bias"]
    g = torch.Generator().manual_seed(77 + rows + dims[1])
    x = torch.randn(rows, dims[1], generator=g)
    r = torch.randn(rows, W.shape[0], generator=g)
    if out != "f32":                                                     # a 16-bit handle feeds 16-bit rows and multiplies by 16-bit weights
        x, W = x.to(LB.TDT[out]).float(), W.to(LB.TDT[out]).float()
    return x, W, b, r


@pytest.mark.parametrize("out", OUTS)
def test_honest_emulation_is_within_the_bound(out):
    worst = 0.0
    for dims, rows in CASES:
        x, W, b, _ = _case(dims, rows, out)
        ref, bound = AB.gelu_linear_reference(x, W, b, out)
        for order in LB.ORDERS:
            got = AB.emulate_gelu_linear(x, W, b, out, order)
            ratio, where = LB.ratio(got, ref, bound)
            print(f"gelu linear {dims[1]}->{W.shape[0]} rows {rows} {out} {order}: worst ratio {ratio:.4f} at {where}")
            worst = max(worst, ratio)
    assert worst <= 1.0


@pytest.mark.parametrize("mutation", AB.GELU_MUTATIONS)
def test_broken_copies_leave_the_bound_at_float32_output(mutation):
    caught = {}
    for dims, rows in CASES:
        x, W, b, r = _case(dims, rows, "f32")
        ref, bound = AB.gelu_linear_reference(x, W, b, "f32")
        for order in LB.ORDERS:
            got = AB.emulate_gelu_linear(x, W, b, "f32", order, mutation, r=r)
            ratio, where = LB.ratio(got, ref, bound)
            print(f"{mutation} {dims[1]}->{W.shape[0]} {order}: ratio {ratio:.1f} at {where}")
            caught[(dims[1], order)] = ratio > 1.0
    assert all(caught[(128, o)] for o in LB.ORDERS), caught              # every order of the K = 128 case
    if mutation != "tanh":
        assert all(caught.values()), caught


def test_the_tanh_form_is_not_what_tf_gelu_f32_computes():
    """The K = 384 case above cannot tell the tanh form from the erf form through a linear.  Directly, on the activation alone: over
    [-6, 6] the float32 emulation of tf_gelu_f32 stays within G_WORST 2^-23 |x| of fp64, and the tanh form leaves that by orders of
    magnitude (its gap to the erf form is up to 4.7e-4 near |x| = 2)."""
    x = torch.linspace(-6, 6, 120001, dtype=torch.float32)
    x = x[x != 0]
    ref = AB.gelu64(x)
    unit = AB.G_WORST * LB.ACC * x.double().abs() + 2.0 ** -149
    honest = float(((AB.gelu_f32(x).double() - ref).abs() / unit).max())
    tanh = 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
    d = (tanh.double() - ref).abs()
    broken = float((d / unit).max())
    print(f"against fp64 in units of G_WORST 2^-23 |x|: tf_gelu_f32 {honest:.3f}, the tanh form {broken:.1f}; largest gap {float(d.max()):.2e} at x = {float(x[int(d.argmax())]):.3f}")
    assert honest <= 1.0 and broken > 100.0 and 1e-4 < float(d.max()) < 1e-3


def test_the_constants():
    import math
    assert AB.G == 2 * math.ceil(AB.G_WORST) and AB.GELU_SLOPE >= 1.1290
    x = torch.linspace(-6, 6, 200001, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(AB.gelu64(x).sum(), x)
    i = int(g.abs().argmax())
    print(f"sup |gelu'| = {float(g.abs().max()):.5f} at x = {float(x[i]):.4f}")
    assert float(g.abs().max()) <= AB.GELU_SLOPE and abs(float(x[i]) - 2 ** 0.5) < 1e-3
