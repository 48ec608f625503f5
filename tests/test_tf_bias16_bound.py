"""The checker of tests/test_gpu_tf_bias16.py checked on the CPU (tests/tf_attn_bias16_bound.py):

  1. the float32 emulation of the BIASED tf_attn_tiled_masked passes the element-wise bound on every shape the device test holds to it, at
     every head_dim and both 16-bit dtypes;
  2. each broken copy of it fails the bound, or is non-finite, on a shape where the defect can show (chosen and named);
  3. under a zero bias the emulation is tests/tf_attn_mask16_bound.py's in bits, and the bound is never smaller than that module's;
  4. a sequence of a ragged batch is that sequence alone under the bias's corner, in bits.

The factors printed here (python -m pytest -s) are the ones DESIGN.md 44 quotes.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tf_attn_bias16_bound as B16           # noqa: E402
import tf_attn_mask16_bound as M16           # noqa: E402
import tf_attn_mask_bound as MB              # noqa: E402
from test_tf_mask16_bound import shapes as mask16_shapes      # noqa: E402  (the masks tests/test_gpu_tf_mask16.py holds to its bound)

H = 2


@pytest.mark.parametrize("hd", B16.HEAD_DIMS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_emulation_passes_the_bound_on_every_device_shape(dtype, hd):
    worst = 0.0
    for name, kind, L, planes, lengths in B16.shapes():
        B = 1 if lengths is None else len(lengths)
        qkv = MB.make_qkv(B, L, H, hd, dtype)
        bias = B16.make_bias(kind, L, H, planes)
        ref, bound = B16.reference_of(qkv, bias, H, dtype, lengths)
        r, where = B16.ratio(B16.emulate(qkv, bias, H, dtype, lengths), ref, bound, lengths)
        print(f"{dtype} {name} hd {hd}: emulation at {r:.3f} of the bound at {where}")
        assert r <= 1.0, (name, r, where)
        worst = max(worst, r)
    print(f"{dtype} hd {hd}: worst {worst:.3f}")


# where each defect shows: (kind, L, head_dim, planes, lengths)
SHOWS = {
    "nobias": ("holes", 129, 64, None, None),
    "plane0": ("alibi", 129, 32, None, None),               # head 1's slope is half of head 0's
    "nolog2e": ("alibi", 129, 96, None, None),
    "bitmap": ("holes", 65, 128, None, None),
    "transposed": ("holes", 65, 64, None, None),
    "cornerstride": ("holes", 257, 32, None, (130, 66)),    # both sequences shorter than L: every row but row 0 reads another row's entries
}


@pytest.mark.parametrize("mutation", B16.MUTATIONS)
def test_each_broken_copy_fails(mutation):
    kind, L, hd, planes, lengths = SHOWS[mutation]
    bias = B16.make_bias(kind, L, H, planes)
    for dtype in ("f16", "bf16"):
        qkv = MB.make_qkv(1 if lengths is None else len(lengths), L, H, hd, dtype)
        ref, bound = B16.reference_of(qkv, bias, H, dtype, lengths)
        good, _ = B16.ratio(B16.emulate(qkv, bias, H, dtype, lengths), ref, bound, lengths)
        bad, where = B16.ratio(B16.emulate(qkv, bias, H, dtype, lengths, mutation=mutation), ref, bound, lengths)
        print(f"{mutation} on {kind}{L} {dtype}: walk {good:.3f}, broken {bad:.3g} of the bound at {where}")
        assert good <= 1.0 and bad > 1.0, (mutation, dtype, good, bad)


def test_cornerstride_cannot_show_in_a_full_length_batch():
    """... which is why its shape is ragged: with n = L the stride is the right one"""
    bias = B16.make_bias("holes", 65, H)
    qkv = MB.make_qkv(1, 65, H, 32, "f16")
    assert torch.equal(B16.emulate(qkv, bias, H, "f16", mutation="cornerstride").view(torch.int16), B16.emulate(qkv, bias, H, "f16").view(torch.int16))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_zero_bias_is_the_mask_emulation_in_bits_and_the_bound_is_no_smaller(dtype):
    n = 0
    for name, allowed, L, hd, lengths in mask16_shapes():
        B = 1 if lengths is None else len(lengths)
        qkv = MB.make_qkv(B, L, H, hd, dtype)
        zero = B16.zero_over(allowed, H if n % 2 else 1)
        got = B16.emulate(qkv, zero, H, dtype, lengths)
        want = M16.emulate(qkv, allowed, H, dtype, lengths)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), name
        ref, bound = B16.reference_of(qkv, zero, H, dtype, lengths)
        mref, mbound = M16.reference_of(qkv, allowed, H, dtype, lengths)
        assert torch.equal(ref, mref) or float((ref - mref).abs().max()) < 1e-12, name
        assert bool((bound >= mbound).all()), name
        n += 1
    assert n >= 20


def test_a_ragged_sequence_is_that_sequence_alone_in_bits():
    L, hd, lengths = 257, 32, B16.RAGGED
    bias = B16.make_bias("holes", L, H)                            # its diagonal is allowed: every corner leaves every row a key
    qkv = MB.make_qkv(len(lengths), L, H, hd, "f16")
    got = B16.emulate(qkv, bias, H, "f16", lengths)
    for b, n in enumerate(lengths):
        alone = B16.emulate(qkv[b:b + 1, :n], bias[:, :n, :n].contiguous(), H, "f16")
        assert torch.equal(got[b, :n].view(torch.int16), alone[0].view(torch.int16)), (b, n)
        assert not got[b, n:].any()
