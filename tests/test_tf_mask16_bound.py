"""The checker of tests/test_gpu_tf_mask16.py checked on the CPU (tests/tf_attn_mask16_bound.py):

  1. the float32 emulation of tf_attn_tiled_masked's walk passes the element-wise bound on every shape the device test holds to it;
  2. each broken copy of the walk fails the bound, or is non-finite, on at least one of those shapes (the shape is chosen where the
     defect can show, and named);
  3. the emulation reproduces the bit contracts it can state in float32: an all-clear mask is tf_attn_bound.emulate, a causal band is
     tf_attn_window16_bound.emulate, a sequence of a ragged batch is that sequence alone.

The factors printed here (python -m pytest -s) are the ones DESIGN.md 38 quotes.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tf_attn_bound as AB                   # noqa: E402
import tf_attn_mask16_bound as M16           # noqa: E402
import tf_attn_mask_bound as MB              # noqa: E402
import tf_attn_window16_bound as W16         # noqa: E402

H = 2
PACKED = [4, 1, 33, 65, 27]                  # block-diagonal at offsets that are no multiples of 32: held to the bound


def shapes():
    """(name, allowed, L, head_dim, lengths): what tests/test_gpu_tf_mask16.py holds to the bound; one head_dim per length, all four used"""
    for i, L in enumerate(M16.LENGTHS):
        for kind in M16.KINDS:
            yield f"{kind}{L}", MB.make_allowed(kind, L), L, M16.HEAD_DIMS[i % 4], None
    yield "gap257", M16.gap_mask(), 257, 64, None
    yield "dead129", M16.dead_mask(129), 129, 96, None
    yield "packed130", MB.block_diagonal(PACKED), sum(PACKED), 128, None
    yield "random257ragged", MB.make_allowed("random", 257), 257, 32, (257, 130, 66)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_emulation_passes_the_bound_on_every_device_shape(dtype):
    worst = 0.0
    for name, allowed, L, hd, lengths in shapes():
        B = 1 if lengths is None else len(lengths)
        qkv = MB.make_qkv(B, L, H, hd, dtype)
        ref, bound = M16.reference_of(qkv, allowed, H, dtype, lengths)
        r, where = M16.ratio(M16.emulate(qkv, allowed, H, dtype, lengths), ref, bound, lengths)
        print(f"{dtype} {name} hd {hd}: emulation at {r:.3f} of the bound at {where}")
        assert r <= 1.0, (name, r, where)
        worst = max(worst, r)
    print(f"{dtype}: worst {worst:.3f}")


# where each defect shows: (mask name, allowed, L, head_dim, poisoned keys)
SHOWS = {
    "noword": ("random129", lambda: MB.make_allowed("random", 129), 129, 64, None),
    "nextword": ("random129", lambda: MB.make_allowed("random", 129), 129, 64, None),
    "bitmap": ("random65", lambda: MB.make_allowed("random", 65), 65, 32, None),
    "some0": ("band129", lambda: MB.make_allowed("band", 129), 129, 96, None),
    "some2": ("prefix65", lambda: MB.make_allowed("prefix", 65), 65, 128, None),
    "noguard": ("band129", lambda: MB.make_allowed("band", 129), 129, 64, None),
    "nocolany": ("dead129", lambda: M16.dead_mask(129), 129, 96, [M16.DEAD_KEY]),
    "stagekb": ("gap257", M16.gap_mask, 257, 64, None),
}


@pytest.mark.parametrize("mutation", M16.MUTATIONS)
def test_each_broken_copy_fails(mutation):
    name, make, L, hd, dead = SHOWS[mutation]
    allowed = make()
    for dtype in ("f16", "bf16"):
        qkv = MB.make_qkv(1, L, H, hd, dtype)
        ref, bound = M16.reference_of(qkv, allowed, H, dtype)
        fed = M16.poison(qkv, dead) if dead else qkv
        good, _ = M16.ratio(M16.emulate(fed, allowed, H, dtype), ref, bound)
        bad, where = M16.ratio(M16.emulate(fed, allowed, H, dtype, mutation=mutation), ref, bound)
        print(f"{mutation} on {name} {dtype}: walk {good:.3f}, broken {bad:.3g} of the bound at {where}")
        assert good <= 1.0 and bad > 1.0, (mutation, dtype, good, bad)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_all_clear_is_the_unmasked_emulation_in_bits(dtype):
    for B, L, Hh, hd in AB.cases(64, 2):
        qkv = AB.make_qkv(B, L, Hh, hd, dtype)
        got = M16.emulate(qkv, torch.ones(L, L, dtype=torch.bool), Hh, dtype, rows="sequence")     # the products shaped as that emulation's
        want = AB.emulate(qkv, Hh, dtype)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (B, L, Hh, hd)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_band_is_the_windowed_emulation_in_bits(dtype):
    for (B, L, Hh, hd), W in W16.CASES:
        qkv = AB.make_qkv(B, L, Hh, hd, dtype)
        got = M16.emulate(qkv, MB.band_causal(L, W), Hh, dtype)
        want = W16.emulate(qkv, Hh, dtype, W)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (B, L, Hh, hd, W)


def test_a_ragged_sequence_is_that_sequence_alone_in_bits():
    L, hd, lengths = 257, 32, (257, 130, 66, 1)
    allowed = MB.make_allowed("random", L)                         # its diagonal is set: every corner leaves every row a key
    qkv = MB.make_qkv(len(lengths), L, H, hd, "f16")
    got = M16.emulate(qkv, allowed, H, "f16", lengths)
    for b, n in enumerate(lengths):
        alone = M16.emulate(qkv[b:b + 1, :n], allowed[:n, :n], H, "f16")
        assert torch.equal(got[b, :n].view(torch.int16), alone[0].view(torch.int16)), (b, n)
        assert not got[b, n:].any()
