"""The checker of the encoder's attention under a compiled mask (tests/tf_attn_mask_bound.py), held on the CPU before the
device is held to it (tests/test_gpu_tf_mask.py):

  1. the fp64 restatement of the masked forward matches the reference module's recorded output under three masks that are neither
     causal nor a band (tests/golden/tf_mask_fixture.npz) within 1e-5, bool and float spellings alike;
  2. the element-wise bound passes the emulation of the kernel's walk on every test shape and fails every one of its broken copies;
  3. the C-ABI: _lib.SIGNATURES holds the new symbols, the library exports them, NULL arguments are refused.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tf_attn_mask_bound as MB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["flope_tf_mask_create", "flope_tf_mask_destroy", "flope_tf_mask_info", "flope_tf_forward_masked", "flope_tf_attention_masked",
           "flope_tf_forward_flops_masked"]


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_mask_fixture.npz"), allow_pickle=False)
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    return f, sd


def test_fixture_is_small_and_data_only(fixture):
    f, sd = fixture
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "tf_mask_fixture.npz")) < 128 * 1024
    assert f["x"].shape == (6, 15, 16)
    for name in ("random", "blocks", "prefix"):
        assert f["mask_" + name].shape == (15, 15) and f["mask_" + name].dtype == np.bool_ and f["y_" + name].shape == (6, 15, 9)
        assert not f["mask_" + name].all(axis=1).any()                       # True = masked: no row without a key
    assert np.isfinite(f["y_random_float"]).all()


def test_fixture_masks_are_the_documented_ones(fixture):
    f, _ = fixture
    assert np.array_equal(~f["mask_blocks"], MB.block_diagonal([4, 1, 7, 3]).numpy())
    assert np.array_equal(~f["mask_prefix"], MB.make_allowed("prefix", 15).numpy())
    assert not f["mask_random"].diagonal().any() and 0.25 < f["mask_random"].mean() < 0.5
    for name in ("random", "blocks", "prefix"):                              # none of them has one of the three dedicated kernels
        from flope_amd.tf_encoder import _mask_window
        with pytest.raises(ValueError, match="has a kernel"):
            _mask_window(torch.from_numpy(f["mask_" + name]), 15)


def test_bool_and_float_spellings_agree(fixture):
    f, _ = fixture
    assert np.array_equal(f["y_random"], f["y_random_float"])


@pytest.mark.parametrize("name", ["random", "blocks", "prefix"])
def test_restatement_matches_the_reference(fixture, name):
    f, sd = fixture
    got = MB.masked_forward(sd, f["x"], ~f["mask_" + name])
    worst = float(np.abs(got - f["y_" + name]).max())
    print(f"fp64 restatement vs the reference under the {name} mask: {worst:.2e}")
    assert worst < 1e-5


def test_restatement_with_lengths_is_each_sequence_under_the_corner(fixture):
    f, sd = fixture
    allowed = ~f["mask_prefix"]
    lengths = [15, 1, 7, 12, 3, 15]
    got = MB.masked_forward(sd, f["x"], allowed, lengths)
    for b, n in enumerate(lengths):
        alone = MB.masked_forward(sd, f["x"][b:b + 1, :n], allowed[:n, :n])
        assert np.array_equal(got[b, :n], alone[0])
        assert np.array_equal(got[b, n:], np.broadcast_to(sd["out_layer.bias"].astype(np.float64), (15 - n, 9)))


# ---- 2. the bound and the walk -----------------------------------------------------------------------------------------------------
CASES = [(kind, L, hd) for kind in MB.KINDS for L in MB.LENGTHS for hd in MB.HEAD_DIMS]


def test_edge_mask_has_the_rows_the_kernel_can_go_wrong_at():
    a = MB.make_allowed("edge", 130)
    first = [int(r.nonzero()[0]) for r in a]
    last = [int(r.nonzero()[-1]) for r in a]
    assert (first[0], last[0]) == (129, 129) and (first[1], last[1]) == (0, 0)
    for f in MB.FIRSTS:
        assert first[f] == f and last[f] == 129
    trips = a[2, 0:64].any(), a[2, 64:128].any(), a[2, 128:].any()
    assert trips == (True, False, True)
    assert a[3, 1:65].any() and not a[3, 65:129].any() and a[3, 129]
    for L in MB.LENGTHS:
        for kind in MB.KINDS:
            assert MB.make_allowed(kind, L).any(dim=1).all(), (kind, L)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_bound_passes_the_emulation(dtype):
    worst = 0.0
    for kind, L, hd in CASES:
        if dtype != "f32" and L == 130 and kind in ("prefix", "band"):      # the three dtypes share the walk: the long cases once
            continue
        qkv = MB.make_qkv(2, L, 2, hd, dtype)
        ref, bound = MB.reference(kind, 2, L, 2, hd, dtype)
        r, at = MB.ratio(MB.emulate(qkv, MB.make_allowed(kind, L), 2, dtype), ref, bound)
        worst = max(worst, r)
        assert r < 1.0, (kind, L, hd, r, at)
    print(f"{dtype}: emulation within {worst:.3f} of the bound")


def test_bound_passes_the_emulation_under_lengths():
    lengths = (65, 1, 33)
    qkv = MB.make_qkv(3, 65, 2, 6, "f32")
    for kind in ("prefix", "band"):
        ref, bound = MB.reference(kind, 3, 65, 2, 6, "f32", lengths)
        r, at = MB.ratio(MB.emulate(qkv, MB.make_allowed(kind, 65), 2, "f32", lengths), ref, bound, lengths)
        assert r < 1.0, (kind, r, at)


# the case each defect shows at: (kind, L, head_dim)
MUTATION_CASE = {"nobit": ("random", 33, 6), "word31": ("random", 65, 6), "base0": ("edge", 130, 6), "lastdrop": ("random", 15, 6),
                 "maskedsum": ("random", 65, 64), "skiptrip": ("edge", 130, 6)}


@pytest.mark.parametrize("mutation", MB.MUTATIONS)
def test_bound_fails_every_mutation(mutation):
    kind, L, hd = MUTATION_CASE[mutation]
    for dtype in ("f32", "bf16"):                                            # the widest bound of the three is bf16's
        qkv = MB.make_qkv(2, L, 2, hd, dtype)
        ref, bound = MB.reference(kind, 2, L, 2, hd, dtype)
        ok, _ = MB.ratio(MB.emulate(qkv, MB.make_allowed(kind, L), 2, dtype), ref, bound)
        bad, at = MB.ratio(MB.emulate(qkv, MB.make_allowed(kind, L), 2, dtype, mutation=mutation), ref, bound)
        print(f"{mutation} {dtype}: {bad:.3g} of the bound at {at} (intact: {ok:.3f})")
        assert ok < 1.0 < bad, (mutation, dtype, ok, bad)


def test_mutation_list_is_the_documented_one():
    assert set(MB.MUTATIONS) == set(MUTATION_CASE) and len(MB.MUTATIONS) == 6


# ---- 3. the C-ABI -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    from flope_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name + "(" in header, name
    assert _lib.TF_ATTN_MASKED == 4
    assert _lib.SIGNATURES["flope_tf_forward_masked"] == _lib.SIGNATURES["flope_tf_attention_masked"]
    assert "scripts/tf_encoder.py" in header[header.index("flope_tf_mask_handle") - 4000:header.index("flope_tf_mask_handle")]


def test_null_arguments_are_refused():
    from flope_amd import _lib
    lib = _lib.load()
    out = C.c_void_p()
    bits = (C.c_uint32 * 1)(1)
    assert lib.flope_tf_mask_create(None, 1, bits, C.byref(out)) == _lib.EINVAL and not out.value
    assert "NULL handle" in _lib.load().flope_tf_last_error(None).decode()
    assert lib.flope_tf_mask_destroy(None) == 0
    assert lib.flope_tf_mask_info(None, None, None) == _lib.EINVAL
    assert lib.flope_tf_forward_masked(None, None, 1, 1, None, None, None, None) == _lib.EINVAL
    assert lib.flope_tf_attention_masked(None, None, 1, 1, None, None, None, None) == _lib.EINVAL
    assert lib.flope_tf_forward_flops_masked(None, 1, None, None) == 0.0
