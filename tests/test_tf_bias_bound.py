"""The checker of the encoder's attention under a compiled additive bias (tests/tf_attn_bias_bound.py), held on the CPU
before the device is held to it (tests/test_gpu_tf_bias.py):

  1. the fp64 restatement of the biased forward matches the reference module's recorded output under four biases, two of them per
     head (tests/golden/tf_bias_fixture.npz), within 1e-5 (measured 5.0e-7 / 4.3e-7 / 4.7e-7 / 4.5e-7), and with a zero bias it is
     tests/tf_attn_mask_bound.py's masked_forward;
  2. the element-wise bound passes the emulation of the kernel's walk on every test shape and fails every one of its broken copies;
  3. the C-ABI: the library exports the two new symbols and refuses NULL arguments.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tf_attn_bias_bound as BB
import tf_attn_mask_bound as MB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alibi", "alibi_h", "rand", "rand_h"]


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_bias_fixture.npz"), allow_pickle=False)
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    return f, sd


def test_fixture_is_small_and_data_only(fixture):
    f, sd = fixture
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "tf_bias_fixture.npz")) < 128 * 1024
    assert f["x"].shape == (6, 15, 16)
    for name in NAMES:
        b = f["bias_" + name]
        assert b.dtype == np.float32 and b.shape == ((4, 15, 15) if name.endswith("_h") else (15, 15)) and f["y_" + name].shape == (6, 15, 9)
        assert np.isfinite(f["y_" + name]).all()
        assert not np.isnan(b).any() and not (b == np.inf).any() and (b > -np.inf).any(axis=-1).all()      # -inf or finite; no row without a key
    mask_fixture = np.load(os.path.join(ROOT, "tests", "golden", "tf_mask_fixture.npz"), allow_pickle=False)
    assert np.array_equal(f["x"], mask_fixture["x"])                             # the mask fixture's x and weights
    assert all(np.array_equal(sd[k], mask_fixture["sd::" + k]) for k in sd)


def test_fixture_biases_are_the_documented_ones(fixture):
    f, _ = fixture
    from flope_amd.tf_encoder import alibi_bias
    assert np.array_equal(f["bias_alibi"], alibi_bias(15, [0.5])[0].numpy())
    assert np.array_equal(f["bias_alibi_h"], alibi_bias(15, [2.0 ** -(h + 1) for h in range(4)]).numpy())
    masked = f["bias_rand"] == -np.inf
    assert not masked.diagonal().any() and 0.25 < masked.mean() < 0.5
    assert np.array_equal(f["bias_rand_h"] == -np.inf, np.broadcast_to(masked, (4, 15, 15)))               # one allowed set
    fin = f["bias_rand_h"][:, ~masked]
    assert 1.5 < fin.std() < 2.5 and not np.array_equal(fin[0], fin[1])          # 2 randn, independent per head
    from flope_amd.tf_encoder import _mask_allowed
    for name in ("alibi", "rand"):                                               # make_mask keeps refusing them
        with pytest.raises(ValueError, match="additive biases have no kernel"):
            _mask_allowed(torch.from_numpy(f["bias_" + name]))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference(fixture, name):
    f, sd = fixture
    got = BB.biased_forward(sd, f["x"], f["bias_" + name])
    worst = float(np.abs(got - f["y_" + name]).max())
    print(f"fp64 restatement vs the reference under the {name} bias: {worst:.2e}")
    assert worst < 1e-5


def test_zero_bias_is_the_masked_forward(fixture):
    f, sd = fixture
    allowed = f["bias_rand"] > -np.inf
    zero = np.where(allowed, 0.0, -np.inf)
    for lengths in (None, [15, 1, 7, 12, 3, 15]):
        if lengths is not None:
            allowed = np.tril(np.ones((15, 15), dtype=bool)) | allowed            # every corner keeps its rows' keys
            zero = np.where(allowed, 0.0, -np.inf)
        assert np.array_equal(BB.biased_forward(sd, f["x"], zero, lengths), MB.masked_forward(sd, f["x"], allowed, lengths))
        assert np.array_equal(BB.biased_forward(sd, f["x"], np.broadcast_to(zero, (4, 15, 15)), lengths), MB.masked_forward(sd, f["x"], allowed, lengths))


def test_restatement_with_lengths_is_each_sequence_under_the_corner(fixture):
    f, sd = fixture
    bias = f["bias_alibi_h"]
    lengths = [15, 1, 7, 12, 3, 15]
    got = BB.biased_forward(sd, f["x"], bias, lengths)
    for b, n in enumerate(lengths):
        alone = BB.biased_forward(sd, f["x"][b:b + 1, :n], bias[:, :n, :n])
        assert np.array_equal(got[b, :n], alone[0])
        assert np.array_equal(got[b, n:], np.broadcast_to(sd["out_layer.bias"].astype(np.float64), (15 - n, 9)))


# ---- 2. the bound and the walk -----------------------------------------------------------------------------------------------------
CASES = [(kind, L, hd) for kind in BB.KINDS for L in BB.LENGTHS for hd in BB.HEAD_DIMS]
RAGGED = (65, 1, 33)                                                             # lengths of the ragged case, L = 65


def test_biases_are_well_formed():
    for kind, L, _ in CASES:
        for planes in (None, 1):
            b = BB.make_bias(kind, L, 2, planes)
            assert b.dtype == torch.float32 and tuple(b.shape) == (2 if planes is None else 1, L, L)
            assert not torch.isnan(b).any() and not (b == float("inf")).any()
            assert ((b > BB.NINF) == BB.allowed_of(b)[None]).all() and BB.allowed_of(b).any(dim=1).all()
    assert torch.equal(BB.allowed_of(BB.make_bias("edge", 130, 2)), MB.make_allowed("edge", 130))
    assert torch.equal(BB.allowed_of(BB.make_bias("holes", 65, 2)), MB.make_allowed("random", 65))
    assert not torch.equal(BB.make_bias("holes", 65, 2)[0], BB.make_bias("holes", 65, 2)[1])


def test_zero_bias_bound_is_the_mask_bound_plus_one_rounding():
    """b = 0: the reference is the mask's, the bound the mask's with e one u a larger (the add that rounds nothing is still counted)"""
    qkv = MB.make_qkv(2, 33, 2, 6, "f32")
    allowed = MB.make_allowed("random", 33)
    zero = BB.over(allowed, torch.zeros(1, 33, 33))
    ref, bound = BB.reference_of(qkv, zero, 2, "f32")
    mref, mbound = MB.reference_of(qkv, allowed, 2, "f32")
    assert torch.equal(ref, mref) and (bound >= mbound).all() and (bound <= 1.2 * mbound).all()
    assert torch.equal(BB.emulate(qkv, zero, 2, "f32"), MB.emulate(qkv, allowed, 2, "f32"))


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_bound_passes_the_emulation(dtype):
    worst = 0.0
    for kind, L, hd in CASES:
        if dtype != "f32" and L == 130 and kind != "edge":                      # the three dtypes share the walk: the long cases once
            continue
        qkv = MB.make_qkv(2, L, 2, hd, dtype)
        ref, bound = BB.reference(kind, 2, L, 2, hd, dtype)
        r, at = BB.ratio(BB.emulate(qkv, BB.make_bias(kind, L, 2), 2, dtype), ref, bound)
        worst = max(worst, r)
        assert r < 1.0, (kind, L, hd, r, at)
    print(f"{dtype}: emulation within {worst:.3f} of the bound")


def test_bound_passes_the_emulation_with_one_plane_and_under_lengths():
    qkv = MB.make_qkv(3, 65, 2, 6, "f32")
    for kind in ("alibi", "holes"):                                              # both keep the diagonal, so every corner keeps its rows' keys
        for planes in (None, 1):
            ref, bound = BB.reference(kind, 3, 65, 2, 6, "f32", RAGGED, planes)
            r, at = BB.ratio(BB.emulate(qkv, BB.make_bias(kind, 65, 2, planes), 2, "f32", RAGGED), ref, bound, RAGGED)
            assert r < 1.0, (kind, planes, r, at)


# the case each defect shows at: (kind, L, head_dim, lengths)
MUTATION_CASE = {"nobias": ("holes", 33, 6, None), "plane0": ("alibi", 33, 6, None), "lanerel": ("edge", 65, 6, None),
                 "transposed": ("holes", 33, 64, None), "prescale": ("holes", 15, 6, None), "cornerstride": ("alibi", 65, 6, RAGGED)}


@pytest.mark.parametrize("mutation", BB.MUTATIONS)
def test_bound_fails_every_mutation(mutation):
    kind, L, hd, lengths = MUTATION_CASE[mutation]
    B = 2 if lengths is None else len(lengths)
    for dtype in ("f32", "bf16"):                                                # the widest bound of the three is bf16's
        qkv = MB.make_qkv(B, L, 2, hd, dtype)
        bias = BB.make_bias(kind, L, 2)
        ref, bound = BB.reference(kind, B, L, 2, hd, dtype, lengths)
        ok, _ = BB.ratio(BB.emulate(qkv, bias, 2, dtype, lengths), ref, bound, lengths)
        bad, at = BB.ratio(BB.emulate(qkv, bias, 2, dtype, lengths, mutation=mutation), ref, bound, lengths)
        print(f"{mutation} {dtype}: {bad:.3g} of the bound at {at} (intact: {ok:.3f})")
        assert ok < 1.0 < bad, (mutation, dtype, ok, bad)


def test_cornerstride_shows_only_in_a_ragged_batch():
    qkv = MB.make_qkv(2, 33, 2, 6, "f32")
    bias = BB.make_bias("alibi", 33, 2)
    assert torch.equal(BB.emulate(qkv, bias, 2, "f32", mutation="cornerstride"), BB.emulate(qkv, bias, 2, "f32"))


def test_mutation_list_is_the_documented_one():
    assert set(BB.MUTATIONS) == set(MUTATION_CASE) and len(BB.MUTATIONS) == 6


# ---- 3. the C-ABI -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_null_arguments_refused():
    from flope_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "flope_tf_bias_create") and hasattr(lib, "flope_tf_mask_bias_planes")
    out = C.c_void_p()
    b = (C.c_float * 1)(0.0)
    assert lib.flope_tf_bias_create(None, 1, 1, b, C.byref(out)) == _lib.EINVAL and not out.value
    assert "NULL handle" in lib.flope_tf_last_error(None).decode()
    assert lib.flope_tf_mask_bias_planes(None) == _lib.EINVAL
    assert "NULL mask" in lib.flope_tf_last_error(None).decode()
