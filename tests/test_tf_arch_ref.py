"""The fp64 reference of the encoder's architectures without a device: tests/golden/tf_arch_fixture.npz equals torch's own
nn.TransformerEncoder recomputed; for the default architecture that construction agrees with oracle/tf_encoder_ref.py; arch_of reads
the three keywords from torch modules of all eight architectures and refuses what the kernels cannot run; expected_keys(final_norm=)."""
import numpy as np
import pytest
import torch

import tf_arch_cases as AC
from flope_amd.tf_encoder import arch_of, check_arch, expected_keys
from oracle import tf_encoder_ref as T


@pytest.fixture(scope="module")
def FX():
    return np.load(AC.FIXTURE)


@pytest.mark.parametrize("shape", list(AC.SHAPES))
def test_fixture_equals_torch_recomputed(FX, shape):
    dims = AC.SHAPES[shape]
    sd = AC.state_dict(dims, True)
    assert np.array_equal(FX[f"fnw_{shape}"], sd["transformer_encoder.norm.weight"].numpy())
    assert np.array_equal(FX[f"fnb_{shape}"], sd["transformer_encoder.norm.bias"].numpy())
    for B, L in AC.BL:
        x = AC.inputs(dims, B, L)
        assert np.array_equal(FX[f"x_{shape}_{B}x{L}"], x.numpy())
        for arch in AC.NON_DEFAULT:
            y = FX[AC.key(shape, arch, B, L)]
            assert y.dtype == np.float64 and y.shape == (B, L, dims[2])
            err = float(np.abs(AC.torch_reference(dims, arch, x).numpy() - y).max())
            assert err <= 1e-12, (AC.arch_id(arch), B, L, err)
    assert len(FX.files) == 2 * (2 + len(AC.BL) * (1 + len(AC.NON_DEFAULT)))


def test_default_architecture_agrees_with_the_oracle():
    dims = AC.SHAPES["a"]
    x = AC.inputs(dims, 2, 33)
    sd = {k: v.double().numpy() for k, v in AC.state_dict(dims, False).items()}
    ref = T.forward(sd, x.double().numpy(), dims[3])
    err = float(np.abs(AC.torch_reference(dims, AC.DEFAULT, x).numpy() - ref).max())
    print(f"torch fp64 vs oracle, default architecture: {err:.2e}")
    assert err <= 1e-6


def test_variants_differ_from_one_another():
    """the seven references are seven different functions: no keyword is ignored by the construction"""
    dims = AC.SHAPES["a"]
    x = AC.inputs(dims, 2, 33)
    ys = [AC.torch_reference(dims, a, x) for a in AC.ARCHS]
    for i in range(len(ys)):
        for j in range(i):
            assert float((ys[i] - ys[j]).abs().max()) > 1e-3, (AC.arch_id(AC.ARCHS[i]), AC.arch_id(AC.ARCHS[j]))


@pytest.mark.parametrize("arch", AC.ARCHS, ids=AC.arch_id)
def test_arch_of_reads_torch_modules(arch):
    m = AC.TorchEncoder(AC.SHAPES["a"], **arch)
    assert arch_of(m) == arch == check_arch(**arch)
    assert set(m.state_dict()) == set(expected_keys(2, arch["final_norm"]))


def test_arch_of_refuses_what_has_no_kernel():
    dims = AC.SHAPES["a"]
    bad = [AC.TorchEncoder(dims, layer_norm_eps=1e-6), AC.TorchEncoder(dims, bias=False), AC.TorchEncoder(dims, activation=torch.tanh),
           AC.TorchEncoder(dims, activation=torch.nn.GELU(approximate="tanh")), torch.nn.Linear(4, 4)]
    m = AC.TorchEncoder(dims, final_norm=True)
    m.transformer_encoder.norm = torch.nn.LayerNorm(dims[1], eps=1e-6)
    bad.append(m)
    m = AC.TorchEncoder(dims)
    m.transformer_encoder.layers[1].norm_first = True
    bad.append(m)
    for m in bad:
        with pytest.raises(ValueError):
            arch_of(m)
    assert arch_of(AC.TorchEncoder(dims, activation=torch.nn.GELU()))["activation"] == "gelu"


def test_expected_keys_with_a_final_norm():
    k = expected_keys(3, final_norm=True)
    assert k[-4:] == ["transformer_encoder.norm.weight", "transformer_encoder.norm.bias", "out_layer.weight", "out_layer.bias"]
    assert [x for x in k if "transformer_encoder.norm." not in x] == expected_keys(3)
