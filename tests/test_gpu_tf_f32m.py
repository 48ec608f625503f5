"""The float32 encoder on the exact-fp32 matrix instruction (flope_tf option f32mfma, TransformerEncoder(dtype="f32m")):
tf_linear_f32m and tf_attn_f32m of flope_amd/csrc/tf_encoder.hip.

Held to the reference's own output at the toy configuration (tests/golden/reference_fixtures.npz, 1e-5: the tolerance of the strict
float32 mode, which is another summation order of the same float32 arithmetic), to the fp64 oracle (oracle/tf_encoder_ref.py) at
2e-4 where the kernels can go wrong, to option 0 on the same handle, element by element to the bound of an fma chain in any order,
and bit for bit to the CPU walk of the kernel's feed order (tests/host_harness/harness_tf_f32m.cpp).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def _enc(dims, sd, dtype, max_tokens):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return enc


def _synthetic(dims, seed=5):
    from oracle import tf_encoder_ref as T
    return T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=seed)


def _run(enc, x):
    return enc(torch.from_numpy(np.ascontiguousarray(x)).cuda()).cpu().numpy()


# ---- 1. the reference's own output -------------------------------------------------------------------------------------------
def test_toy_f32m_matches_the_reference_output(ref_fixtures):
    sd = {k[len("tf_sd::"):]: v for k, v in ref_fixtures.items() if k.startswith("tf_sd::")}
    enc = _enc((16, 32, 9, 4, 2, 64), sd, "f32m", 128)
    x = ref_fixtures["tf_x"]
    y = _run(enc, x)
    assert y.shape == (8, 10, 9)
    err = float(np.abs(y - ref_fixtures["tf_y"]).max())
    print(f"toy f32m: max |y - tf_y| = {err:.2e}")
    assert err < 1e-5
    assert np.array_equal(_run(enc, x[:3]), y[:3])
    assert np.array_equal(_run(enc, x), y)
    enc.close()


# ---- 2. shapes where the kernels can go wrong ----------------------------------------------------------------------------------
CASES = [((20, 72, 9, 6, 1, 100), 3, 19),       # head_dim 12; no K and no N a multiple of 16
         ((24, 384, 9, 6, 2, 1536), 3, 257),    # the throughput shape, two layers
         ((16, 128, 9, 1, 1, 128), 2, 1),       # head_dim 128, a single token
         ((18, 64, 5, 2, 1, 64), 2, 21),        # K = 18: the embedding stays generic, the rest moves
         ((16, 40, 9, 4, 1, 48), 2, 17),        # head_dim 10: attention stays generic, the linears move
         ((16, 64, 9, 1, 1, 64), 1, 600)]       # more keys than the 16-bit kernel takes, several key tiles per wave


@pytest.mark.parametrize("dims,B,L", CASES)
def test_f32m_vs_oracle_and_strict_mode(dims, B, L):
    from oracle import tf_encoder_ref as T
    sd = _synthetic(dims)
    x = np.random.default_rng(1).standard_normal((B, L, dims[0])).astype(np.float32)
    ref = T.forward(sd, x, num_heads=dims[3])
    enc = _enc(dims, sd, "f32m", B * L)
    y = _run(enc, x)
    assert enc.set_option("f32mfma", 0) == 1
    y0 = _run(enc, x)
    assert enc.set_option("f32mfma", 1) == 0
    assert np.isfinite(y).all()
    e1, e0, dd = (float(np.abs(a).max()) for a in (y - ref, y0 - ref, y - y0))
    print(f"{dims} B = {B} L = {L}: |f32m - fp64| {e1:.2e}  |option 0 - fp64| {e0:.2e}  |f32m - option 0| {dd:.2e}  max |ref| {np.abs(ref).max():.2f}")
    assert e1 < 2e-4 and e0 < 2e-4 and dd < 2e-4
    enc.close()


# ---- 3. the linear kernel, element by element ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tfh():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_f32m.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_f32m.so"])
    lib = C.CDLL(path)
    lib.tf_f32m_image_floats.restype = C.c_long
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _walk(tfh, x, w, b):
    (M, K), N = x.shape, w.shape[0]
    w, b, x = (np.ascontiguousarray(a, dtype=np.float32) for a in (w, b, x))
    img = np.zeros(tfh.tf_f32m_image_floats(N, K), dtype=np.float32)
    tfh.tf_f32m_pack(_ptr(w), N, K, _ptr(img))
    y = np.full((M, N), np.nan, dtype=np.float32)
    assert tfh.tf_f32m_walk(_ptr(x), _ptr(img), _ptr(b), None, _ptr(y), M, K, N, 0, 2) == 0
    return y


@pytest.mark.parametrize("din,d,dout,M", [(20, 72, 9, 37), (16, 1536, 9, 50), (24, 384, 13, 131)])
def test_two_chained_linears_element_by_element(tfh, din, d, dout, M):
    """num_layers = 0: embedding, then out_layer.  bound = e1 |W2|^T + gamma(d + 1) ((|h| + e1) |W2|^T + |b2|) with
    e1 = gamma(in + 1) (|x| |W1|^T + |b1|) and h the fp64 intermediate: the bound of an fma chain in any order, the first layer's
    error carried through the second.  The model is the float32 one the handle holds: synthetic_state_dict may return float64 arrays
    (a float32 array over a float64 scalar), load_state_dict rounds them to float32, and the fp64 product and the walk take the
    same rounded weights."""
    dims = (din, d, dout, 1, 0, 16)
    sd = {k: np.asarray(v, dtype=np.float32) for k, v in _synthetic(dims).items()}
    x = np.random.default_rng(1).standard_normal((1, M, din)).astype(np.float32)
    enc = _enc(dims, sd, "f32m", M)
    y = _run(enc, x)[0]
    enc.close()
    W1, b1, W2, b2 = (sd[k].astype(np.float64) for k in ("embedding.weight", "embedding.bias", "out_layer.weight", "out_layer.bias"))
    x64 = x[0].astype(np.float64)
    h = x64 @ W1.T + b1
    ref = h @ W2.T + b2
    e1 = gamma(din + 1) * (np.abs(x64) @ np.abs(W1).T + np.abs(b1))
    bound = e1 @ np.abs(W2).T + gamma(d + 1) * ((np.abs(h) + e1) @ np.abs(W2).T + np.abs(b2))
    ratio = float((np.abs(y - ref) / bound).max())
    print(f"(in, d, out, M) = {(din, d, dout, M)}: max err / bound {ratio:.4f}, max |err| {np.abs(y - ref).max():.2e}")
    assert ratio <= 1.0
    hw = _walk(tfh, x[0], sd["embedding.weight"], sd["embedding.bias"])
    yw = _walk(tfh, hw, sd["out_layer.weight"], sd["out_layer.bias"])
    assert np.array_equal(y, yw), f"device and host walk differ in {np.count_nonzero(y != yw)} of {y.size} elements, max {np.abs(y - yw).max():.2e}"


# ---- 4. batch independence ---------------------------------------------------------------------------------------------------------
def test_a_sequence_does_not_depend_on_its_batch():
    dims, B, L = (20, 72, 9, 6, 1, 100), 5, 19
    rng = np.random.default_rng(1)
    x = rng.standard_normal((B, L, dims[0])).astype(np.float32)
    enc = _enc(dims, _synthetic(dims), "f32m", B * L)
    y = _run(enc, x)
    perm = rng.permutation(B)
    assert np.array_equal(_run(enc, x[perm]), y[perm])
    for i in range(B):
        assert np.array_equal(_run(enc, x[i:i + 1])[0], y[i])
    tperm = rng.permutation(L)
    dt = float(np.abs(_run(enc, x[:, tperm]) - y[:, tperm]).max())
    print(f"token permutation: max difference {dt:.2e}")
    assert dt < 2e-4                                                   # the key order changes the sums
    enc.close()


# ---- 5. option mechanics -------------------------------------------------------------------------------------------------------------
def test_option_mechanics():
    dims, B, L = (20, 72, 9, 6, 1, 100), 3, 19
    sd = _synthetic(dims)
    x = np.random.default_rng(1).standard_normal((B, L, dims[0])).astype(np.float32)
    enc = _enc(dims, sd, "f32m", B * L)
    y1 = _run(enc, x)
    enc.set_option("f32mfma", 0)
    y0 = _run(enc, x)
    enc.set_option("f32mfma", 1)
    assert np.array_equal(_run(enc, x), y1)
    strict = _enc(dims, sd, "f32", B * L)
    assert np.array_equal(_run(strict, x), y0)                         # option 0 is the strict mode
    strict.close()
    assert enc.set_option("nonsense", 1) < 0
    assert enc(torch.zeros(0, L, dims[0], device="cuda")).shape == (0, L, 9)
    with pytest.raises(RuntimeError, match="max_tokens"):
        enc(torch.zeros(B + 1, L, dims[0], device="cuda"))
    enc.close()
    h16 = _enc(dims, sd, "f16", B * L)
    a = _run(h16, x)
    assert h16.set_option("f32mfma", 1) == 0
    assert np.array_equal(_run(h16, x), a)
    h16.close()
