"""The float32 MFMA encoder linear (flope_tf option f32mfma, tf_linear_f32m in flope_amd/csrc/tf_encoder.hip) as far as a CPU can see it,
through tests/host_harness/harness_tf_f32m.cpp: the weight packer of host_pack.h (pack_tf_f32m) and a scalar walk of the kernel's
operand feed -- the float every lane loads for every MFMA of every 16-deep K step, from the packed image and row-major tokens,
accumulated as a float fmaf chain from the bias, then residual, then ReLU.

The bound is the standard one of an fma chain of K products and the bias in ANY order: |err| <= gamma(K + 1) (|x| |W|^T + |b|),
gamma(n) = n u / (1 - n u), u = 2^-24; the residual add costs one more rounding, u |y|, and ReLU none.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SHAPES = [(72, 20), (216, 72), (9, 72), (1536, 384), (32, 16)]      # (N, K)
TOKENS = [1, 19, 131]


def gamma(n):
    return n * U / (1 - n * U)


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


def pack(tfh, w):
    N, K = w.shape
    img = np.full(tfh.tf_f32m_image_floats(N, K), np.nan, dtype=np.float32)
    tfh.tf_f32m_pack(_ptr(np.ascontiguousarray(w)), N, K, _ptr(img))
    return img


def walk(tfh, x, w, b, r=None, relu=False, mp=1):
    M, K = x.shape
    N = w.shape[0]
    img = pack(tfh, w)
    y = np.full((M, N), np.nan, dtype=np.float32)
    rc = tfh.tf_f32m_walk(_ptr(np.ascontiguousarray(x)), _ptr(img), _ptr(np.ascontiguousarray(b)),
                          _ptr(np.ascontiguousarray(r)) if r is not None else None, _ptr(y), M, K, N, int(relu), mp)
    assert rc == 0, f"the walk left a buffer (code {rc})"
    return y


def _data(N, K, M, seed=3):
    rng = np.random.default_rng(seed)
    w = (rng.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.uniform(-.1, .1, N).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("N,K", SHAPES)
def test_packed_image_is_a_permutation_of_the_weights_plus_zeros(tfh, N, K):
    _, w, _ = _data(N, K, 1)
    img = pack(tfh, w)
    Np, Kp = (N + 15) // 16 * 16, (K + 15) // 16 * 16
    assert img.size == Np * Kp and np.isfinite(img).all()
    assert np.count_nonzero(w) == w.size                              # (so that zeros of the image are padding)
    nz = img[img != 0]
    assert nz.size == w.size and np.array_equal(np.sort(nz), np.sort(w.ravel()))
    assert np.count_nonzero(img == 0) == Np * Kp - N * K


@pytest.mark.parametrize("N,K", SHAPES)
def test_padding_rows_and_padding_k_are_zero(tfh, N, K):
    """Image position [block][step][tile][lane][s] is W[feature(block, tile, lane & 15)][16 step + 4 (lane >> 4) + s], and zero
    wherever that feature is >= N or that k is >= K: decoded here independently of the packer."""
    _, w, _ = _data(N, K, 1)
    img = pack(tfh, w)
    nsteps, nblk, pos, seen_pad = (K + 15) // 16, (N + 63) // 64, 0, 0
    for blk in range(nblk):
        nct = min(4, (N + 15) // 16 - blk * 4)
        tile = img[pos:pos + nsteps * nct * 256].reshape(nsteps, nct, 4, 16, 4)          # [step][ct][kq][i][s]
        pos += tile.size
        for ct in range(nct):
            for i in range(16):
                n = blk * 64 + (i >> 2) * 4 * nct + ct * 4 + (i & 3)
                row = tile[:, ct, :, i, :].reshape(-1)                                  # k = 16 step + 4 kq + s
                if n >= N:
                    assert not row.any()
                    seen_pad += 1
                else:
                    assert np.array_equal(row[:K], w[n]) and not row[K:].any()
    assert pos == img.size and seen_pad == (N + 15) // 16 * 16 - N


@pytest.mark.parametrize("M", TOKENS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_walk_is_within_the_fma_chain_bound_of_the_fp64_product(tfh, N, K, M):
    x, w, b = _data(N, K, M)
    y = walk(tfh, x, w, b, mp=2)
    assert np.isfinite(y).all(), "an output the walk never stored"
    x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    ref = x64 @ w64.T + b64
    bound = gamma(K + 1) * (np.abs(x64) @ np.abs(w64).T + np.abs(b64))
    ratio = float((np.abs(y - ref) / bound).max())
    print(f"N = {N}, K = {K}, M = {M}: max err / bound {ratio:.4f}, max |err| {np.abs(y - ref).max():.2e}")
    assert ratio <= 1.0


def test_residual_and_relu_epilogues(tfh):
    x, w, b = _data(72, 20, 19)
    r = np.random.default_rng(4).standard_normal((19, 72)).astype(np.float32)
    base = walk(tfh, x, w, b)
    assert np.array_equal(walk(tfh, x, w, b, r=r), base + r)           # one float add on the chain's result
    assert np.array_equal(walk(tfh, x, w, b, relu=True), np.maximum(base, 0))
    assert (base < 0).any() and (base > 0).any()


@pytest.mark.parametrize("N,K", SHAPES)
def test_tile_height_does_not_change_a_bit(tfh, N, K):
    """Every output is summed in one k order whatever the tiling: 1, 2 and 4 token tiles per wave give the same floats."""
    x, w, b = _data(N, K, 131 if N < 1000 else 19)
    a, c, d = (walk(tfh, x, w, b, mp=mp) for mp in (1, 2, 4))
    assert np.array_equal(a, c) and np.array_equal(a, d)


def test_tile_height_minimises_whole_rounds(tfh):
    def cost(M, N, mp, slots):
        return -(-(-(-M // (64 * mp)) * -(-N // 64)) // slots) * (4 * mp + 1)
    assert tfh.tf_f32m_plan_mp(65792, 1536, 256) == 4                  # many rounds: the large tile
    assert tfh.tf_f32m_plan_mp(57, 72, 256) == 1                       # a handful of tokens: as many workgroups as there are
    for M, N in ((65792, 384), (16384, 768), (771, 1152), (80, 32), (1, 9), (600, 64)):
        for slots in (256, 512):
            mp = tfh.tf_f32m_plan_mp(M, N, slots)
            assert mp in (1, 2, 4) and all(cost(M, N, mp, slots) <= cost(M, N, o, slots) for o in (1, 2, 4)), (M, N, slots, mp)
