"""The streaming 16-bit MFMA attention of the encoder (tf_attn_tiled, option attn_tiled) on the device:

  1. every output element of flope_tf_attention against fp64 within the derived bound of tests/tf_attn_bound.py, on the smallest
     shapes at which a single step, a ragged step, a second query block, a block boundary, the reuse of a ring stage and each head
     width can go wrong; the rows behind the input are NaN and those behind the output a sentinel, so a read past B L shows up
     as NaN and a write past it in the sentinel, without any fault being provoked; two runs give equal bits;
  2. the kernel id the device reports equals the host rule (flope_amd/csrc/tf_attn_plan.h through the harness);
  3. head_dim 64, L <= 512: the bits of tf_attn_mfma (same lane-to-key map, same 32-key steps, same expression order);
  4. the whole encoder with attn_tiled = 1 against the fp64 oracle at the tolerances of tests/test_gpu_tf_encoder.py, token
     permutation equivariance, and option 0 afterwards reproduces the bits taken before.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import tf_attn_bound as AB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_ID = {"bf16": 0, "f16": 1, "f32": 2}
GENERIC, MFMA64, TILED, F32M = 0, 1, 2, 3
SENTINEL = 1234.0                    # exact in f16 and bf16


def _plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_attn.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_attn.so"])
    return C.CDLL(path)


PLAN = _plan()
KB, RING = PLAN.tf_attn_tiled_kb(), PLAN.tf_attn_tiled_ring()
CASES = AB.cases(KB, RING)


def _attn_handle(H, hd, dtype, max_tokens, **kw):
    """A handle for attention() alone: no layers, no weights."""
    from flope_amd.tf_encoder import TransformerEncoder
    return TransformerEncoder(16, H * hd, 9, H, 0, 64, dtype=dtype, max_tokens=max_tokens, **kw)


def _guarded(qkv, d):
    """qkv at the head of a tensor whose tail rows are NaN, out at the head of one whose tail is the sentinel"""
    B, L, d3 = qkv.shape
    big = torch.full((B * L + 64, d3), float("nan"), dtype=qkv.dtype, device="cuda")
    big[:B * L] = qkv.reshape(B * L, d3).cuda()
    obig = torch.full((B * L + 64, d), SENTINEL, dtype=qkv.dtype, device="cuda")
    return big, big[:B * L].view(B, L, d3), obig, obig[:B * L].view(B, L, d)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-L%d-H%d-hd%d" % c)
def test_every_element_within_the_bound_of_fp64(dtype, case):
    B, L, H, hd = case
    qkv = AB.make_qkv(B, L, H, hd, dtype)
    ref, bound = AB.reference(B, L, H, hd, dtype)
    enc = _attn_handle(H, hd, dtype, B * L, attn_tiled=2)
    big, q_in, obig, out = _guarded(qkv, H * hd)
    got = enc.attention(q_in, out=out)
    assert enc.last_attn_kernel == TILED
    torch.cuda.synchronize()
    first = obig.clone()
    assert torch.isfinite(got).all(), "a non-finite output: rows past B L were read, or a padded key was not masked"
    assert (obig[B * L:] == SENTINEL).all(), "a store past the last token"
    r, where = AB.ratio(got, ref, bound)
    print(f"{dtype} B={B} L={L} H={H} hd={hd}: max err / bound {r:.3f} at {where}")
    assert r <= 1.0
    obig[:B * L] = SENTINEL
    enc.attention(q_in, out=out)
    torch.cuda.synchronize()
    assert torch.equal(obig.view(torch.int16), first.view(torch.int16)), "two runs differ"
    assert torch.isnan(big[B * L:]).all()
    enc.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_dispatch_on_the_device_is_the_host_rule(dtype):
    def ids(H, hd, L, opts=(0, 1, 2), generic=0):
        enc = _attn_handle(H, hd, dtype, L)
        qkv = AB.make_qkv(1, L, H, hd, dtype).cuda()
        got = []
        for t in opts:
            assert enc.set_option("attn_tiled", t) >= 0
            enc.set_option("generic", generic)
            enc.attention(qkv)
            assert enc.last_attn_kernel == PLAN.tf_attn_pick(DT_ID[dtype], hd, L, generic, 0, t, 1)
            got.append(enc.last_attn_kernel)
        torch.cuda.synchronize()
        enc.close()
        return got

    assert ids(2, 32, 33) == [GENERIC, TILED, TILED]
    assert ids(1, 64, 50) == [MFMA64, MFMA64, TILED]
    assert ids(1, 64, 577) == [GENERIC, TILED, TILED]
    assert ids(2, 40, 33) == [GENERIC, GENERIC, GENERIC]
    assert ids(2, 32, 33, generic=1) == [GENERIC, GENERIC, GENERIC]
    assert ids(1, 64, 50, generic=1) == [GENERIC, GENERIC, GENERIC]


def test_option_values_and_float32_handles():
    enc = _attn_handle(2, 32, "f32", 33)
    assert enc.set_option("attn_tiled", 2) == 0 and enc.set_option("attn_tiled", 1) == 2      # stored: returns the previous value
    assert enc.set_option("attn_tiled", 3) < 0 and enc.set_option("attn_tiled", -1) < 0
    assert enc.set_option("attn_tiled", 2) == 1                                                 # a refused value changed nothing
    qkv = torch.randn(1, 33, 192, device="cuda")
    out = enc.attention(qkv)
    assert enc.last_attn_kernel == GENERIC == PLAN.tf_attn_pick(DT_ID["f32"], 32, 33, 0, 0, 2, 1)    # ... and ignored
    enc.set_option("f32mfma", 1)
    out_m = enc.attention(qkv)
    assert enc.last_attn_kernel == F32M
    q, k, v = (t.double().cpu() for t in AB.split_heads(qkv, 2))
    ref = AB.merge_heads(torch.softmax(q @ k.transpose(-1, -2) / 32 ** 0.5, dim=-1) @ v)
    assert (out.double().cpu() - ref).abs().max() < 1e-5 and (out_m.double().cpu() - ref).abs().max() < 1e-5
    with pytest.raises(ValueError):
        enc.attention(qkv.half())
    enc.close()
    from flope_amd.tf_encoder import TransformerEncoder
    with pytest.raises(ValueError, match="attn_tiled"):
        TransformerEncoder(16, 64, 9, 2, 0, 64, dtype="f16", max_tokens=8, attn_tiled=3)


def test_a_misaligned_buffer_runs_generic():
    enc = _attn_handle(2, 32, "f16", 33, attn_tiled=2)
    qkv = AB.make_qkv(1, 33, 2, 32, "f16")
    ref, bound = AB.reference(1, 33, 2, 32, "f16")
    flat = torch.zeros(qkv.numel() + 8, dtype=torch.float16, device="cuda")
    flat[1:1 + qkv.numel()] = qkv.reshape(-1).cuda()
    got = enc.attention(flat[1:1 + qkv.numel()].view(1, 33, 192))            # 2 bytes past a 16-byte boundary
    assert enc.last_attn_kernel == GENERIC == PLAN.tf_attn_pick(DT_ID["f16"], 32, 33, 0, 0, 2, 0)
    # the generic kernel keeps its probabilities in float32: inside the same bound
    assert AB.ratio(got, ref, bound)[0] <= 1.0
    enc.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("B,L,H", [(2, 129, 2), (3, 65, 2), (1, 50, 1), (1, 512, 1)])
def test_head_dim_64_gives_the_bits_of_the_resident_kernel(dtype, B, L, H):
    qkv = AB.make_qkv(B, L, H, 64, dtype).cuda()
    enc = _attn_handle(H, 64, dtype, B * L)
    old = enc.attention(qkv).clone()
    assert enc.last_attn_kernel == MFMA64
    enc.set_option("attn_tiled", 2)
    new = enc.attention(qkv)
    assert enc.last_attn_kernel == TILED
    torch.cuda.synchronize()
    diff = int((old.view(torch.int16) != new.view(torch.int16)).sum())
    print(f"{dtype} B={B} L={L} H={H}: {diff} of {old.numel()} elements differ in bits")
    assert diff == 0
    enc.close()


ENCODER_CASES = [((16, 128, 9, 4, 2, 256), 3, 50),        # head_dim 32
                 ((16, 128, 9, 2, 1, 128), 1, 577)]       # head_dim 64 past the resident kernel's 512 keys


@pytest.mark.parametrize("dims,B,L", ENCODER_CASES)
@pytest.mark.parametrize("dtype,tol", [("f16", 1.5e-2), ("bf16", 1.2e-1)])
def test_whole_encoder_with_the_option(dims, B, L, dtype, tol):
    from flope_amd.tf_encoder import TransformerEncoder
    from oracle import tf_encoder_ref as T
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((B, L, dims[0])).astype(np.float32)
    ref = T.forward(sd, x, num_heads=dims[3])
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=B * L)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    xg = torch.from_numpy(x).cuda()
    probe = torch.zeros(B, L, 3 * dims[1], dtype=AB.TDT[dtype], device="cuda")
    y0 = enc(xg).cpu().numpy()
    enc.attention(probe)
    assert enc.last_attn_kernel == GENERIC                   # what the forward above launched
    assert enc.set_option("attn_tiled", 1) == 0
    y = enc(xg).cpu().numpy()
    enc.attention(probe)
    assert enc.last_attn_kernel == TILED
    assert np.isfinite(y).all()
    print(f"{dtype} {dims} B={B} L={L}: |y - fp64|max {np.abs(y - ref).max():.3e} (option 0: {np.abs(y0 - ref).max():.3e}), tolerance {tol}")
    assert np.abs(y - ref).max() < tol
    perm = rng.permutation(L)
    yp = enc(xg[:, torch.from_numpy(perm).cuda()]).cpu().numpy()
    assert np.abs(yp - y[:, perm]).max() < tol
    assert enc.set_option("attn_tiled", 0) == 1
    assert np.array_equal(enc(xg).cpu().numpy(), y0)
    enc.close()
