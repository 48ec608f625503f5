"""Sliding-window attention on the 16-bit MFMA kernels on the device (option "window_mfma", TransformerEncoder(..., window_mfma=1);
DESIGN.md 28): under causal with a window a 16-bit launch keeps tf_attn_mfma / tf_attn_tiled, their WINDOW instantiations.

  1. attention alone   the eight cases of tests/tf_attn_window16_bound.py under attn_tiled 0, 1 and 2 wherever the pick is an MFMA
                       kernel: every element within the bound of reference_of, the kernel id tf_attn_pick names, option 0 on the same
                       input still generic and within the same bound
  2. equal bits        head_dim 64 resident = streamed, W >= L = causal on the same kernel, prefix = prefix, ragged = each sequence alone
  3. the whole forward TOY / WIDE / LONG of tests/test_gpu_tf_window.py within DESIGN.md 24's tolerances, mask= in bits, an undisturbed
                       handle, FLOPs
  4. stream            prefill = the ragged windowed forward in bits, steps within the tolerances, in bits where the kernel is generic
  5. refusals
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import tf_attn_bound as AB
import tf_attn_window16_bound as W16
import tf_attn_window_bound as WB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_ID = {"bf16": 0, "f16": 1}
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
GENERIC, MFMA64, TILED = 0, 1, 2
SENTINEL = 1234.0                    # exact in f16, bf16 and float32
TOL = {"f16": 1.5e-2, "bf16": 1.2e-1}
TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)


def _harness(name):
    path = os.path.join(ROOT, "tests", "host_harness", name)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/" + name])
    return C.CDLL(path)


def _pick(dtype, hd, L, tiled):
    """tf_attn_pick for an aligned 16-bit launch under options generic = 0, attn_tiled = tiled"""
    return _harness("libflope_host_tf_attn.so").tf_attn_pick(DT_ID[dtype], hd, L, 0, 0, tiled, 1)


def _rule(hd, L, tiled):
    """the same, restated for the parameter lists (include/flope_amd.h: "attn_tiled")"""
    pick = MFMA64 if hd == 64 and (L + 31) // 32 * 32 <= 512 else GENERIC
    if hd % 32 == 0 and hd <= 128 and (tiled == 2 or (tiled == 1 and pick == GENERIC)):
        pick = TILED
    return pick


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _attn_encoder(dtype, H, hd, max_tokens, tiled, window_mfma=1):
    from flope_amd.tf_encoder import TransformerEncoder
    return TransformerEncoder(16, H * hd, 9, H, 0, 64, dtype=dtype, max_tokens=max_tokens, attn_tiled=tiled, window_mfma=window_mfma)


@functools.lru_cache(maxsize=None)
def _reference(case, W, dtype):
    """computed once per case, shared, never changed"""
    return W16.reference_of(AB.make_qkv(*case, dtype), case[2], dtype, W)


# ---- 1. attention alone -----------------------------------------------------------------------------------------------------------
ATTN = [(c, W, t) for c, W in W16.CASES for t in (0, 1, 2) if _rule(c[3], c[1], t) != GENERIC]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case,W,tiled", ATTN, ids=lambda v: str(v).replace(" ", ""))
def test_attention_within_the_bound(case, W, tiled, dtype):
    Bn, L, H, hd = case
    d = H * hd
    want = _pick(dtype, hd, L, tiled)
    assert want == _rule(hd, L, tiled) and want in (MFMA64, TILED)
    enc = _attn_encoder(dtype, H, hd, Bn * L, tiled)
    host = AB.make_qkv(*case, dtype)
    qkv = host.cuda()
    ref, bound = _reference(case, W, dtype)
    obig = torch.full((64 + Bn * L + 64, d), SENTINEL, dtype=TDT[dtype], device="cuda")
    got = enc.attention(qkv, out=obig[64:64 + Bn * L].view(Bn, L, d), is_causal=True, window=W)
    assert enc.last_attn_kernel == want, "window_mfma = 1 keeps tf_attn_pick's kernel"
    torch.cuda.synchronize()
    assert (obig[:64] == SENTINEL).all() and (obig[64 + Bn * L:] == SENTINEL).all(), "a store outside the output"
    r, where = AB.ratio(got, ref, bound)
    print(f"{dtype} {case} W={W} attn_tiled={tiled} kernel {want}: err / bound {r:.3f} at {where} (headroom {1.0 / max(r, 1e-30):.2f}x)")
    assert torch.isfinite(got).all(), "a non-finite output: a query that saw nothing in its wave's first step"
    assert r <= 1.0, where
    assert enc.set_option("window_mfma", 0) == 1
    gen = enc.attention(qkv, is_causal=True, window=W)
    assert enc.last_attn_kernel == GENERIC, "window_mfma = 0 is the generic kernel"
    rg, whereg = AB.ratio(gen, ref, bound)
    print(f"    window_mfma=0 (generic): err / bound {rg:.3f} at {whereg}")
    assert rg <= 1.0, whereg
    enc.close()


# ---- 2. equal bits by construction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_head_dim_64_resident_and_streamed_give_equal_bits(dtype):
    for case, W in [(c, W) for c, W in W16.CASES if c[3] == 64]:
        Bn, L, H, hd = case
        assert L <= 512 and _pick(dtype, hd, L, 0) == MFMA64 and _pick(dtype, hd, L, 2) == TILED
        qkv = AB.make_qkv(*case, dtype).cuda()
        e0, e2 = _attn_encoder(dtype, H, hd, Bn * L, 0), _attn_encoder(dtype, H, hd, Bn * L, 2)
        a, b = e0.attention(qkv, is_causal=True, window=W), e2.attention(qkv, is_causal=True, window=W)
        assert (e0.last_attn_kernel, e2.last_attn_kernel) == (MFMA64, TILED)
        diff = int((_bits(a) != _bits(b)).sum())
        assert diff == 0, f"{dtype} {case} W={W}: {diff} elements differ between tf_attn_mfma and tf_attn_tiled"
        e0.close(); e2.close()


VARIANTS = [((2, 129, 2, 64), 33, 0), ((2, 129, 2, 64), 8, 2), ((1, 200, 1, 96), 64, 1), ((1, 161, 2, 32), 1, 1), ((1, 577, 2, 128), 100, 2),
            ((1, 290, 1, 64), 130, 0), ((1, 290, 1, 64), 130, 2)]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case,W,tiled", VARIANTS, ids=lambda v: str(v).replace(" ", ""))
def test_whole_windows_are_causal_and_a_prefix_is_the_prefix(case, W, tiled, dtype):
    Bn, L, H, hd = case
    want = _pick(dtype, hd, L, tiled)
    assert want != GENERIC
    enc = _attn_encoder(dtype, H, hd, Bn * L, tiled)
    qkv = AB.make_qkv(*case, dtype).cuda()
    causal = enc.attention(qkv, is_causal=True).clone()
    assert enc.last_attn_kernel == want
    for big in (L, L + 5):                                              # a window that holds the whole sequence: the same kernel's causal bits
        y = enc.attention(qkv, is_causal=True, window=big)
        assert enc.last_attn_kernel == want
        diff = int((_bits(y) != _bits(causal)).sum())
        assert diff == 0, f"W = {big} >= L = {L}: {diff} elements differ from is_causal=True"
    got = enc.attention(qkv, is_causal=True, window=W).clone()
    if W < L:
        assert not torch.equal(_bits(got), _bits(causal)), "the window changed nothing"
    for n in sorted({W, W + 1, 33, L - 1}):                             # the attention of a prefix is the prefix of the attention
        if not 1 <= n < L:
            continue
        pre = enc.attention(qkv[:, :n].contiguous(), is_causal=True, window=W)
        assert enc.last_attn_kernel != GENERIC
        diff = int((_bits(pre) != _bits(got[:, :n])).sum())
        assert diff == 0, f"{diff} elements of the windowed attention of the first {n} rows differ from the first {n} rows of the whole"
    enc.close()


LENGTHS = [129, 5, 33, 64, 65, 200, 1]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("hd,tiled,W", [(64, 0, 8), (64, 2, 33), (32, 1, 64), (128, 1, 100), (96, 2, 32)], ids=lambda v: str(v))
def test_ragged_batches_are_each_sequence_alone(hd, tiled, W, dtype):
    """packed sequences of a ragged batch, NaN behind the pack, sequences shorter than W (5 and 1 keys) and longer"""
    H = 2
    d = H * hd
    T = sum(LENGTHS)
    want = _pick(dtype, hd, max(LENGTHS), tiled)
    assert want != GENERIC and all(_pick(dtype, hd, n, tiled) == want for n in LENGTHS) and min(LENGTHS) < W
    enc = _attn_encoder(dtype, H, hd, T, tiled)
    seqs = [AB.make_qkv(1, n, H, hd, dtype, seed=11 + i)[0] for i, n in enumerate(LENGTHS)]
    big = torch.full((T + 64, 3 * d), float("nan"), dtype=TDT[dtype], device="cuda")
    big[:T] = torch.cat(seqs).cuda()
    obig = torch.full((64 + T + 64, d), SENTINEL, dtype=TDT[dtype], device="cuda")
    packed = enc.attention(big[:T], lengths=LENGTHS, out=obig[64:64 + T], is_causal=True, window=W)
    assert enc.last_attn_kernel == want
    torch.cuda.synchronize()
    assert torch.isfinite(packed).all() and (obig[:64] == SENTINEL).all() and (obig[64 + T:] == SENTINEL).all()
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    for i, n in enumerate(LENGTHS):
        alone = enc.attention(seqs[i].cuda().view(1, n, 3 * d), is_causal=True, window=W)
        assert enc.last_attn_kernel == want
        diff = int((_bits(alone[0]) != _bits(packed[off[i]:off[i + 1]])).sum())
        assert diff == 0, f"{dtype} hd={hd}: sequence {i} (length {n}) of the ragged windowed batch differs in {diff} elements from itself alone"
    ref, bound = W16.reference_of(seqs[5][None], H, dtype, W)
    r, where = AB.ratio(packed[off[5]:off[6]][None], ref, bound)
    print(f"{dtype} hd={hd} W={W} ragged, length {LENGTHS[5]}: err / bound {r:.3f} at {where}")
    assert r <= 1.0
    enc.close()


# ---- 3. the whole forward -----------------------------------------------------------------------------------------------------------
def _sd_t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _encoder(dims, sd, dtype, max_tokens, tiled=0, window_mfma=1):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, attn_tiled=tiled, window_mfma=window_mfma)
    enc.load_state_dict(_sd_t(sd))
    return enc


@pytest.fixture(scope="module")
def shapes():
    """tests/test_gpu_tf_window.py's: name -> (dims, state dict, x [B, L, in], W, lengths, fp64 windowed restatement of x)"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_window_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    wsd = T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)
    wx = np.random.default_rng(1).standard_normal((3, 50, 16)).astype(np.float32)
    lx = np.random.default_rng(2).standard_normal((2, 150, 16)).astype(np.float32)
    res = {"toy": (TOY, sd, f["x"], int(f["W"]), [15, 1, 7, 12, 3, 15]),
           "long": (TOY, sd, lx, 70, [150, 41]),
           "wide": (WIDE, wsd, wx, 8, [50, 1, 33])}
    return {k: v + (WB.window_forward(v[1], v[2], v[3], num_heads=v[0][3]),) for k, v in res.items()}


def _forward_kernel(enc, dims, dtype, B, L, W):
    enc.attention(torch.zeros(B, L, 3 * dims[1], dtype=TDT[dtype], device="cuda"), is_causal=True, window=W)
    return enc.last_attn_kernel


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("shape,tiled", [("toy", 0), ("wide", 0), ("wide", 2), ("long", 0)], ids=lambda v: str(v))
def test_forward(shapes, shape, tiled, dtype):
    dims, sd, x, W, lens, ref = shapes[shape]
    tol = TOL[dtype]
    B, L = x.shape[0], x.shape[1]
    hd = dims[1] // dims[3]
    xg = torch.from_numpy(x).cuda()
    fresh = _encoder(dims, sd, dtype, B * L, tiled, window_mfma=0)      # what every call returns on a handle without the option
    plain0, causal0, win0 = fresh(xg).clone(), fresh(xg, is_causal=True).clone(), fresh(xg, is_causal=True, window=W).clone()
    assert _forward_kernel(fresh, dims, dtype, B, L, W) == GENERIC
    flops0 = (fresh.flops(B, L, is_causal=True, window=W), fresh.flops(B, L, lengths=lens, is_causal=True, window=W), fresh.flops(B, L))
    fresh.close()

    enc = _encoder(dims, sd, dtype, B * L, tiled)
    want = _harness("libflope_host_tf_window16.so").tfw16_pick(DT_ID[dtype], hd, L, 0, 0, tiled, 1, 1)
    kernel = _forward_kernel(enc, dims, dtype, B, L, W)
    assert kernel == want and (kernel != GENERIC) == (shape == "wide"), kernel
    y = enc(xg, is_causal=True, window=W).clone()
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print(f"{dtype} {shape} W={W} attn_tiled={tiled} kernel {kernel}: |y - fp64|max {err:.3e}, tolerance {tol}")
    assert torch.isfinite(y).all() and err < tol
    if kernel == GENERIC:
        assert torch.equal(_bits(y), _bits(win0)), "where the pick is generic the option changes nothing"
    assert float((y - causal0).abs().max()) > 1e-3, "the window changed nothing"
    for dt in (torch.float32, torch.bool):                              # torch's spelling: the banded mask
        assert torch.equal(_bits(enc(xg, mask=WB.band_mask(L, W, dt))), _bits(y)), dt
    for big in (L, L + 5):                                              # the whole sequence: the causal forward's bits on the same kernels
        assert torch.equal(_bits(enc(xg, is_causal=True, window=big)), _bits(causal0)), big
    for n in sorted({1, W, W + 1, L - 1}):                              # the prefix property
        assert torch.equal(_bits(enc(xg[:, :n].contiguous(), is_causal=True, window=W)), _bits(y[:, :n])), n
    # ragged: NaN behind every sequence, a sequence shorter than W; each sequence is its own call's bits
    assert min(lens) < W
    xn = xg.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    yr = enc(xn, lengths=lens, is_causal=True, window=W)
    bias = torch.from_numpy(np.asarray(sd["out_layer.bias"], dtype=np.float32)).cuda()
    for b, n in enumerate(lens):
        assert torch.equal(_bits(yr[b, :n]), _bits(enc(xg[b:b + 1, :n].contiguous(), is_causal=True, window=W)[0])), b
        assert torch.equal(_bits(yr[b, :n]), _bits(y[b, :n])), b
        assert torch.equal(yr[b, n:], bias.expand(L - n, -1)), b
    # FLOPs do not depend on the option
    assert (enc.flops(B, L, is_causal=True, window=W), enc.flops(B, L, lengths=lens, is_causal=True, window=W), enc.flops(B, L)) == flops0
    # the handle is undisturbed: plain, causal, and a window_mfma = 0 windowed call afterwards
    assert torch.equal(_bits(enc(xg)), _bits(plain0))
    assert torch.equal(_bits(enc(xg, is_causal=True)), _bits(causal0))
    assert enc.set_option("window_mfma", 0) == 1
    assert torch.equal(_bits(enc(xg, is_causal=True, window=W)), _bits(win0))
    assert _forward_kernel(enc, dims, dtype, B, L, W) == GENERIC
    enc.close()


# ---- 4. stream ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("shape", ["toy", "wide"])
def test_stream(shapes, shape, dtype):
    dims, sd, x, W, lens, ref = shapes[shape]
    tol = TOL[dtype]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L)
    xg = torch.from_numpy(x).cuda()
    kernel = _forward_kernel(enc, dims, dtype, B, L, W)
    assert (kernel == MFMA64) == (shape == "wide") and kernel in (GENERIC, MFMA64)
    want = enc(xg, is_causal=True, window=W).clone()
    st = enc.open_stream(B, W + 3, window=W)
    half = [max(1, n // 2) for n in lens]
    enc(xg[:1, :1].contiguous())                                       # states causal = 0, window = 0
    pre = st.prefill(xg, lengths=half)
    assert enc.set_option("window", 0) == 0 and enc.set_option("causal", 0) == 0 and enc.set_option("window_mfma", 1) == 1
    assert torch.equal(_bits(pre), _bits(enc(xg, lengths=half, is_causal=True, window=W))), "prefill is the ragged windowed forward"
    assert st.positions == half
    worst = 0.0
    for t in range(min(half), L):
        rows = [b for b in range(B) if half[b] <= t < lens[b]]
        if not rows:
            continue
        y = st.step(torch.stack([xg[b, t] for b in rows]), rows)
        worst = max(worst, float(np.abs(y.cpu().numpy() - np.stack([ref[b, t] for b in rows])).max()))
        if kernel == GENERIC:                                           # DESIGN.md 25's rule: bits where the forward's attention is generic
            assert torch.equal(_bits(y), _bits(torch.stack([want[b, t] for b in rows]))), f"step {t} behind the prefill"
    print(f"{dtype} {shape} W={W} forward kernel {kernel}: steps behind a prefill |y - fp64|max {worst:.3e}, tolerance {tol}")
    assert worst < tol and st.positions == lens
    st.close(); enc.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(shapes):
    from flope_amd import _lib
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, x, W, lens, ref = shapes["wide"]
    for bad in (2, -1):
        with pytest.raises(ValueError, match="window_mfma must be 0 or 1"):
            TransformerEncoder(*dims, dtype="f16", max_tokens=64, window_mfma=bad)
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, "f16", B * L)
    xg = torch.from_numpy(x).cuda()
    want = enc(xg, is_causal=True, window=W).clone()
    assert enc.set_option("window_mfma", 3) == _lib.EINVAL and "window_mfma is 0 or 1" in enc.lib.flope_tf_last_error(enc.handle).decode()
    assert enc.set_option("window_mfma", 1) == 1, "a refused value changed the option"
    q = torch.zeros(1, 40, 3 * dims[1], dtype=torch.float16, device="cuda")
    for call, msg in [(lambda: enc(xg, window=W), r"window=8 needs is_causal=True"),
                      (lambda: enc.attention(q, window=2), r"window=2 needs is_causal=True"),
                      (lambda: enc(xg, is_causal=True, window=-2), r"window must be 0 \(none\) or a positive")]:
        with pytest.raises(ValueError, match=msg):
            call()
    enc.set_option("causal", 0)                                         # the C entry points refuse the pair themselves
    assert enc.set_option("window", 3) >= 0
    a = torch.full((1, 40, dims[1]), SENTINEL, dtype=torch.float16, device="cuda")
    assert enc.lib.flope_tf_attention(enc.handle, q.data_ptr(), 1, 40, a.data_ptr(), None) == _lib.EINVAL
    assert "window = 3 needs option causal = 1" in enc.lib.flope_tf_last_error(enc.handle).decode()
    y = torch.full((B, L, dims[2]), SENTINEL, device="cuda")
    assert enc.lib.flope_tf_forward(enc.handle, xg.data_ptr(), B, L, y.data_ptr(), None) == _lib.EINVAL
    torch.cuda.synchronize()
    assert (a == SENTINEL).all() and (y == SENTINEL).all(), "a refused call wrote"
    assert enc.set_option("window", 0) == 3
    got = enc(xg, is_causal=True, window=W)                             # the next valid call
    assert torch.equal(_bits(got), _bits(want))
    err = float(np.abs(got.cpu().numpy() - ref).max())
    assert err < TOL["f16"]
    enc.close()
