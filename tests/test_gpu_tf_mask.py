"""Any [L, L] attention mask, compiled once, on the device (enc.make_mask, forward / attention(..., mask=<compiled>)).

The contract: a compiled mask runs tf_attn_masked for every dtype and shape -- the generic kernel's order over the allowed keys -- so
wherever the mask says what one of the dedicated kernels can say (all-clear, causal, a causal band, block-diagonal = ragged), the
result is that kernel's IN BITS wherever it is tf_attn_generic; a masked key is never loaded; every other mask is held element-wise
to fp64 within the bound of tests/tf_attn_mask_bound.py, and the whole forward to DESIGN.md 24's tolerances: 2e-4 (f32, f32m), 1.5e-2
(f16), 1.2e-1 (bf16).  Shapes are the smallest at which the walk can go wrong: L 1 / 15 / 33 / 65 / 130 (one key; inside a word; one
bit into the second word; one key into the second 64-key trip; a third trip), head_dim 6 (element-wise loads) and 64, and the edge
mask's rows: first key 31 / 32 / 63 / 64 / 65, only key L - 1, only key 0, a trip without a key between two that have some.

  ODD   (5, 30, 3, 5, 1, 20)      head_dim 6, one layer
  TOY   (16, 32, 9, 4, 2, 64)     the reference fixture's dims
  WIDE  (16, 128, 9, 2, 2, 256)   head_dim 64: a 16-bit forward whose unmasked attention is tf_attn_mfma

  1. bit contracts   2. masked keys are never loaded   3. against fp64   4. ragged   5. state   6. refusals
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tf_attn_mask_bound as MB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = MB.TDT
GENERIC, MFMA64, MASKED = 0, 1, 4
EINVAL, ESTATE = -1, -3
SENTINEL = 1234.0
ODD = (5, 30, 3, 5, 1, 20)
TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)
DIMS = {"odd": ODD, "toy": TOY, "wide": WIDE}
MODES = [("f32", 2e-4), ("f32m", 2e-4), ("f16", 1.5e-2), ("bf16", 1.2e-1)]
BANDS = (1, 4, 64, 70)
BLOCKS = [4, 1, 33, 65, 27]              # sum 130: blocks that end inside a word, at bit 4 / 5, across two words and a trip


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _sd_t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _encoder(dims, sd, dtype, max_tokens, fused=0, generic=0):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, fused=fused)
    if sd is not None:
        enc.load_state_dict(_sd_t(sd))
    if generic:
        enc.set_option("generic", 1)
    return enc


@pytest.fixture(scope="module")
def sds():
    """name -> state dict; computed once, never changed"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_mask_fixture.npz"))
    return {"toy": {k[4:]: f[k] for k in f.files if k.startswith("sd::")},
            "odd": T.synthetic_state_dict(ODD[0], ODD[1], ODD[2], ODD[4], ODD[5], seed=3),
            "wide": T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)}


def _x(B, L, in_dim, seed=1):
    return torch.from_numpy(np.random.default_rng(seed * 1000 + L).standard_normal((B, L, in_dim)).astype(np.float32))


# ---- 1. bit contracts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", ["odd", "wide"])
def test_masks_the_dedicated_kernels_can_say_are_their_bits(sds, shape, dtype):
    """all-clear = enc(x), causal = is_causal, band W = window W: at enc.attention and at the whole forward"""
    dims = DIMS[shape]
    enc = _encoder(dims, sds[shape], dtype, 2 * 130, generic=int(shape == "wide" and dtype != "f32"))
    d = dims[1]
    n = 0
    for L in MB.LENGTHS:
        x = _x(2, L, dims[0]).cuda()
        qkv = MB.make_qkv(2, L, dims[3], d // dims[3], dtype).cuda()
        cases = [("clear", MB.make_allowed("clear", L), dict()), ("causal", MB.make_allowed("causal", L), dict(is_causal=True))]
        cases += [(f"band {W}", MB.band_causal(L, W), dict(is_causal=True, window=W)) for W in BANDS]
        for name, allowed, kw in cases:
            m = enc.make_mask(MB.to_torch_mask(allowed, floating=(n % 2 == 1)).to("cuda" if n % 3 == 0 else "cpu"))
            assert (m.L, m.allowed) == (L, int(allowed.sum()))
            want = enc.attention(qkv, **kw).clone()
            assert enc.last_attn_kernel == GENERIC, "the comparison is with tf_attn_generic"
            got = enc.attention(qkv, mask=m)
            assert enc.last_attn_kernel == MASKED
            assert torch.equal(_bits(got), _bits(want)), (name, L, "attention")
            want = enc(x, **kw).clone()
            got = enc(x, mask=m)
            assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), (name, L, "forward")
            m.close()
            n += 1
    assert n == 30


@pytest.mark.parametrize("causal", [False, True], ids=["blocks", "causal blocks"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", ["odd", "wide"])
def test_block_diagonal_is_the_ragged_batch(sds, shape, dtype, causal):
    """sequences concatenated at B = 1 under a block-diagonal mask = the valid rows of the padded batch with lengths"""
    dims = DIMS[shape]
    T, Lp = sum(BLOCKS), max(BLOCKS)
    enc = _encoder(dims, sds[shape], dtype, len(BLOCKS) * Lp, generic=int(shape == "wide" and dtype != "f32"))
    m = enc.make_mask(MB.to_torch_mask(MB.block_diagonal(BLOCKS, causal)))
    assert m.allowed == sum(n * (n + 1) // 2 if causal else n * n for n in BLOCKS)
    # attention: the packed rows are the concatenation
    qkv = MB.make_qkv(1, T, dims[3], dims[1] // dims[3], dtype).cuda()
    want = enc.attention(qkv[0], lengths=BLOCKS, is_causal=causal).clone()
    assert enc.last_attn_kernel == GENERIC
    got = enc.attention(qkv, mask=m)
    assert enc.last_attn_kernel == MASKED and torch.equal(_bits(got[0]), _bits(want))
    # the forward
    xc = _x(1, T, dims[0]).cuda()
    xp = torch.full((len(BLOCKS), Lp, dims[0]), float("nan"), device="cuda")
    o = 0
    for b, n in enumerate(BLOCKS):
        xp[b, :n] = xc[0, o:o + n]
        o += n
    want = enc(xp, lengths=BLOCKS, is_causal=causal).clone()
    got = enc(xc, mask=m)
    o = 0
    for b, n in enumerate(BLOCKS):
        assert torch.equal(_bits(got[0, o:o + n]), _bits(want[b, :n])), b
        o += n
    assert torch.isfinite(got).all()
    assert enc.flops(1, T, mask=m) == enc.flops(len(BLOCKS), Lp, lengths=BLOCKS, is_causal=causal)


# ---- 2. masked keys are never loaded ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("hd", MB.HEAD_DIMS)
def test_keys_no_query_allows_may_hold_nan(dtype, hd):
    H, L = 2, 65
    d = H * hd
    enc = _encoder((5, d, 3, H, 1, 20), None, dtype, 2 * L)
    dead = [0, 3, 31, 32, 63, 64]                                            # word and trip boundaries among them
    allowed = MB.make_allowed("random", L).clone()
    allowed[:, dead] = False
    allowed[:, 1] = True                                                     # every row keeps a key
    m = enc.make_mask(~allowed)
    qkv = MB.make_qkv(2, L, H, hd, dtype).cuda()
    clean = enc.attention(qkv, mask=m).clone()
    bad = qkv.clone()
    bad[:, dead, d:] = float("nan")                                          # k and v of the dead keys; their q rows stay queries
    got = enc.attention(bad, mask=m)
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(clean))
    ref, bound = MB.reference_of(qkv, allowed, H, dtype)
    r, at = MB.ratio(clean, ref, bound)
    assert r < 1.0, (r, at)
    bad[:, dead, d:] = float("inf")
    assert torch.equal(_bits(enc.attention(bad, mask=m)), _bits(clean))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_padding_rows_under_lengths_may_hold_nan(sds, dtype):
    L, lens = 33, [33, 1, 20]
    enc = _encoder(TOY, sds["toy"], dtype, 3 * L)
    m = enc.make_mask(~MB.make_allowed("prefix", L))
    x = _x(3, L, TOY[0]).cuda()
    clean = enc(x, lengths=lens, mask=m).clone()
    xn = x.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    got = enc(xn, lengths=lens, mask=m)
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(clean))
    pad = torch.tensor([[n <= i for i in range(L)] for n in lens])
    assert torch.equal(_bits(enc(xn, src_key_padding_mask=pad, mask=m)), _bits(clean))
    # the packed attention rows: a sequence's keys end at its own length, the next sequence's rows are not its keys
    d = TOY[1]
    qkv = MB.make_qkv(1, sum(lens), TOY[3], d // TOY[3], dtype).cuda()[0]
    out = enc.attention(qkv, lengths=lens, mask=m)
    o = 0
    for n in lens:
        mm = enc.make_mask(~MB.make_allowed("prefix", L)[:n, :n])
        assert torch.equal(_bits(out[o:o + n]), _bits(enc.attention(qkv[o:o + n][None].contiguous(), mask=mm)[0])), n
        o += n


# ---- 3. random, prefix-LM, +-k band and edge masks against fp64 ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("hd", MB.HEAD_DIMS)
def test_attention_within_the_derived_bound(dtype, hd):
    H = 2
    enc = _encoder((5, H * hd, 3, H, 1, 20), None, dtype, 2 * 130)
    worst = (0.0, ("", 0))
    for kind in MB.KINDS:
        for L in MB.LENGTHS:
            m = enc.make_mask(~MB.make_allowed(kind, L))
            got = enc.attention(MB.make_qkv(2, L, H, hd, dtype).cuda(), mask=m)
            assert enc.last_attn_kernel == MASKED
            ref, bound = MB.reference(kind, 2, L, H, hd, dtype)
            r, at = MB.ratio(got, ref, bound)
            print(f"{dtype} head_dim {hd} {kind} L={L}: {r:.3f} of the bound at {at}")
            assert r < 1.0, (kind, L, r, at)
            worst = max(worst, (r, (kind, L)))
            m.close()
    print(f"{dtype} head_dim {hd}: worst {worst[0]:.3f} of the bound at {worst[1]} (headroom {1 / max(worst[0], 1e-9):.1f}x)")


@pytest.fixture(scope="module")
def forward_refs(sds):
    """(shape, kind) -> (x, allowed, fp64 restatement); computed once, never changed"""
    out = {}
    for shape, L in (("toy", 33), ("wide", 65)):
        x = _x(2, L, DIMS[shape][0], seed=2)
        for kind in MB.KINDS:
            allowed = MB.make_allowed(kind, L)
            out[shape, kind] = (x, allowed, MB.masked_forward(sds[shape], x.numpy(), allowed.numpy(), num_heads=DIMS[shape][3]))
    return out


@pytest.mark.parametrize("shape", ["toy", "wide"])
@pytest.mark.parametrize("dtype,tol", MODES, ids=lambda v: str(v))
def test_forward_against_the_restatement(sds, forward_refs, shape, dtype, tol):
    dims = DIMS[shape]
    L = forward_refs[shape, "random"][0].shape[1]
    enc = _encoder(dims, sds[shape], dtype, 2 * L)
    enc.attention(torch.zeros(2, L, 3 * dims[1], dtype=TDT[dtype], device="cuda"))
    unmasked = enc.last_attn_kernel
    if shape == "wide":
        assert unmasked == {"f32": GENERIC, "f32m": 3, "f16": MFMA64, "bf16": MFMA64}[dtype], "the masked forward leaves these for tf_attn_masked"
    for kind in MB.KINDS:
        x, allowed, ref = forward_refs[shape, kind]
        m = enc.make_mask(~allowed)
        y = enc(x.cuda(), mask=m)
        err = float(np.abs(y.cpu().numpy() - ref).max())
        print(f"{dtype} {shape} {kind} L={L}: |y - fp64|max {err:.3e}, tolerance {tol}")
        assert torch.isfinite(y).all() and err < tol, (kind, err)
        assert enc.forward_plan(2, L, mask=m) == "launches" and not enc.last_forward_fused
        enc.attention(torch.zeros(2, L, 3 * dims[1], dtype=TDT[dtype], device="cuda"), mask=m)
        assert enc.last_attn_kernel == MASKED


def test_reference_fixture(sds):
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_mask_fixture.npz"))
    enc = _encoder(TOY, sds["toy"], "f32", 6 * 15, fused=1)
    x = torch.from_numpy(f["x"]).cuda()
    for name in ("random", "blocks", "prefix"):
        mask = torch.from_numpy(f["mask_" + name])
        y = enc(x, mask=enc.make_mask(mask))
        err = float(np.abs(y.cpu().numpy() - f["y_" + name]).max())
        print(f"f32 toy vs the reference module under the {name} mask: {err:.3e}")
        assert err < 1e-5 and not enc.last_forward_fused
        fm = torch.zeros(15, 15).masked_fill(mask, float("-inf"))
        assert torch.equal(_bits(enc(x, mask=enc.make_mask(fm.cuda()))), _bits(y)), "the float spelling"


# ---- 4. ragged ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("kind", ["prefix", "band", "random"])
def test_each_sequence_is_itself_alone_under_the_corner(sds, dtype, kind):
    L, lens = 65, [65, 1, 33, 20, 64]
    enc = _encoder(TOY, sds["toy"], dtype, sum(lens))
    allowed = MB.make_allowed(kind, L)
    m = enc.make_mask(~allowed)
    x = _x(len(lens), L, TOY[0]).cuda()
    y = enc(x, lengths=lens, mask=m).clone()
    bias = torch.from_numpy(np.asarray(sds["toy"]["out_layer.bias"], dtype=np.float32)).cuda()
    for b, n in enumerate(lens):
        alone = enc(x[b:b + 1, :n].contiguous(), mask=enc.make_mask(~allowed[:n, :n]))
        assert torch.equal(_bits(y[b, :n]), _bits(alone[0])), b
        assert torch.equal(y[b, n:], bias.expand(L - n, -1)), b
    ref = MB.masked_forward(sds["toy"], x.cpu().numpy(), allowed.numpy(), lens)
    assert float(np.abs(y.cpu().numpy() - ref).max()) < dict(MODES)[dtype]
    want = enc.flops(len(lens), L, lengths=lens, mask=m)
    pairs = sum(int(allowed[:n, :n].sum()) for n in lens)
    i, d, o, H, nl, ff = TOY
    M = sum(lens)
    assert want == 2.0 * (M * i * d + M * d * o + nl * (M * d * 3 * d + M * d * d + 2.0 * M * d * ff + 2.0 * pairs * d))


def test_length_whose_corner_leaves_a_row_without_keys(sds):
    L = 33
    enc = _encoder(TOY, sds["toy"], "f32", 3 * L)
    allowed = MB.make_allowed("edge", L)                                     # row 0 sees key L - 1 only, row 32 sees key 32 only
    m = enc.make_mask(~allowed)
    x = _x(3, L, TOY[0]).cuda()
    good = enc(x, mask=m).clone()
    y = torch.full((3, L, TOY[2]), SENTINEL, device="cuda")
    with pytest.raises(ValueError, match=r"b = 1, row 0 has no allowed key below 20"):
        enc(x, lengths=[33, 20, 33], mask=m)
    with pytest.raises(ValueError, match=r"b = 2, row 0"):
        enc.attention(torch.zeros(33 + 33 + 5, 3 * TOY[1], device="cuda"), lengths=[33, 33, 5], mask=m)
    rc = enc.lib.flope_tf_forward_masked(enc.handle, x.data_ptr(), 3, L, (C.c_int * 3)(33, 20, 33), m.handle, y.data_ptr(), None)
    assert rc == EINVAL and bool((y == SENTINEL).all()), "refused before anything is enqueued"
    assert torch.equal(_bits(enc(x, mask=m)), _bits(good)), "the next valid call"
    assert torch.equal(_bits(enc(x, lengths=[33, 33, 33], mask=m)), _bits(good))


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------
def test_other_forwards_keep_their_bits_around_masked_calls(sds):
    L = 15
    enc = _encoder(TOY, sds["toy"], "f32", 6 * L, fused=1)
    x = _x(6, L, TOY[0]).cuda()
    ma, mb = enc.make_mask(~MB.make_allowed("random", L)), enc.make_mask(~MB.make_allowed("prefix", L))
    calls = [dict(), dict(is_causal=True), dict(is_causal=True, window=4), dict(lengths=[15, 1, 7, 12, 3, 15])]
    before, fused = [], []
    for kw in calls:
        before.append(enc(x, **kw).clone())
        fused.append(enc.last_forward_fused)
    assert fused[0] and fused[1] and not fused[2], "plain and causal are the single launch here, a window never is"
    ya, yb = enc(x, mask=ma).clone(), enc(x, mask=mb).clone()
    assert float((ya - yb).abs().max()) > 1e-3
    for kw, want, fz in zip(calls, before, fused):
        for m, ym in ((ma, ya), (mb, yb), (ma, ya)):                          # two masks on one handle, alternately
            assert torch.equal(_bits(enc(x, mask=m)), _bits(ym))
            assert not enc.last_forward_fused
        assert torch.equal(_bits(enc(x, **kw)), _bits(want)), kw
        assert enc.last_forward_fused == fz, kw
    # options "causal" / "window" are neither read nor written by a masked call
    enc(x, is_causal=True, window=4)
    enc(x, mask=ma)
    enc.attention(torch.zeros(6, L, 3 * TOY[1], device="cuda"), mask=mb)
    assert enc.last_attn_kernel == MASKED
    assert enc.lib.flope_tf_last_forward(enc.handle) == 0
    assert enc.set_option("window", 4) == 4 and enc.set_option("causal", 1) == 1
    enc(x)
    enc(x, mask=ma)
    assert enc.set_option("causal", 0) == 0 and enc.set_option("window", 0) == 0
    assert enc.last_forward_fused is False and enc(x) is not None and enc.last_forward_fused is True
    mb.close()
    assert torch.equal(_bits(enc(x, mask=ma)), _bits(ya)), "closing one mask leaves the other"


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_make_mask_refusals(sds):
    enc = _encoder(TOY, sds["toy"], "f32", 64)
    for bad in (torch.zeros(3, 4, dtype=torch.bool), torch.zeros(2, 3, 3, dtype=torch.bool), torch.zeros(3, 3, dtype=torch.int32),
                torch.zeros(0, 0, dtype=torch.bool)):
        with pytest.raises(ValueError, match="mask must be"):
            enc.make_mask(bad)
    f = torch.zeros(5, 5)
    f[3, 2] = -1.5
    with pytest.raises(ValueError, match=r"mask\[3, 2\] = -1.5"):
        enc.make_mask(f)
    f[3, 2] = float("nan")
    with pytest.raises(ValueError, match=r"mask\[3, 2\]"):
        enc.make_mask(f)
    b = torch.zeros(5, 5, dtype=torch.bool)
    b[2] = True
    with pytest.raises(ValueError, match="row 2 has no allowed key"):
        enc.make_mask(b)
    with pytest.raises(ValueError, match="row 2 has no allowed key"):
        enc.make_mask(torch.zeros(5, 5).masked_fill(b, float("-inf")))
    with pytest.raises(ValueError, match="max_tokens"):
        enc.make_mask(torch.zeros(65, 65, dtype=torch.bool))
    # the C entry point itself
    lib, out = enc.lib, C.c_void_p()
    one = (C.c_uint32 * 2)(1, 0)
    assert lib.flope_tf_mask_create(enc.handle, 1, None, C.byref(out)) == EINVAL
    assert lib.flope_tf_mask_create(enc.handle, 1, one, None) == EINVAL
    assert lib.flope_tf_mask_create(enc.handle, 0, one, C.byref(out)) == EINVAL
    assert lib.flope_tf_mask_create(enc.handle, 65, one, C.byref(out)) == EINVAL
    assert lib.flope_tf_mask_create(enc.handle, 1, (C.c_uint32 * 1)(3), C.byref(out)) == EINVAL       # a padding bit: column 1 of L = 1
    assert b"padding bit set in row 0, column 1" in lib.flope_tf_last_error(enc.handle)
    assert lib.flope_tf_mask_create(enc.handle, 2, (C.c_uint32 * 2)(1, 0), C.byref(out)) == EINVAL     # row 1 without a key
    assert b"row 1 has no allowed key" in lib.flope_tf_last_error(enc.handle) and not out.value
    assert lib.flope_tf_mask_create(enc.handle, 1, one, C.byref(out)) == 0 and out.value
    n, pairs = C.c_int(), C.c_longlong()
    assert lib.flope_tf_mask_info(out, C.byref(n), C.byref(pairs)) == 0 and (n.value, pairs.value) == (1, 1)
    assert lib.flope_tf_mask_info(out, None, None) == 0
    assert lib.flope_tf_mask_destroy(out) == 0


def test_call_refusals_leave_the_buffers_alone(sds):
    L = 15
    enc = _encoder(TOY, sds["toy"], "f32", 4 * L)
    other = _encoder(TOY, sds["toy"], "f32", 4 * L)
    m, mo = enc.make_mask(~MB.make_allowed("prefix", L)), other.make_mask(~MB.make_allowed("prefix", L))
    x = _x(4, L, TOY[0]).cuda()
    qkv = torch.zeros(4, L, 3 * TOY[1], device="cuda")
    for kw in (dict(is_causal=True), dict(window=3), dict(is_causal=True, window=3)):
        with pytest.raises(ValueError, match="say it in the mask"):
            enc(x, mask=m, **kw)
        with pytest.raises(ValueError, match="say it in the mask"):
            enc.attention(qkv, mask=m, **kw)
    with pytest.raises(ValueError, match="another encoder"):
        enc(x, mask=mo)
    with pytest.raises(ValueError, match="15 tokens, this call has 14"):
        enc(x[:, :14].contiguous(), mask=m)
    with pytest.raises(ValueError, match="differs from the mask's"):
        enc.attention(qkv[:, :14].contiguous(), mask=m)
    with pytest.raises(ValueError, match=r"lengths\[2\] = 16"):
        enc(x, lengths=[15, 1, 16, 2], mask=m)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 0"):
        enc(x, lengths=[15, 0, 1, 2], mask=m)
    with pytest.raises(ValueError, match="max_tokens"):
        enc(torch.cat([x, x[:1]]), mask=m)
    with pytest.raises(ValueError, match="max_tokens"):
        enc.attention(torch.zeros(5 * L, 3 * TOY[1], device="cuda"), lengths=[L] * 5, mask=m)
    with pytest.raises(ValueError, match="compiled mask"):
        enc.attention(qkv, mask=~MB.make_allowed("prefix", L))
    with pytest.raises(ValueError):
        enc.flops(4, 14, mask=m)
    with pytest.raises(ValueError):
        enc.forward_plan(4, L, mask=m, is_causal=True)
    # the C entry points, with sentinels around y and out
    lib = enc.lib
    ybuf = torch.full((4 * L + 2, TOY[2]), SENTINEL, device="cuda")
    obuf = torch.full((4 * L + 2, TOY[1]), SENTINEL, device="cuda")
    y, out = ybuf[1:-1], obuf[1:-1]
    fwd = lambda h, xp, B, Ls, lens, mh, yp: lib.flope_tf_forward_masked(h, xp, B, Ls, lens, mh, yp, None)
    att = lambda h, qp, B, Ls, lens, mh, op: lib.flope_tf_attention_masked(h, qp, B, Ls, lens, mh, op, None)
    for call, src, dst in ((fwd, x, y), (att, qkv, out)):
        assert call(enc.handle, None, 4, L, None, m.handle, dst.data_ptr()) == EINVAL
        assert call(enc.handle, src.data_ptr(), 4, L, None, m.handle, None) == EINVAL
        assert call(enc.handle, src.data_ptr(), 4, L, None, None, dst.data_ptr()) == EINVAL
        assert call(enc.handle, src.data_ptr(), 0, L, None, m.handle, dst.data_ptr()) == EINVAL
        assert call(enc.handle, src.data_ptr(), 4, 14, None, m.handle, dst.data_ptr()) == EINVAL
        assert call(enc.handle, src.data_ptr(), 5, L, None, m.handle, dst.data_ptr()) == EINVAL
        assert call(enc.handle, src.data_ptr(), 4, L, None, mo.handle, dst.data_ptr()) == EINVAL
        assert b"another handle" in lib.flope_tf_last_error(enc.handle)
        assert call(enc.handle, src.data_ptr(), 2, L, (C.c_int * 2)(15, 16), m.handle, dst.data_ptr()) == EINVAL
        assert call(enc.handle, src.data_ptr(), 2, L, (C.c_int * 2)(0, 3), m.handle, dst.data_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((ybuf == SENTINEL).all()) and bool((obuf == SENTINEL).all()), "a refused call wrote something"
    assert fwd(enc.handle, x.data_ptr(), 4, L, None, m.handle, y.data_ptr()) == 0
    assert att(enc.handle, qkv.data_ptr(), 4, L, None, m.handle, out.data_ptr()) == MASKED
    torch.cuda.synchronize()
    for buf in (ybuf, obuf):
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()) and not bool((buf[1:-1] == SENTINEL).any())
    assert torch.equal(_bits(y.reshape(4, L, -1)), _bits(enc(x, mask=m)))
    # a plain arbitrary tensor is refused as it always was
    with pytest.raises(ValueError, match="has a kernel"):
        enc(x, mask=~MB.make_allowed("prefix", L))
    with pytest.raises(ValueError, match="has a kernel"):
        enc(x, mask=~MB.make_allowed("random", L))


def test_closed_mask_and_closed_encoder(sds):
    L = 15
    enc = _encoder(TOY, sds["toy"], "f32", L)
    x = _x(1, L, TOY[0]).cuda()
    m, keep = enc.make_mask(~MB.make_allowed("band", L)), enc.make_mask(~MB.make_allowed("random", L))
    enc(x, mask=m)
    m.close()
    m.close()
    with pytest.raises(RuntimeError, match="mask has been closed"):
        enc(x, mask=m)
    with pytest.raises(RuntimeError, match="mask has been closed"):
        enc.attention(torch.zeros(1, L, 3 * TOY[1], device="cuda"), mask=m)
    handle = keep.handle
    lib = enc.lib
    enc.close()
    with pytest.raises(RuntimeError, match="encoder of this mask has been closed"):
        enc(x, mask=keep)
    with pytest.raises(RuntimeError, match="closed"):
        enc.make_mask(~MB.make_allowed("band", L))
    assert lib.flope_tf_mask_info(handle, None, None) == ESTATE                # the masks ended with the handle
    other = _encoder(TOY, sds["toy"], "f32", L)
    y = torch.full((1, L, TOY[2]), SENTINEL, device="cuda")
    assert lib.flope_tf_forward_masked(other.handle, x.data_ptr(), 1, L, None, handle, y.data_ptr(), None) == ESTATE
    assert bool((y == SENTINEL).all())
    keep.close()                                                             # frees the host part only
