"""A compiled [L, L] mask on the 16-bit MFMA attention, on the device (option "mask_mfma", tf_attn_tiled_masked).

The contract: with mask_mfma = 1 a 16-bit masked launch at head_dim 32 / 64 / 96 / 128 walks tf_attn_tiled's ring and step over the key
blocks of the mask's tile map.  Where the mask says what tf_attn_tiled can say itself -- all-clear, causal, a causal band (window_mfma =
1), block-diagonal at multiples of 32 = a ragged batch -- the result is tf_attn_tiled's IN BITS, at enc.attention and at the whole
forward; a sequence of a ragged batch is that sequence alone, in bits; a key no query allows may hold NaN; every other mask is held
element-wise to fp64 within the bound of tests/tf_attn_mask16_bound.py and the whole forward to 1.5e-2 (f16) / 1.2e-1 (bf16) of
tests/tf_attn_mask_bound.masked_forward.  Option 0, generic = 1, float32 handles and other head_dims keep tf_attn_masked.

One model per head_dim, d = 2 head_dim, two heads, two layers (head_dim 128: one).  Lengths 1 / 33 / 65 / 129 / 257: one key; one key
into a second step; into a second block; a ring stage used twice; a second and a third query block.

  1. bit contracts   2. keys no query allows   3. against fp64   4. ragged   5. state and ids   6. refusals
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tf_attn_mask16_bound as M16
import tf_attn_mask_bound as MB

pytestmark = pytest.mark.gpu

TDT = MB.TDT
GENERIC, MFMA64, TILED, MASKED, MASKED16 = 0, 1, 2, 4, 5
EINVAL = -1
SENTINEL = 1234.0
TOL = {"f16": 1.5e-2, "bf16": 1.2e-1}
DTYPES = ["f16", "bf16"]
H = 2
BANDS = (1, 33, 100)
PACKED = [4, 1, 33, 65, 27]              # blocks at offsets that are no multiples of 32: another grouping of the keys, held to the bound


def _dims(hd):
    return (7, H * hd, 5, H, 1 if hd == 128 else 2, 2 * hd)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


_SD = {}


def _sd(hd):
    if hd not in _SD:
        from oracle import tf_encoder_ref as T
        i, d, o, _, nl, ff = _dims(hd)
        _SD[hd] = T.synthetic_state_dict(i, d, o, nl, ff, seed=hd)
    return _SD[hd]


def _encoder(hd, dtype, max_tokens=1024, weights=True, **kw):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*_dims(hd), dtype=dtype, max_tokens=max_tokens, **kw)
    if weights:
        enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in _sd(hd).items()})
    return enc


def _x(B, L, in_dim=7, seed=1):
    return torch.from_numpy(np.random.default_rng(seed * 1000 + L).standard_normal((B, L, in_dim)).astype(np.float32))


def _at32(blocks, causal=False):
    """The blocks laid out at B = 1 with every block starting at a multiple of 32: the rows between a block's end and the next multiple
    of 32 are blocks of one row each (a row needs a key), so the mask stays block-diagonal.  -> (allowed [T, T], the blocks' offsets)"""
    offs, o = [], 0
    for n in blocks:
        offs.append(o)
        o = (o + n + 31) // 32 * 32
    T = offs[-1] + blocks[-1]
    a = torch.eye(T, dtype=torch.bool)
    for o, n in zip(offs, blocks):
        a[o:o + n, o:o + n] = torch.ones(n, n, dtype=torch.bool).tril() if causal else True
    return a, offs


# ---- 1. bit contracts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", M16.HEAD_DIMS)
def test_masks_tf_attn_tiled_can_say_are_its_bits(hd, dtype):
    """all-clear = enc(x), causal = is_causal, causal band W = window W under window_mfma = 1: at enc.attention and at the forward"""
    enc = _encoder(hd, dtype, attn_tiled=2, window_mfma=1, mask_mfma=1)
    n = 0
    for L in M16.LENGTHS:
        x = _x(2, L).cuda()
        qkv = MB.make_qkv(2, L, H, hd, dtype).cuda()
        cases = [("clear", MB.make_allowed("clear", L), dict()), ("causal", MB.make_allowed("causal", L), dict(is_causal=True))]
        cases += [(f"band {W}", MB.band_causal(L, W), dict(is_causal=True, window=W)) for W in BANDS]
        for name, allowed, kw in cases:
            m = enc.make_mask(MB.to_torch_mask(allowed, floating=(n % 2 == 1)))
            assert m.tile_stats == M16.tile_stats(allowed.numpy()), (name, L)
            want = enc.attention(qkv, **kw).clone()
            assert enc.last_attn_kernel == TILED, "the comparison is with tf_attn_tiled"
            got = enc.attention(qkv, mask=m)
            assert enc.last_attn_kernel == MASKED16
            assert torch.isfinite(got.float()).all() and torch.equal(_bits(got), _bits(want)), (name, L, "attention")
            want = enc(x, **kw).clone()
            got = enc(x, mask=m)
            assert enc.last_attn_kernel == MASKED16, "the forward records the kernel of its attention launches"
            assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), (name, L, "forward")
            m.close()
            n += 1
    assert n == 25


@pytest.mark.parametrize("causal", [False, True], ids=["blocks", "causal blocks"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blocks,hd", [([32, 64, 33], 32), ([32, 64, 33], 64), ([128, 1, 96, 32], 96), ([128, 1, 96, 32], 128)], ids=str)
def test_block_diagonal_at_multiples_of_32_is_the_ragged_batch(blocks, hd, dtype, causal):
    """sequences laid out at B = 1, each starting at a multiple of 32, under the block-diagonal mask = the valid rows of the padded batch
    with lengths: a key keeps its place in its 32-key step, and a query's state depends on its own row and that grouping alone"""
    allowed, offs = _at32(blocks, causal)
    T, Lp = allowed.shape[0], max(blocks)
    enc = _encoder(hd, dtype, attn_tiled=2, mask_mfma=1)
    m = enc.make_mask(~allowed)
    qkv = MB.make_qkv(1, T, H, hd, dtype).cuda()
    packed = torch.cat([qkv[0, o:o + n] for o, n in zip(offs, blocks)]).contiguous()
    want = enc.attention(packed, lengths=blocks, is_causal=causal).clone()
    assert enc.last_attn_kernel == TILED
    got = enc.attention(qkv, mask=m)
    assert enc.last_attn_kernel == MASKED16 and torch.isfinite(got.float()).all()
    r = 0
    for o, n in zip(offs, blocks):
        assert torch.equal(_bits(got[0, o:o + n]), _bits(want[r:r + n])), (o, n, "attention")
        r += n
    xc = _x(1, T).cuda()
    xp = torch.full((len(blocks), Lp, 7), float("nan"), device="cuda")
    for b, (o, n) in enumerate(zip(offs, blocks)):
        xp[b, :n] = xc[0, o:o + n]
    want = enc(xp, lengths=blocks, is_causal=causal).clone()
    got = enc(xc, mask=m)
    assert torch.isfinite(got).all()
    for b, (o, n) in enumerate(zip(offs, blocks)):
        assert torch.equal(_bits(got[0, o:o + n]), _bits(want[b, :n])), (b, "forward")


@pytest.mark.parametrize("dtype", DTYPES)
def test_blocks_at_other_offsets_are_within_the_bound(dtype):
    hd, T = 64, sum(PACKED)
    allowed = MB.block_diagonal(PACKED)
    enc = _encoder(hd, dtype, attn_tiled=2, mask_mfma=1)
    m = enc.make_mask(~allowed)
    qkv = MB.make_qkv(1, T, H, hd, dtype)
    got = enc.attention(qkv.cuda(), mask=m)
    assert enc.last_attn_kernel == MASKED16
    r, at = M16.ratio(got, *M16.reference_of(qkv, allowed, H, dtype))
    print(f"{dtype} blocks {PACKED}: {r:.3f} of the bound at {at}")
    assert r < 1.0, (r, at)
    x = _x(1, T)
    err = float(np.abs(enc(x.cuda(), mask=m).cpu().numpy() - MB.masked_forward(_sd(hd), x.numpy(), allowed.numpy(), num_heads=H)).max())
    print(f"{dtype} blocks {PACKED} forward: |y - fp64|max {err:.3e}, tolerance {TOL[dtype]}")
    assert err < TOL[dtype]


def test_all_clear_at_a_length_past_the_generic_kernels_lds():
    """10304 tokens: tf_attn_masked's four score rows do not fit the LDS and option 0 refuses; tf_attn_tiled_masked keeps no row there,
    runs, and is tf_attn_tiled in bits (81 query blocks of 161 trips)"""
    L, hd = 10304, 32
    enc = _encoder(hd, "f16", max_tokens=L, weights=False, attn_tiled=2)
    bits = np.full(L * (L // 32), 0xffffffff, dtype=np.uint32)
    mh = C.c_void_p()
    assert enc.lib.flope_tf_mask_create(enc.handle, L, bits.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(mh)) == 0
    qb, st = C.c_int(), [C.c_longlong() for _ in range(4)]
    assert enc.lib.flope_tf_mask_tiles(mh, C.byref(qb), *[C.byref(v) for v in st]) == 0
    assert (qb.value, [v.value for v in st]) == (81, [81 * 161, 161 * 4, 0, 80 * 161 * 8 + 161 * 4])      # the last query block has two waves
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(1, L, 3 * H * hd, generator=g).to(torch.float16).cuda()
    out = torch.full((1, L, H * hd), SENTINEL, dtype=torch.float16, device="cuda")
    rc = enc.lib.flope_tf_attention_masked(enc.handle, qkv.data_ptr(), 1, L, None, mh, out.data_ptr(), None)
    assert rc == EINVAL and b"too long for the score rows" in enc.lib.flope_tf_last_error(enc.handle) and bool((out == SENTINEL).all())
    assert enc.set_option("mask_mfma", 1) == 0
    rc = enc.lib.flope_tf_attention_masked(enc.handle, qkv.data_ptr(), 1, L, None, mh, out.data_ptr(), None)
    assert rc == MASKED16
    want = enc.attention(qkv)
    assert enc.last_attn_kernel == TILED and torch.equal(_bits(out), _bits(want))
    assert enc.lib.flope_tf_mask_destroy(mh) == 0


# ---- 2. keys no query allows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", M16.HEAD_DIMS)
def test_keys_no_query_allows_may_hold_nan(hd, dtype):
    L = 129
    d = H * hd
    enc = _encoder(hd, dtype, weights=False, mask_mfma=1)
    dead = [0, 31, 32, 63, 64, 100]                                          # step and block boundaries, and one inside a block beside allowed keys
    allowed = MB.make_allowed("random", L).clone()
    allowed[:, dead] = False
    allowed[:, 1] = True                                                     # every row keeps a key
    m = enc.make_mask(~allowed)
    qkv = MB.make_qkv(2, L, H, hd, dtype)
    clean = enc.attention(qkv.cuda(), mask=m).clone()
    assert enc.last_attn_kernel == MASKED16
    r, at = M16.ratio(clean, *M16.reference_of(qkv, allowed, H, dtype))
    assert r < 1.0, (r, at)
    for value in (float("nan"), float("inf")):
        got = enc.attention(M16.poison(qkv, dead, value).cuda(), mask=m)
        assert torch.isfinite(got.float()).all() and torch.equal(_bits(got), _bits(clean)), value


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding_rows_of_a_ragged_batch_may_hold_nan(dtype):
    hd, L, lens = 64, 129, [129, 1, 70, 33]
    enc = _encoder(hd, dtype, mask_mfma=1)
    allowed = MB.make_allowed("prefix", L)
    m = enc.make_mask(~allowed)
    x = _x(len(lens), L).cuda()
    clean = enc(x, lengths=lens, mask=m).clone()
    assert enc.last_attn_kernel == MASKED16
    for value in (float("nan"), float("inf")):
        xn = x.clone()
        for b, n in enumerate(lens):
            xn[b, n:] = value
        got = enc(xn, lengths=lens, mask=m)
        assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(clean))
    # the packed attention rows with a sentinel behind the output: a sequence's keys and rows end at its own length
    T, d = sum(lens), H * hd
    qkv = MB.make_qkv(1, T, H, hd, dtype).cuda()[0].contiguous()
    buf = torch.full((T + 64, d), SENTINEL, dtype=TDT[dtype], device="cuda")
    out = enc.attention(qkv, lengths=lens, mask=m, out=buf[:T])
    assert enc.last_attn_kernel == MASKED16 and bool((buf[T:] == SENTINEL).all()) and torch.isfinite(out.float()).all()
    o = 0
    for n in lens:
        alone = enc.attention(qkv[o:o + n].contiguous(), lengths=[n], mask=m)
        assert torch.equal(_bits(out[o:o + n]), _bits(alone)), n
        o += n


# ---- 3. random, prefix-LM, +-3 band, edge, gap and dead-key masks against fp64 ------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", M16.HEAD_DIMS)
def test_attention_within_the_derived_bound(hd, dtype):
    enc = _encoder(hd, dtype, weights=False, mask_mfma=1)
    cases = [(f"{kind}{L}", MB.make_allowed(kind, L), L) for kind in M16.KINDS for L in M16.LENGTHS]
    cases += [("gap257", M16.gap_mask(), 257), ("dead129", M16.dead_mask(129), 129)]
    worst = (0.0, "")
    for name, allowed, L in cases:
        m = enc.make_mask(~allowed)
        assert m.tile_stats == M16.tile_stats(allowed.numpy()), name
        qkv = MB.make_qkv(2, L, H, hd, dtype)
        got = enc.attention(qkv.cuda(), mask=m)
        assert enc.last_attn_kernel == MASKED16
        r, at = M16.ratio(got, *M16.reference_of(qkv, allowed, H, dtype))
        print(f"{dtype} head_dim {hd} {name}: {r:.3f} of the bound at {at}")
        assert r < 1.0, (name, r, at)
        worst = max(worst, (r, name))
        m.close()
    print(f"{dtype} head_dim {hd}: worst {worst[0]:.3f} of the bound at {worst[1]} (headroom {1 / max(worst[0], 1e-9):.1f}x)")


def test_the_gap_mask_skips_a_block_and_starts_waves_on_nothing():
    """what the gap mask is there for, said of the mask itself"""
    tm = M16.tile_map(M16.gap_mask().numpy())
    assert [e[0] for e in tm[0]] == [0, 2, 4] and [e[0] for e in tm[1]] == [1, 3] and [e[0] for e in tm[2]] == [0, 4]
    a = M16.gap_mask()
    assert tm[0][0][2][0][0] == M16.SOME and not a[16:32, :32].any() and a[0:16, :32].any()      # wave 0 takes step 0; rows 16 .. 31 see nothing in it


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", M16.HEAD_DIMS)
def test_forward_against_the_restatement(hd, dtype):
    enc = _encoder(hd, dtype, mask_mfma=1)
    L = 129 if hd == 64 else 65
    x = _x(2, L, seed=2)
    for kind in M16.KINDS if hd == 64 else ("random", "edge"):
        allowed = MB.make_allowed(kind, L)
        m = enc.make_mask(~allowed)
        y = enc(x.cuda(), mask=m)
        assert enc.last_attn_kernel == MASKED16 and enc.forward_plan(2, L, mask=m) == "launches"
        err = float(np.abs(y.cpu().numpy() - MB.masked_forward(_sd(hd), x.numpy(), allowed.numpy(), num_heads=H)).max())
        print(f"{dtype} head_dim {hd} {kind} L={L}: |y - fp64|max {err:.3e}, tolerance {TOL[dtype]}")
        assert torch.isfinite(y).all() and err < TOL[dtype], (kind, err)


# ---- 4. ragged ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,kind", [(32, "random"), (64, "band"), (96, "prefix"), (128, "random")])
def test_each_sequence_is_itself_alone_under_the_same_mask(hd, kind, dtype):
    L, lens = 257, [257, 130, 66, 1, 129]
    enc = _encoder(hd, dtype, mask_mfma=1)
    allowed = MB.make_allowed(kind, L)
    m = enc.make_mask(~allowed)
    x = _x(len(lens), L).cuda()
    y = enc(x, lengths=lens, mask=m).clone()
    assert enc.last_attn_kernel == MASKED16
    T = sum(lens)
    qkv = MB.make_qkv(1, T, H, hd, dtype).cuda()[0].contiguous()
    att = enc.attention(qkv, lengths=lens, mask=m).clone()
    o = 0
    for b, n in enumerate(lens):
        xb = torch.full((1, L, 7), float("nan"), device="cuda")
        xb[0, :n] = x[b, :n]
        alone = enc(xb, lengths=[n], mask=m)
        assert torch.equal(_bits(y[b, :n]), _bits(alone[0, :n])), (b, "forward")
        assert torch.equal(_bits(att[o:o + n]), _bits(enc.attention(qkv[o:o + n].contiguous(), lengths=[n], mask=m))), (b, "attention")
        o += n
    ref = MB.masked_forward(_sd(hd), x.cpu().numpy(), allowed.numpy(), lens, num_heads=H)
    assert float(np.abs(y.cpu().numpy() - ref).max()) < TOL[dtype]
    qp = torch.zeros(len(lens), L, 3 * H * hd, dtype=TDT[dtype])                # the packed rows as a padded batch, for the checker
    ap = torch.zeros(len(lens), L, H * hd, dtype=TDT[dtype])
    o = 0
    for b, n in enumerate(lens):
        qp[b, :n], ap[b, :n] = qkv[o:o + n].cpu(), att[o:o + n].cpu()
        o += n
    r, at = M16.ratio(ap, *M16.reference_of(qp, allowed, H, dtype, lens), lens)
    print(f"{dtype} head_dim {hd} {kind} ragged: {r:.3f} of the bound at {at}")
    assert r < 1.0, (r, at)


# ---- 5. state and ids -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_option_0_keeps_tf_attn_masked_and_its_bits(dtype):
    hd, L = 64, 129
    allowed = MB.make_allowed("random", L)
    qkv = MB.make_qkv(2, L, H, hd, dtype)
    x = _x(2, L).cuda()
    plain = _encoder(hd, dtype)                                              # a handle that never heard of the option
    mp = plain.make_mask(~allowed)
    a0, y0 = plain.attention(qkv.cuda(), mask=mp).clone(), plain(x, mask=mp).clone()
    assert plain.last_attn_kernel == MASKED
    r, at = MB.ratio(a0, *MB.reference_of(qkv, allowed, H, dtype))
    assert r < 1.0, "tf_attn_masked's own bound"
    enc = _encoder(hd, dtype, mask_mfma=0)
    m = enc.make_mask(~allowed)
    prev = 0
    for opt, kernel in ((0, MASKED), (1, MASKED16), (0, MASKED), (1, MASKED16)):      # flipped between calls
        assert enc.set_option("mask_mfma", opt) == prev
        prev = opt
        a, y = enc.attention(qkv.cuda(), mask=m), enc(x, mask=m)
        assert enc.last_attn_kernel == kernel
        if opt == 0:
            assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(y), _bits(y0))
        else:
            assert float((a.float() - a0.float()).abs().max()) > 0, "another summation order"


def test_fallbacks_keep_tf_attn_masked():
    L = 65
    allowed = MB.make_allowed("random", L)
    for hd, dtype, kw in ((64, "f16", dict(generic=1)), (64, "f32", dict()), (6, "f16", dict()), (6, "bf16", dict())):
        from flope_amd.tf_encoder import TransformerEncoder
        enc = TransformerEncoder(5, H * hd, 3, H, 1, 20, dtype=dtype, max_tokens=2 * L, mask_mfma=1)
        if kw:
            enc.set_option("generic", 1)
        plain = TransformerEncoder(5, H * hd, 3, H, 1, 20, dtype=dtype, max_tokens=2 * L)
        if kw:
            plain.set_option("generic", 1)
        qkv = MB.make_qkv(2, L, H, hd, dtype).cuda()
        got = enc.attention(qkv, mask=enc.make_mask(~allowed))
        assert enc.last_attn_kernel == MASKED, (hd, dtype)
        assert torch.equal(_bits(got), _bits(plain.attention(qkv, mask=plain.make_mask(~allowed))))
        assert enc.set_option("mask_mfma", 0) == 1, "stored, also where it is ignored"


def test_a_misaligned_buffer_falls_back():
    hd, L = 32, 33
    enc = _encoder(hd, "f16", weights=False, mask_mfma=1)
    m = enc.make_mask(~MB.make_allowed("random", L))
    qkv = MB.make_qkv(1, L, H, hd, "f16").cuda()
    want = enc.attention(qkv, mask=m).clone()
    assert enc.last_attn_kernel == MASKED16
    big = torch.zeros(qkv.numel() + 8, dtype=torch.float16, device="cuda")
    off = big[1:1 + qkv.numel()].view_as(qkv)                               # 2 bytes off a 16-byte boundary
    off.copy_(qkv)
    out = torch.empty_like(want)
    rc = enc.lib.flope_tf_attention_masked(enc.handle, off.data_ptr(), 1, L, None, m.handle, out.data_ptr(), None)
    assert rc == MASKED
    r, at = MB.ratio(out, *MB.reference_of(qkv.cpu(), MB.make_allowed("random", L), H, "f16"))
    assert r < 1.0 and not torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_other_calls_keep_their_bits_around_mask_mfma_calls(dtype):
    hd, L = 64, 129
    lens = [129, 1, 70]
    base = _encoder(hd, dtype, attn_tiled=1, window_mfma=0)
    x = _x(3, L).cuda()
    calls = [dict(), dict(is_causal=True), dict(is_causal=True, window=40), dict(lengths=lens)]
    ma_allowed, mb_allowed = MB.make_allowed("random", L), MB.make_allowed("prefix", L)

    def run_all(enc, ma, mb):
        out = []
        for wm in (0, 1):
            enc.set_option("window_mfma", wm)
            out += [enc(x, **kw).clone() for kw in calls]
        enc.set_option("mask_mfma", 0)
        out += [enc(x, mask=ma).clone(), enc(x, lengths=lens, mask=mb).clone()]
        return out

    before = run_all(base, base.make_mask(~ma_allowed), base.make_mask(~mb_allowed))
    enc = _encoder(hd, dtype, attn_tiled=1, mask_mfma=1)
    ma, mb = enc.make_mask(~ma_allowed), enc.make_mask(~mb_allowed)
    ya, yb = enc(x, mask=ma).clone(), enc(x, mask=mb).clone()
    assert enc.last_attn_kernel == MASKED16 and float((ya - yb).abs().max()) > 1e-3
    for m, ym in ((ma, ya), (mb, yb), (ma, ya), (mb, yb)):                   # two masks on one handle, alternately: each itself used alone
        assert torch.equal(_bits(enc(x, mask=m)), _bits(ym))
    for got, want in zip(run_all(enc, ma, mb), before):
        assert torch.equal(_bits(got), _bits(want))
    assert enc.set_option("mask_mfma", 1) == 0
    assert torch.equal(_bits(enc(x, mask=ma)), _bits(ya)) and enc.last_attn_kernel == MASKED16
    for got, want in zip(run_all(enc, ma, mb), before):
        assert torch.equal(_bits(got), _bits(want))
    mb.close()
    enc.set_option("mask_mfma", 1)
    assert torch.equal(_bits(enc(x, mask=ma)), _bits(ya)), "closing one mask leaves the other"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_option_values():
    from flope_amd.tf_encoder import TransformerEncoder
    enc = _encoder(32, "f16", weights=False)
    assert enc.set_option("mask_mfma", 1) == 0
    for bad in (2, -1):
        with pytest.raises(ValueError, match="mask_mfma is 0 or 1"):
            enc.set_option("mask_mfma", bad)
        assert enc.lib.flope_tf_set_option(enc.handle, b"mask_mfma", bad) == EINVAL
    assert enc.set_option("mask_mfma", 1) == 1, "a refused value changes nothing"
    for bad in (2, -1):
        with pytest.raises(ValueError, match="mask_mfma must be 0 or 1"):
            TransformerEncoder(*_dims(32), dtype="f16", mask_mfma=bad)
    f32 = TransformerEncoder(*_dims(32), dtype="f32", mask_mfma=1)             # stored and ignored
    assert f32.set_option("mask_mfma", 0) == 1


def test_the_masked_refusals_stay_under_option_1():
    hd, L = 32, 33
    enc, other = _encoder(hd, "f16", mask_mfma=1), _encoder(hd, "f16", mask_mfma=1)
    allowed = MB.make_allowed("edge", L)                                     # row 0 sees key L - 1 only
    m, mo = enc.make_mask(~allowed), other.make_mask(~allowed)
    x = _x(3, L).cuda()
    qkv = torch.zeros(3, L, 3 * H * hd, dtype=torch.float16, device="cuda")
    good = enc(x, mask=m).clone()
    for kw in (dict(is_causal=True), dict(window=3), dict(is_causal=True, window=3)):
        with pytest.raises(ValueError, match="say it in the mask"):
            enc(x, mask=m, **kw)
        with pytest.raises(ValueError, match="say it in the mask"):
            enc.attention(qkv, mask=m, **kw)
    with pytest.raises(ValueError, match="another encoder"):
        enc(x, mask=mo)
    with pytest.raises(ValueError, match="33 tokens, this call has 32"):
        enc(x[:, :32].contiguous(), mask=m)
    with pytest.raises(ValueError, match=r"b = 1, row 0 has no allowed key below 20"):
        enc(x, lengths=[33, 20, 33], mask=m)
    with pytest.raises(ValueError, match=r"b = 2, row 0"):
        enc.attention(torch.zeros(33 + 33 + 5, 3 * H * hd, dtype=torch.float16, device="cuda"), lengths=[33, 33, 5], mask=m)
    y = torch.full((3, L, 5), SENTINEL, device="cuda")
    rc = enc.lib.flope_tf_forward_masked(enc.handle, x.data_ptr(), 3, L, (C.c_int * 3)(33, 20, 33), m.handle, y.data_ptr(), None)
    assert rc == EINVAL and bool((y == SENTINEL).all()), "refused before anything is enqueued"
    assert enc.lib.flope_tf_attention_masked(enc.handle, qkv.data_ptr(), 3, L, None, None, y.data_ptr(), None) == EINVAL
    assert enc.lib.flope_tf_attention_masked(enc.handle, qkv.data_ptr(), 0, L, None, m.handle, y.data_ptr(), None) == EINVAL
    assert enc.lib.flope_tf_attention_masked(enc.handle, qkv.data_ptr(), 40, L, None, m.handle, y.data_ptr(), None) == EINVAL      # max_tokens
    assert enc.lib.flope_tf_mask_tiles(None, None, None, None, None, None) == EINVAL
    assert enc.lib.flope_tf_mask_tiles(m.handle, None, None, None, None, None) == 0
    assert torch.equal(_bits(enc(x, mask=m)), _bits(good)), "the next valid call"
    assert torch.equal(_bits(enc(x, lengths=[33, 33, 33], mask=m)), _bits(good)) and enc.last_attn_kernel == MASKED16
