"""A compiled additive bias on the 16-bit MFMA attention, on the device (option "bias_mfma", the BIASED instantiation of
tf_attn_tiled_masked).

The contract: with bias_mfma = 1 a 16-bit launch under a compiled bias at head_dim 32 / 64 / 96 / 128 walks tf_attn_tiled's ring and
step over the key blocks of the tile map of the bias's allowed set, the score of a seen key being fma(bias, log2e, fl(s scale log2e)).
A zero bias over A is enc.make_mask(A) under mask_mfma = 1 IN BITS (and so tf_attn_tiled's where DESIGN.md 38 gives them), equal planes
are the one plane, a sequence of a ragged batch is that sequence alone under the bias's corner, two biases used alternately are each
themselves; every other bias is held element-wise to fp64 within the bound of tests/tf_attn_bias16_bound.py and the whole forward to
tests/test_gpu_tf_bias.py's pins, 1.5e-2 (f16) / 1.2e-1 (bf16) of tests/tf_attn_bias_bound.biased_forward.  Option 0, generic = 1, float32
handles, head_dim 6 and misaligned buffers keep tf_attn_masked's BIASED instantiation (id 6) and its bits; no head_dim is refused for
scratch (tests/test_tf_bias16_host.py).

One model per head_dim, d = 2 head_dim, two heads, two layers (head_dim 128: one), as tests/test_gpu_tf_mask16.py.  Lengths 1 / 33 / 65 /
129 / 257: one key; one key into a second step; into a second block; a ring stage used twice; a second and a third query block.  257 and
33 take the dword form of the bias load everywhere, 1 / 65 / 129 too (no multiple of 4); the 16-byte form runs at L = 132 in the
tf_attn_tiled bit contract and the poison test (head_dim 64), at L = 260 in the ragged test (head_dim 64 and 96) and in the long
forward (head_dim 32); head_dim 128 has the dword form alone.

  1. the option and id 7   2. bit contracts   3. against fp64   4. poison   5. fallbacks   6. neighbours, values, refusals, a long forward
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tf_attn_bias16_bound as B16
import tf_attn_bias_bound as BB
import tf_attn_mask16_bound as M16
import tf_attn_mask_bound as MB

pytestmark = pytest.mark.gpu

TDT = MB.TDT
GENERIC, MFMA64, TILED, MASKED, MASKED16, BIASED, BIASED16 = 0, 1, 2, 4, 5, 6, 7
EINVAL = -1
SENTINEL = 1234.0
NINF = float("-inf")
TOL = {"f16": 1.5e-2, "bf16": 1.2e-1}          # tests/test_gpu_tf_bias.py's pins for the 16-bit modes
DTYPES = ["f16", "bf16"]
H = 2
RAGGED = list(B16.RAGGED)                      # 257 / 130 / 66 / 1 / 129 at L = 257


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


def _encoder(hd, dtype, max_tokens=5 * 260, weights=True, **kw):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*_dims(hd), dtype=dtype, max_tokens=max_tokens, **kw)
    if weights:
        enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in _sd(hd).items()})
    return enc


def _x(B, L, in_dim=7, seed=1):
    return torch.from_numpy(np.random.default_rng(seed * 1000 + L).standard_normal((B, L, in_dim)).astype(np.float32))


def _pad(packed, lens, L):
    """packed rows [sum(lens), w] -> [len(lens), L, w] on the CPU, zeros behind each length"""
    out = torch.zeros(len(lens), L, packed.shape[-1], dtype=packed.dtype)
    o = 0
    for b, n in enumerate(lens):
        out[b, :n] = packed[o:o + n].cpu()
        o += n
    return out


# ---- 1. the option and id 7 (what fails without the feature) ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_option_is_accepted_and_a_biased_call_reports_7(dtype):
    hd, L = 64, 65
    enc = _encoder(hd, dtype)
    assert enc.set_option("bias_mfma", 1) == 0
    b = enc.make_bias(BB.make_bias("alibi", L, H))
    enc.attention(MB.make_qkv(2, L, H, hd, dtype).cuda(), mask=b)
    assert enc.last_attn_kernel == BIASED16
    y = enc(_x(2, L).cuda(), mask=b)
    assert enc.last_attn_kernel == BIASED16 and torch.isfinite(y).all() and not enc.last_forward_fused
    assert enc.lib.flope_tf_last_forward_masked(enc.handle) == BIASED16
    assert enc.set_option("bias_mfma", 0) == 1
    made = _encoder(hd, dtype, bias_mfma=1)                                   # the constructor keyword
    assert made.set_option("bias_mfma", 1) == 1


# ---- 2. bit contracts -----------------------------------------------------------------------------------------------------------------
def _sets(L):
    """the allowed sets of contract (a): clear, causal, band 33, random 40 %, the edge rows, and DESIGN.md 38's gap mask at L = 257"""
    out = [("clear", MB.make_allowed("clear", L)), ("causal", MB.make_allowed("causal", L)), ("band33", MB.band_causal(L, 33)),
           ("random", MB.make_allowed("random", L)), ("edge", MB.make_allowed("edge", L))]
    if L == 257:
        out.append(("gap", M16.gap_mask()))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", B16.HEAD_DIMS)
def test_zero_bias_is_the_compiled_mask_under_mask_mfma(hd, dtype):
    """(a) at enc.attention and at the whole forward, one plane and H planes"""
    enc = _encoder(hd, dtype, mask_mfma=1, bias_mfma=1)
    n = 0
    for L in B16.LENGTHS:
        x = _x(2, L).cuda()
        qkv = MB.make_qkv(2, L, H, hd, dtype).cuda()
        for name, allowed in _sets(L):
            m = enc.make_mask(~allowed)
            zero = B16.zero_over(allowed, H if n % 2 else 1)
            b = enc.make_bias(zero[0] if n % 4 == 0 else zero)
            assert (b.planes, m.planes) == (H if n % 2 else 1, 0) and b.tile_stats == m.tile_stats == M16.tile_stats(allowed.numpy())
            want = enc.attention(qkv, mask=m).clone()
            assert enc.last_attn_kernel == MASKED16
            got = enc.attention(qkv, mask=b)
            assert enc.last_attn_kernel == BIASED16
            assert torch.isfinite(got.float()).all() and torch.equal(_bits(got), _bits(want)), (name, L, "attention")
            want = enc(x, mask=m).clone()
            got = enc(x, mask=b)
            assert enc.last_attn_kernel == BIASED16
            assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), (name, L, "forward")
            m.close()
            b.close()
            n += 1
    assert n == 26


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_bias_is_tf_attn_tiled_where_the_mask_is(dtype):
    """... and therefore, by DESIGN.md 38, the plain / causal / windowed tf_attn_tiled bits"""
    hd = 64
    enc = _encoder(hd, dtype, attn_tiled=2, window_mfma=1, bias_mfma=1)
    for L in (65, 132, 257):                                                  # 132: the 16-byte form of the bias load, held to bits
        x, qkv = _x(2, L).cuda(), MB.make_qkv(2, L, H, hd, dtype).cuda()
        for allowed, kw in ((MB.make_allowed("clear", L), dict()), (MB.make_allowed("causal", L), dict(is_causal=True)),
                            (MB.band_causal(L, 33), dict(is_causal=True, window=33))):
            b = enc.make_bias(B16.zero_over(allowed, H))
            want = enc.attention(qkv, **kw).clone()
            assert enc.last_attn_kernel == TILED
            assert torch.equal(_bits(enc.attention(qkv, mask=b)), _bits(want)) and enc.last_attn_kernel == BIASED16, (L, kw)
            want = enc(x, **kw).clone()
            assert torch.equal(_bits(enc(x, mask=b)), _bits(want)), (L, kw)
            b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", B16.HEAD_DIMS)
def test_equal_planes_are_the_one_plane(hd, dtype):
    """(b)"""
    enc = _encoder(hd, dtype, bias_mfma=1)
    for L in B16.LENGTHS:
        for kind in ("holes", "edge"):
            one = BB.make_bias(kind, L, H, 1)
            b1, bh = enc.make_bias(one[0]), enc.make_bias(one.expand(H, L, L))
            assert (b1.planes, bh.planes) == (1, H)
            qkv = MB.make_qkv(2, L, H, hd, dtype).cuda()
            a1 = enc.attention(qkv, mask=b1).clone()
            assert enc.last_attn_kernel == BIASED16
            assert torch.equal(_bits(enc.attention(qkv, mask=bh)), _bits(a1)), (kind, L)
            x = _x(2, L).cuda()
            y1 = enc(x, mask=b1).clone()
            assert torch.equal(_bits(enc(x, mask=bh)), _bits(y1)), (kind, L)
            b1.close()
            bh.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,kind,L,lens", [(32, "holes", 257, RAGGED), (64, "alibi", 257, RAGGED), (96, "holes", 257, RAGGED),
                                            (128, "alibi", 257, RAGGED), (64, "holes", 260, [260, 130, 66, 1, 129]),
                                            (96, "alibi", 260, [260, 132, 1])], ids=str)
def test_each_sequence_is_itself_alone_under_the_corner(hd, kind, L, lens, dtype):
    """(c) each sequence of a ragged batch = itself encoded alone under make_bias(bias[..., :n, :n]); the packed attention rows within
    the bound.  L = 260: the 16-byte form of the bias load, row stride 260 under every corner"""
    enc = _encoder(hd, dtype, bias_mfma=1)
    bias = BB.make_bias(kind, L, H)
    m = enc.make_bias(bias)
    x = _x(len(lens), L).cuda()
    y = enc(x, lengths=lens, mask=m).clone()
    assert enc.last_attn_kernel == BIASED16
    T = sum(lens)
    qkv = MB.make_qkv(1, T, H, hd, dtype).cuda()[0].contiguous()
    att = enc.attention(qkv, lengths=lens, mask=m).clone()
    assert enc.last_attn_kernel == BIASED16
    o = 0
    for b, n in enumerate(lens):
        corner = enc.make_bias(bias[:, :n, :n])
        assert torch.equal(_bits(y[b, :n]), _bits(enc(x[b:b + 1, :n].contiguous(), mask=corner)[0])), (b, "forward")
        assert torch.equal(_bits(att[o:o + n]), _bits(enc.attention(qkv[o:o + n][None].contiguous(), mask=corner)[0])), (b, "attention")
        assert enc.last_attn_kernel == BIASED16
        corner.close()
        o += n
    ref = BB.biased_forward(_sd(hd), x.cpu().numpy(), bias.numpy(), lens, num_heads=H)
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print(f"{dtype} head_dim {hd} {kind} L={L} ragged forward: |y - fp64|max {err:.3e}, tolerance {TOL[dtype]}")
    assert err < TOL[dtype]
    qp, ap = _pad(qkv, lens, L), _pad(att, lens, L)
    r, at = B16.ratio(ap, *B16.reference_of(qp, bias, H, dtype, lens), lens)
    print(f"{dtype} head_dim {hd} {kind} L={L} ragged: {r:.3f} of the bound at {at}")
    assert r < 1.0, (r, at)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_biases_used_alternately_are_each_themselves(dtype):
    """(d)"""
    hd, L = 96, 129
    enc = _encoder(hd, dtype, bias_mfma=1)
    x, qkv = _x(2, L).cuda(), MB.make_qkv(2, L, H, hd, dtype).cuda()
    ba, bb = enc.make_bias(BB.make_bias("holes", L, H)), enc.make_bias(BB.make_bias("alibi", L, H, 1))
    ya, yb = enc(x, mask=ba).clone(), enc(x, mask=bb).clone()
    aa, ab = enc.attention(qkv, mask=ba).clone(), enc.attention(qkv, mask=bb).clone()
    assert float((ya - yb).abs().max()) > 1e-3
    for m, ym, am in ((ba, ya, aa), (bb, yb, ab), (ba, ya, aa), (bb, yb, ab)):
        assert torch.equal(_bits(enc(x, mask=m)), _bits(ym)) and torch.equal(_bits(enc.attention(qkv, mask=m)), _bits(am))
        assert enc.last_attn_kernel == BIASED16
    bb.close()
    assert torch.equal(_bits(enc(x, mask=ba)), _bits(ya)), "closing one bias leaves the other"


# ---- 3. against fp64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", B16.HEAD_DIMS)
def test_attention_within_the_derived_bound(hd, dtype):
    """every element of enc.attention: a random bias with holes, per-head ALiBi 2^-(h+1), the edge mask with a bias, the gap mask with a
    bias, one plane, ragged batches (tf_attn_bias16_bound.shapes)"""
    enc = _encoder(hd, dtype, weights=False, bias_mfma=1)
    worst = (0.0, "")
    for name, kind, L, planes, lengths in B16.shapes():
        bias = B16.make_bias(kind, L, H, planes)
        m = enc.make_bias(bias)
        B = 2 if lengths is None else len(lengths)
        qkv = MB.make_qkv(B, L, H, hd, dtype)
        if lengths is None:
            got = enc.attention(qkv.cuda(), mask=m)
        else:
            packed = torch.cat([qkv[b, :n] for b, n in enumerate(lengths)]).contiguous().cuda()
            got = _pad(enc.attention(packed, lengths=list(lengths), mask=m), lengths, L)
        assert enc.last_attn_kernel == BIASED16
        r, at = B16.ratio(got, *B16.reference_of(qkv, bias, H, dtype, lengths), lengths)
        print(f"{dtype} head_dim {hd} {name}: {r:.3f} of the bound at {at}")
        assert r < 1.0, (name, r, at)
        worst = max(worst, (r, name))
        m.close()
    print(f"{dtype} head_dim {hd}: worst {worst[0]:.3f} of the bound at {worst[1]} (headroom {1 / max(worst[0], 1e-9):.1f}x)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", B16.HEAD_DIMS)
def test_forward_against_the_restatement(hd, dtype):
    enc = _encoder(hd, dtype, bias_mfma=1)
    L = 129 if hd == 64 else 65
    x = _x(2, L, seed=2)
    for kind in BB.KINDS:
        bias = BB.make_bias(kind, L, H)
        m = enc.make_bias(bias)
        y = enc(x.cuda(), mask=m)
        assert enc.last_attn_kernel == BIASED16 and not enc.last_forward_fused and enc.forward_plan(2, L, mask=m) == "launches"
        err = float(np.abs(y.cpu().numpy() - BB.biased_forward(_sd(hd), x.numpy(), bias.numpy(), num_heads=H)).max())
        print(f"{dtype} head_dim {hd} {kind} L={L}: |y - fp64|max {err:.3e}, tolerance {TOL[dtype]}")
        assert torch.isfinite(y).all() and err < TOL[dtype], (kind, err)


# ---- 4. poison ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,L", [(32, 129), (64, 132), (96, 129), (128, 132)])
def test_keys_no_query_allows_may_hold_nan(hd, L, dtype):
    """NaN, then Inf, in k and v of keys no query allows; sentinels around out.  L = 132: the 16-byte form of the bias load"""
    d = H * hd
    enc = _encoder(hd, dtype, weights=False, bias_mfma=1)
    dead = [0, 31, 32, 63, 64, 100]
    g = torch.Generator().manual_seed(L)
    bias = BB.over(MB.make_allowed("random", 129)[:L, :L] if L <= 129 else torch.rand(L, L, generator=g) < 0.6, 2 * torch.randn(H, L, L, generator=g)).clone()
    bias[:, :, dead] = NINF
    bias[:, :, 1] = 0.25                                                     # every row keeps a key
    m = enc.make_bias(bias)
    qkv = MB.make_qkv(2, L, H, hd, dtype)
    obuf = torch.full((2 * L + 2, d), SENTINEL, dtype=TDT[dtype], device="cuda")
    out = obuf[1:-1].view(2, L, d)                                            # d 16-bit elements a row: 16-byte aligned behind one row
    clean = enc.attention(qkv.cuda(), mask=m, out=out).clone()
    assert enc.last_attn_kernel == BIASED16
    assert bool((obuf[0] == SENTINEL).all()) and bool((obuf[-1] == SENTINEL).all()), "sentinels around out"
    r, at = B16.ratio(clean, *B16.reference_of(qkv, bias, H, dtype))
    assert r < 1.0, (r, at)
    for value in (float("nan"), float("inf")):
        got = enc.attention(M16.poison(qkv, dead, value).cuda(), mask=m, out=out)
        assert enc.last_attn_kernel == BIASED16
        assert torch.isfinite(got.float()).all() and torch.equal(_bits(got), _bits(clean)), value
        assert bool((obuf[0] == SENTINEL).all()) and bool((obuf[-1] == SENTINEL).all()), "sentinels around out"


@pytest.mark.parametrize("dtype", DTYPES)
def test_padding_rows_of_a_ragged_batch_may_hold_nan(dtype):
    hd, L, lens = 64, 129, [129, 1, 70, 33]
    enc = _encoder(hd, dtype, bias_mfma=1)
    m = enc.make_bias(BB.make_bias("alibi", L, H))
    x = _x(len(lens), L).cuda()
    clean = enc(x, lengths=lens, mask=m).clone()
    assert enc.last_attn_kernel == BIASED16
    for value in (float("nan"), float("inf")):
        xn = x.clone()
        for b, n in enumerate(lens):
            xn[b, n:] = value
        got = enc(xn, lengths=lens, mask=m)
        assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(clean)), value
    T, d = sum(lens), H * hd
    qkv = MB.make_qkv(1, T, H, hd, dtype).cuda()[0].contiguous()
    buf = torch.full((T + 64, d), SENTINEL, dtype=TDT[dtype], device="cuda")
    out = enc.attention(qkv, lengths=lens, mask=m, out=buf[:T])
    assert enc.last_attn_kernel == BIASED16 and bool((buf[T:] == SENTINEL).all()) and torch.isfinite(out.float()).all()


# ---- 5. fallbacks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_option_0_keeps_id_6_and_its_bits(dtype):
    hd, L = 64, 129
    bias = BB.make_bias("holes", L, H)
    qkv = MB.make_qkv(2, L, H, hd, dtype)
    x = _x(2, L).cuda()
    plain = _encoder(hd, dtype)                                              # a handle that never heard of the option
    bp = plain.make_bias(bias)
    a0, y0 = plain.attention(qkv.cuda(), mask=bp).clone(), plain(x, mask=bp).clone()
    assert plain.last_attn_kernel == BIASED
    enc = _encoder(hd, dtype, bias_mfma=0, mask_mfma=1)
    b = enc.make_bias(bias)
    plain_mask = enc.make_mask(~BB.allowed_of(bias))
    prev = 0
    for opt, kernel in ((0, BIASED), (1, BIASED16), (0, BIASED), (1, BIASED16)):      # flipped between calls
        assert enc.set_option("bias_mfma", opt) == prev
        prev = opt
        a, y = enc.attention(qkv.cuda(), mask=b), enc(x, mask=b)
        assert enc.last_attn_kernel == kernel
        if opt == 0:
            assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(y), _bits(y0))
        else:
            assert float((a.float() - a0.float()).abs().max()) > 0, "another summation order"
        for mm, want in ((1, MASKED16), (0, MASKED), (1, MASKED16)):               # a plain mask runs 4 / 5 by mask_mfma alone
            enc.set_option("mask_mfma", mm)
            enc.attention(qkv.cuda(), mask=plain_mask)
            assert enc.last_attn_kernel == want, (opt, mm)


def test_fallbacks_keep_id_6_and_its_bits():
    """generic = 1, a float32 handle, head_dim 6 (no head_dim tf_attn_tiled serves is refused for scratch: tests/test_tf_bias16_host.py)"""
    from flope_amd.tf_encoder import TransformerEncoder
    L = 65
    for hd, dtype, generic in ((64, "f16", 1), (64, "f32", 0), (6, "f16", 0), (6, "bf16", 0)):
        bias = BB.make_bias("holes", L, H)
        enc = TransformerEncoder(5, H * hd, 3, H, 1, 20, dtype=dtype, max_tokens=2 * L, bias_mfma=1)
        plain = TransformerEncoder(5, H * hd, 3, H, 1, 20, dtype=dtype, max_tokens=2 * L)
        if generic:
            enc.set_option("generic", 1)
            plain.set_option("generic", 1)
        qkv = MB.make_qkv(2, L, H, hd, dtype).cuda()
        got = enc.attention(qkv, mask=enc.make_bias(bias))
        assert enc.last_attn_kernel == BIASED, (hd, dtype)
        assert torch.equal(_bits(got), _bits(plain.attention(qkv, mask=plain.make_bias(bias))))
        assert enc.set_option("bias_mfma", 0) == 1, "stored, also where it is ignored"


def test_a_misaligned_buffer_falls_back():
    hd, L = 32, 33
    enc = _encoder(hd, "f16", weights=False, bias_mfma=1)
    plain = _encoder(hd, "f16", weights=False)
    bias = BB.make_bias("holes", L, H)
    m = enc.make_bias(bias)
    qkv = MB.make_qkv(1, L, H, hd, "f16").cuda()
    want16 = enc.attention(qkv, mask=m).clone()
    assert enc.last_attn_kernel == BIASED16
    want6 = plain.attention(qkv, mask=plain.make_bias(bias)).clone()
    big = torch.zeros(qkv.numel() + 8, dtype=torch.float16, device="cuda")
    off = big[1:1 + qkv.numel()].view_as(qkv)                               # 2 bytes off a 16-byte boundary
    off.copy_(qkv)
    out = torch.empty_like(want16)
    rc = enc.lib.flope_tf_attention_masked(enc.handle, off.data_ptr(), 1, L, None, m.handle, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == BIASED
    assert torch.equal(_bits(out), _bits(want6)) and not torch.equal(_bits(out), _bits(want16))


# ---- 6. neighbours, values, refusals, a long forward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_other_calls_keep_their_bits_around_bias_mfma_calls(dtype):
    from flope_amd.tf_encoder import alibi_distances
    hd, L = 64, 129
    lens = [129, 1, 70]
    x = _x(3, L).cuda()
    allowed = MB.make_allowed("random", L)
    bias = BB.make_bias("holes", L, H)
    table = alibi_distances(L, [0.5, 0.25])
    calls = [dict(), dict(is_causal=True), dict(is_causal=True, window=40), dict(lengths=lens)]

    def run_all(enc, mk, b):
        out = [enc(x, **kw).clone() for kw in calls]
        for mm in (0, 1):
            enc.set_option("mask_mfma", mm)
            out.append(enc(x, mask=mk).clone())
        enc.set_option("mask_mfma", 0)
        old = enc.set_option("bias_mfma", 0)                                  # option-0 biased, fixed and ragged
        out += [enc(x, mask=b).clone(), enc(x, lengths=lens, mask=b).clone()]
        enc.set_option("bias_mfma", old)
        s = enc.open_stream(3, L, bias=table)                                 # a biased stream: the option does not reach it
        out.append(s.prefill(x, lengths=lens).clone())
        out.append(s.step(x[:2, 0].contiguous(), tracks=[1, 2]).clone())
        s.close()
        return out

    base = _encoder(hd, dtype, attn_tiled=1)
    before = run_all(base, base.make_mask(~allowed), base.make_bias(bias))
    enc = _encoder(hd, dtype, attn_tiled=1)
    mk, b = enc.make_mask(~allowed), enc.make_bias(bias)
    for got, want in zip(run_all(enc, mk, b), before):
        assert torch.equal(_bits(got), _bits(want))
    assert enc.set_option("bias_mfma", 1) == 0
    y16 = enc(x, mask=b).clone()
    assert enc.last_attn_kernel == BIASED16
    for got, want in zip(run_all(enc, mk, b), before):
        assert torch.equal(_bits(got), _bits(want))
    assert enc.set_option("bias_mfma", 1) == 1, "run_all put the option back"
    assert torch.equal(_bits(enc(x, mask=b)), _bits(y16)) and enc.last_attn_kernel == BIASED16
    assert enc.set_option("bias_mfma", 0) == 1
    for got, want in zip(run_all(enc, mk, b), before):
        assert torch.equal(_bits(got), _bits(want))


def test_a_fused_float32_handle_keeps_its_bits():
    """fused = 1 forwards (the single launch) around bias_mfma calls on a float32 handle, which stores the option and ignores it"""
    from flope_amd.tf_encoder import TransformerEncoder
    from oracle import tf_encoder_ref as T
    dims = (9, 32, 4, 4, 2, 64)
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=3)
    enc = TransformerEncoder(*dims, dtype="f32", max_tokens=6 * 15, fused=1)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    x = _x(6, 15, 9).cuda()
    b = enc.make_bias(BB.make_bias("holes", 15, 4))
    y0, yb0 = enc(x).clone(), enc(x, mask=b).clone()
    assert enc.last_attn_kernel == BIASED
    assert enc.set_option("bias_mfma", 1) == 0
    yb1 = enc(x, mask=b).clone()
    assert enc.last_attn_kernel == BIASED and torch.equal(_bits(yb1), _bits(yb0))
    y1 = enc(x)
    assert enc.last_forward_fused and torch.equal(_bits(y1), _bits(y0))
    assert enc.set_option("bias_mfma", 0) == 1


def test_option_values():
    from flope_amd.tf_encoder import TransformerEncoder
    enc = _encoder(32, "f16", weights=False)
    assert enc.set_option("bias_mfma", 1) == 0
    for bad in (2, -1):
        with pytest.raises(ValueError, match="bias_mfma is 0 or 1"):
            enc.set_option("bias_mfma", bad)
        assert enc.lib.flope_tf_set_option(enc.handle, b"bias_mfma", bad) == EINVAL
    assert enc.set_option("bias_mfma", 1) == 1, "a refused value changes nothing"
    assert enc.set_option("mask_mfma", 0) == 0, "an option of its own: mask_mfma was never touched"
    for bad in (2, -1):
        with pytest.raises(ValueError, match="bias_mfma must be 0 or 1"):
            TransformerEncoder(*_dims(32), dtype="f16", bias_mfma=bad)
    f32 = TransformerEncoder(*_dims(32), dtype="f32", bias_mfma=1)             # stored and ignored
    assert f32.set_option("bias_mfma", 0) == 1


def test_the_bias_refusals_keep_their_text_under_option_1():
    hd, L = 32, 33
    enc, other = _encoder(hd, "f16", bias_mfma=1), _encoder(hd, "f16", bias_mfma=1)
    bias = BB.make_bias("edge", L, H)                                        # row 0 sees key L - 1 only
    m, mo = enc.make_bias(bias), other.make_bias(bias)
    x = _x(3, L).cuda()
    qkv = torch.zeros(3, L, 3 * H * hd, dtype=torch.float16, device="cuda")
    good = enc(x, mask=m).clone()
    assert enc.last_attn_kernel == BIASED16
    for kw in (dict(is_causal=True), dict(window=3), dict(is_causal=True, window=3)):
        with pytest.raises(ValueError, match="say it in the mask"):
            enc(x, mask=m, **kw)
        with pytest.raises(ValueError, match="say it in the mask"):
            enc.attention(qkv, mask=m, **kw)
    with pytest.raises(ValueError, match="another encoder"):
        enc(x, mask=mo)
    with pytest.raises(ValueError, match="33 tokens, this call has 32"):
        enc(x[:, :32].contiguous(), mask=m)
    with pytest.raises(ValueError, match="differs from the mask's"):
        enc.attention(qkv[:, :32].contiguous(), mask=m)
    with pytest.raises(ValueError, match=r"b = 1, row 0 has no allowed key below 20"):
        enc(x, lengths=[33, 20, 33], mask=m)
    b = bias.clone()
    b[1, 7, 3] = float("inf")
    with pytest.raises(ValueError, match=r"\(plane 1, row 7, col 3\) is \+inf or NaN"):
        enc.make_bias(b)
    b = bias.clone()
    b[1, 5, 5] = NINF
    with pytest.raises(ValueError, match=r"\(plane 1, row 5, col 5\).*large negative finite value"):
        enc.make_bias(b)
    y = torch.full((3, L, 5), SENTINEL, device="cuda")
    rc = enc.lib.flope_tf_forward_masked(enc.handle, x.data_ptr(), 3, L, (C.c_int * 3)(33, 20, 33), m.handle, y.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == EINVAL and bool((y == SENTINEL).all()), "refused before anything is enqueued"
    assert torch.equal(_bits(enc(x, mask=m)), _bits(good)), "the next valid call"


def test_a_forward_at_a_length_past_the_generic_kernels_lds():
    """10304 tokens: tf_attn_masked's four score rows do not fit the LDS and option 0 refuses; under option 1 the forward runs, and a
    handful of sampled rows of its attention are held to the fp64 bound computed for those rows alone"""
    L, hd = 10304, 32
    enc = _encoder(hd, "f16", max_tokens=L, bias_mfma=0)
    bias = BB.alibi(L, [0.5])                                                # one plane, causal: 412 MiB
    m = enc.make_bias(bias)
    x = _x(1, L).cuda()
    with pytest.raises(ValueError, match="too long for the score rows"):
        enc(x, mask=m)
    assert enc.set_option("bias_mfma", 1) == 0
    y = enc(x, mask=m)
    assert enc.last_attn_kernel == BIASED16 and torch.isfinite(y).all()
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(1, L, 3 * H * hd, generator=g).to(torch.float16)
    got = enc.attention(qkv.cuda(), mask=m).cpu()
    assert enc.last_attn_kernel == BIASED16
    d = H * hd
    qd = qkv[0].double()
    for i in (0, 31, 127, 128, 4097, 10239, 10303):
        n = i + 1                                                            # causal: row i of the whole = the last row of the first n tokens
        worst = 0.0
        for h in range(H):
            q, k, v = qd[i, h * hd:(h + 1) * hd], qd[:n, d + h * hd:d + (h + 1) * hd], qd[:n, 2 * d + h * hd:2 * d + (h + 1) * hd]
            bb = bias[0, i, :n].double()
            p = torch.softmax(k @ q / np.sqrt(hd) + bb, dim=0)
            o, A = p @ v, p @ v.abs()
            aj = (B16.AB.LOG2E / np.sqrt(hd)) * (k.abs() @ q.abs())
            bj = B16.AB.LOG2E * bb.abs()
            a, bl, ab = aj.max(), bj.max(), (aj + bj).max()
            ns, u, uT = (L + 31) // 32, B16.AB.U32, B16.AB.U_T["f16"]           # the operation counts of the whole sequence, as in reference_of
            e = np.log(2.0) * ((hd + 4) * a + 5 * ab + bl) * u + (4 * ns + 8) * u
            E = 2 * e + 2 * (L + ns + 10) * u
            bound = (uT + E) * A
            bound = bound + uT * (o.abs() + bound) + (L * 2.0 ** -25 * qd[:, 2 * d + h * hd:2 * d + (h + 1) * hd].abs().max() + 2.0 ** -25)
            worst = max(worst, float(((got[0, i, h * hd:(h + 1) * hd].double() - o).abs() / bound).max()))
        print(f"L = {L} row {i}: {worst:.3f} of the bound")
        assert worst < 1.0, (i, worst)
