"""An additive attention bias, per head, compiled once, on the device (enc.make_bias, forward / attention(..., mask=<compiled bias>);
DESIGN.md 39).

The contract: a compiled bias runs the BIASED instantiation of tf_attn_masked on every dtype and under every option -- the unbiased order with one float32 add
of the pair's bias after the scale -- so a zero bias over an allowed set is enc.make_mask of that set IN BITS (and so, by DESIGN.md 37,
the causal / window / ragged kernels' bits where those hold), equal planes are the one plane, a masked key is never loaded (not its k,
not its v, not its bias entry); every other bias is held element-wise to fp64 within the bound of tests/tf_attn_bias_bound.py, and the
whole forward to the project's tolerances: 2e-4 (f32, f32m), 1.5e-2 (f16), 1.2e-1 (bf16), the reference module's fixture to 1e-5.
Shapes as tests/test_gpu_tf_mask.py: L 1 / 15 / 33 / 65 / 130, head_dim 6 and 64, the edge mask among the allowed sets.

  ODD   (5, 30, 3, 5, 1, 20)      head_dim 6, one layer, five heads
  TOY   (16, 32, 9, 4, 2, 64)     the reference fixture's dims
  WIDE  (16, 128, 9, 2, 2, 256)   head_dim 64: a 16-bit forward whose unmasked attention is an MFMA kernel

  1. bit contracts   2. masked keys are never loaded   3. against fp64   4. ragged   5. state   6. refusals
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tf_attn_bias_bound as BB
import tf_attn_mask_bound as MB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = MB.TDT
GENERIC, MASKED, MASKED16, BIASED = 0, 4, 5, 6
EINVAL, ESTATE = -1, -3
SENTINEL = 1234.0
NINF = float("-inf")
ODD = (5, 30, 3, 5, 1, 20)
TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)
DIMS = {"odd": ODD, "toy": TOY, "wide": WIDE}
MODES = [("f32", 2e-4), ("f32m", 2e-4), ("f16", 1.5e-2), ("bf16", 1.2e-1)]
SETS = ("clear", "causal", "band", "random", "edge")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _encoder(dims, sd, dtype, max_tokens, **kw):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, **kw)
    if sd is not None:
        enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return enc


@pytest.fixture(scope="module")
def sds():
    """name -> state dict; computed once, never changed"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_bias_fixture.npz"))
    return {"toy": {k[4:]: f[k] for k in f.files if k.startswith("sd::")},
            "odd": T.synthetic_state_dict(ODD[0], ODD[1], ODD[2], ODD[4], ODD[5], seed=3),
            "wide": T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)}


def _x(B, L, in_dim, seed=1):
    return torch.from_numpy(np.random.default_rng(seed * 1000 + L).standard_normal((B, L, in_dim)).astype(np.float32))


def _zero_over(allowed, planes=1):
    return BB.over(allowed, torch.zeros(planes, *allowed.shape))


# ---- 1. bit contracts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", ["odd", "wide"])
def test_zero_bias_is_the_compiled_mask(sds, shape, dtype):
    """a zero bias over A = enc.make_mask(A), one plane and H planes, at enc.attention and at the whole forward"""
    dims = DIMS[shape]
    H, d = dims[3], dims[1]
    enc = _encoder(dims, sds[shape], dtype, 2 * 130)
    n = 0
    for L in MB.LENGTHS:
        x = _x(2, L, dims[0]).cuda()
        qkv = MB.make_qkv(2, L, H, d // H, dtype).cuda()
        for kind in SETS:
            allowed = MB.make_allowed(kind, L)
            m = enc.make_mask(~allowed)
            zero = _zero_over(allowed, H if n % 2 else 1)
            b = enc.make_bias((zero[0] if n % 4 == 0 else zero).to("cuda" if n % 3 == 0 else "cpu"))
            assert (b.L, b.allowed, b.planes, m.planes) == (L, int(allowed.sum()), H if n % 2 else 1, 0)
            assert b.tile_stats == m.tile_stats and enc.flops(2, L, mask=b) == enc.flops(2, L, mask=m)
            want = enc.attention(qkv, mask=m).clone()
            assert enc.last_attn_kernel == MASKED
            got = enc.attention(qkv, mask=b)
            assert enc.last_attn_kernel == BIASED
            assert torch.equal(_bits(got), _bits(want)), (kind, L, "attention")
            want = enc(x, mask=m).clone()
            got = enc(x, mask=b)
            assert enc.last_attn_kernel == BIASED and not enc.last_forward_fused
            assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), (kind, L, "forward")
            m.close()
            b.close()
            n += 1
    assert n == 25


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_zero_causal_bias_is_the_causal_kernel_and_a_band_the_window(sds, dtype):
    """... and therefore the dedicated kernels' bits where DESIGN.md 37 gives them to the mask"""
    enc = _encoder(ODD, sds["odd"], dtype, 2 * 65)
    for L in (15, 65):
        x = _x(2, L, ODD[0]).cuda()
        for allowed, kw in ((MB.make_allowed("causal", L), dict(is_causal=True)), (MB.band_causal(L, 4), dict(is_causal=True, window=4)),
                            (MB.make_allowed("clear", L), dict())):
            want = enc(x, **kw).clone()
            assert torch.equal(_bits(enc(x, mask=enc.make_bias(_zero_over(allowed, ODD[3])))), _bits(want)), (L, kw)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", ["odd", "wide"])
def test_equal_planes_are_the_one_plane(sds, shape, dtype):
    dims = DIMS[shape]
    H, d = dims[3], dims[1]
    enc = _encoder(dims, sds[shape], dtype, 2 * 130)
    for L in MB.LENGTHS:
        for kind in ("holes", "edge"):
            one = BB.make_bias(kind, L, H, 1)
            b1, bh = enc.make_bias(one[0]), enc.make_bias(one.expand(H, L, L))
            assert (b1.planes, bh.planes) == (1, H)
            qkv = MB.make_qkv(2, L, H, d // H, dtype).cuda()
            assert torch.equal(_bits(enc.attention(qkv, mask=bh)), _bits(enc.attention(qkv, mask=b1))), (kind, L)
            x = _x(2, L, dims[0]).cuda()
            assert torch.equal(_bits(enc(x, mask=bh)), _bits(enc(x, mask=b1))), (kind, L)
            b1.close()
            bh.close()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_mask_mfma_handle_returns_the_same_bits(sds, dtype):
    """a bias keeps the BIASED tf_attn_masked on a handle whose masks run the MFMA kernel, and under `generic`"""
    L = 65
    plain, mfma = _encoder(WIDE, sds["wide"], dtype, 2 * L), _encoder(WIDE, sds["wide"], dtype, 2 * L, mask_mfma=1)
    qkv = MB.make_qkv(2, L, 2, 64, dtype).cuda()
    x = _x(2, L, WIDE[0]).cuda()
    mfma.attention(qkv, mask=mfma.make_mask(~MB.make_allowed("random", L)))
    assert mfma.last_attn_kernel == MASKED16, "a plain mask does take the MFMA kernel on this handle"
    for kind in BB.KINDS:
        bias = BB.make_bias(kind, L, 2)
        bp, bm = plain.make_bias(bias), mfma.make_bias(bias)
        want = plain.attention(qkv, mask=bp).clone()
        got = mfma.attention(qkv, mask=bm)
        assert mfma.last_attn_kernel == BIASED and torch.equal(_bits(got), _bits(want)), kind
        wy = plain(x, mask=bp).clone()
        gy = mfma(x, mask=bm)
        assert mfma.last_attn_kernel == BIASED and torch.equal(_bits(gy), _bits(wy)), kind
        plain.set_option("generic", 1)
        assert torch.equal(_bits(plain.attention(qkv, mask=bp)), _bits(want)) and plain.last_attn_kernel == BIASED
        plain.set_option("generic", 0)


# ---- 2. masked keys are never loaded ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("hd", MB.HEAD_DIMS)
def test_keys_no_query_allows_may_hold_nan(dtype, hd):
    H, L = 2, 65
    d = H * hd
    enc = _encoder((5, d, 3, H, 1, 20), None, dtype, 2 * L)
    dead = [0, 3, 31, 32, 63, 64]                                            # word and trip boundaries among them
    bias = BB.make_bias("holes", L, H).clone()
    bias[:, :, dead] = NINF
    bias[:, :, 1] = 0.25                                                     # every row keeps a key
    m = enc.make_bias(bias)
    qkv = MB.make_qkv(2, L, H, hd, dtype).cuda()
    obuf = torch.full((2 * L + 2, d), SENTINEL, dtype=TDT[dtype], device="cuda")
    out = obuf[1:-1].view(2, L, d)
    clean = enc.attention(qkv, mask=m, out=out).clone()
    assert bool((obuf[0] == SENTINEL).all()) and bool((obuf[-1] == SENTINEL).all()), "sentinels around out"
    ref, bound = BB.reference_of(qkv, bias, H, dtype)
    r, at = BB.ratio(clean, ref, bound)
    assert r < 1.0, (r, at)
    bad = qkv.clone()
    for poison in (float("nan"), float("inf")):
        bad[:, dead, d:] = poison                                            # k and v of the dead keys; their q rows stay queries
        got = enc.attention(bad, mask=m)
        assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(clean)), poison


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_padding_rows_under_lengths_may_hold_nan(sds, dtype):
    L, lens = 33, [33, 1, 20]
    enc = _encoder(TOY, sds["toy"], dtype, 3 * L)
    m = enc.make_bias(BB.make_bias("alibi", L, 4))
    x = _x(3, L, TOY[0]).cuda()
    ybuf = torch.full((3 * L + 2, TOY[2]), SENTINEL, device="cuda")
    clean = enc(x, lengths=lens, mask=m).clone()
    for poison in (float("nan"), float("inf")):
        xn = x.clone()
        for b, n in enumerate(lens):
            xn[b, n:] = poison
        got = enc(xn, lengths=lens, mask=m)
        assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(clean)), poison
    rc = enc.lib.flope_tf_forward_masked(enc.handle, x.data_ptr(), 3, L, (C.c_int * 3)(*lens), m.handle, ybuf[1:-1].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((ybuf[0] == SENTINEL).all()) and bool((ybuf[-1] == SENTINEL).all()), "sentinels around y"
    assert torch.equal(_bits(ybuf[1:-1].view(3, L, -1)), _bits(clean))


# ---- 3. against fp64 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("hd", MB.HEAD_DIMS)
def test_attention_within_the_derived_bound(dtype, hd):
    """random bias with holes, per-head ALiBi, the edge mask with a bias; H planes and one"""
    H = 2
    enc = _encoder((5, H * hd, 3, H, 1, 20), None, dtype, 2 * 130)
    worst = (0.0, ("", 0))
    for kind in BB.KINDS:
        for L in MB.LENGTHS:
            for planes in (None, 1):
                if planes == 1 and L not in (33, 130):
                    continue
                m = enc.make_bias(BB.make_bias(kind, L, H, planes))
                got = enc.attention(MB.make_qkv(2, L, H, hd, dtype).cuda(), mask=m)
                assert enc.last_attn_kernel == BIASED
                ref, bound = BB.reference(kind, 2, L, H, hd, dtype, None, planes)
                r, at = BB.ratio(got, ref, bound)
                print(f"{dtype} head_dim {hd} {kind} L={L} planes={m.planes}: {r:.3f} of the bound at {at}")
                assert r < 1.0, (kind, L, planes, r, at)
                worst = max(worst, (r, (kind, L)))
                m.close()
    print(f"{dtype} head_dim {hd}: worst {worst[0]:.3f} of the bound at {worst[1]} (headroom {1 / max(worst[0], 1e-9):.1f}x)")


@pytest.fixture(scope="module")
def forward_refs(sds):
    """(shape, kind) -> (x, bias, fp64 restatement); computed once, never changed"""
    out = {}
    for shape, L in (("toy", 33), ("wide", 65)):
        x = _x(2, L, DIMS[shape][0], seed=2)
        for kind in BB.KINDS:
            bias = BB.make_bias(kind, L, DIMS[shape][3])
            out[shape, kind] = (x, bias, BB.biased_forward(sds[shape], x.numpy(), bias.numpy(), num_heads=DIMS[shape][3]))
    return out


@pytest.mark.parametrize("shape", ["toy", "wide"])
@pytest.mark.parametrize("dtype,tol", MODES, ids=lambda v: str(v))
def test_forward_against_the_restatement(sds, forward_refs, shape, dtype, tol):
    dims = DIMS[shape]
    L = forward_refs[shape, "holes"][0].shape[1]
    enc = _encoder(dims, sds[shape], dtype, 2 * L)
    for kind in BB.KINDS:
        x, bias, ref = forward_refs[shape, kind]
        m = enc.make_bias(bias)
        y = enc(x.cuda(), mask=m)
        err = float(np.abs(y.cpu().numpy() - ref).max())
        print(f"{dtype} {shape} {kind} L={L}: |y - fp64|max {err:.3e}, tolerance {tol}")
        assert torch.isfinite(y).all() and err < tol, (kind, err)
        assert enc.last_attn_kernel == BIASED and not enc.last_forward_fused and enc.forward_plan(2, L, mask=m) == "launches"


def test_reference_fixture(sds):
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_bias_fixture.npz"))
    enc = _encoder(TOY, sds["toy"], "f32", 6 * 15, fused=1)
    x = torch.from_numpy(f["x"]).cuda()
    for name in ("alibi", "alibi_h", "rand", "rand_h"):
        m = enc.make_bias(torch.from_numpy(f["bias_" + name]))
        assert m.planes == (4 if name.endswith("_h") else 1)
        y = enc(x, mask=m)
        err = float(np.abs(y.cpu().numpy() - f["y_" + name]).max())
        print(f"f32 toy vs the reference module under the {name} bias: {err:.3e}")
        assert err < 1e-5 and not enc.last_forward_fused
        assert torch.equal(_bits(enc(x, mask=enc.make_bias(torch.from_numpy(f["bias_" + name]).double().cuda()))), _bits(y)), "a float64 device tensor"


def test_alibi_bias_tells_the_order_of_the_past(sds):
    """what the feature is for: the last row of a one-layer causal forward is a function of the SET of poses behind it (only the order
    of the float32 sums changes when two of them change places: rounding noise, held to 1e-5), under ALiBi it is not (held to a
    hundred times that noise bound)"""
    from flope_amd.tf_encoder import alibi_bias
    L = 15
    enc = _encoder(ODD, sds["odd"], "f32", L)
    x = _x(1, L, ODD[0]).cuda()
    xs = x.clone()
    xs[0, [2, 9]] = x[0, [9, 2]]                                             # two poses of the past change places
    m = enc.make_bias(alibi_bias(L, [2.0 ** -(h + 1) for h in range(ODD[3])]))
    plain = float((enc(x, is_causal=True)[0, -1] - enc(xs, is_causal=True)[0, -1]).abs().max())
    biased = float((enc(x, mask=m)[0, -1] - enc(xs, mask=m)[0, -1]).abs().max())
    print(f"last row after swapping poses 2 and 9: causal {plain:.2e}, causal ALiBi {biased:.2e}")
    assert plain < 1e-5 and biased > 1e-3


# ---- 4. ragged ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("kind,planes", [("alibi", None), ("holes", None), ("holes", 1)])
def test_each_sequence_is_itself_alone_under_the_corner(sds, dtype, kind, planes):
    L, lens = 65, [65, 1, 33, 20, 64]
    enc = _encoder(TOY, sds["toy"], dtype, sum(lens))
    bias = BB.make_bias(kind, L, 4, planes)
    m = enc.make_bias(bias)
    x = _x(len(lens), L, TOY[0]).cuda()
    y = enc(x, lengths=lens, mask=m).clone()
    assert enc.last_attn_kernel == BIASED
    ob = torch.from_numpy(np.asarray(sds["toy"]["out_layer.bias"], dtype=np.float32)).cuda()
    qkv = MB.make_qkv(1, sum(lens), 4, 8, dtype).cuda()[0]
    att = enc.attention(qkv, lengths=lens, mask=m).clone()
    o = 0
    for b, n in enumerate(lens):
        corner = enc.make_bias(bias[:, :n, :n])
        assert torch.equal(_bits(y[b, :n]), _bits(enc(x[b:b + 1, :n].contiguous(), mask=corner)[0])), b
        assert torch.equal(y[b, n:], ob.expand(L - n, -1)), b
        assert torch.equal(_bits(att[o:o + n]), _bits(enc.attention(qkv[o:o + n][None].contiguous(), mask=corner)[0])), b
        corner.close()
        o += n
    ref = BB.biased_forward(sds["toy"], x.cpu().numpy(), bias.numpy(), lens)
    assert float(np.abs(y.cpu().numpy() - ref).max()) < dict(MODES)[dtype]
    assert enc.flops(len(lens), L, lengths=lens, mask=m) == enc.flops(len(lens), L, lengths=lens, mask=enc.make_mask(~BB.allowed_of(bias)))


def test_ragged_attention_within_the_bound():
    H, hd, L, lens = 2, 6, 65, (65, 1, 33)
    enc = _encoder((5, H * hd, 3, H, 1, 20), None, "f32", sum(lens))
    qkv = MB.make_qkv(3, L, H, hd, "f32")
    packed = torch.cat([qkv[b, :n] for b, n in enumerate(lens)]).contiguous().cuda()
    for kind in ("alibi", "holes"):
        got = enc.attention(packed, lengths=list(lens), mask=enc.make_bias(BB.make_bias(kind, L, H)))
        ref, bound = BB.reference(kind, 3, L, H, hd, "f32", lens)
        padded = torch.zeros(3, L, H * hd)
        o = 0
        for b, n in enumerate(lens):
            padded[b, :n] = got[o:o + n].cpu()
            o += n
        r, at = BB.ratio(padded, ref, bound, lens)
        print(f"ragged {kind}: {r:.3f} of the bound at {at}")
        assert r < 1.0, (kind, r, at)


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------
def test_other_forwards_keep_their_bits_around_biased_calls(sds):
    L = 15
    enc = _encoder(TOY, sds["toy"], "f32", 6 * L, fused=1)
    x = _x(6, L, TOY[0]).cuda()
    ba, bb = enc.make_bias(BB.make_bias("holes", L, 4)), enc.make_bias(BB.make_bias("alibi", L, 4, 1))
    mk = enc.make_mask(~MB.make_allowed("prefix", L))
    calls = [dict(), dict(is_causal=True), dict(is_causal=True, window=4), dict(lengths=[15, 1, 7, 12, 3, 15]), dict(mask=mk)]
    before, fused = [], []
    for kw in calls:
        before.append(enc(x, **kw).clone())
        fused.append(enc.last_forward_fused)
    assert fused[0] and fused[1] and not fused[2] and not fused[4], "plain and causal are the single launch here"
    ya, yb = enc(x, mask=ba).clone(), enc(x, mask=bb).clone()
    assert float((ya - yb).abs().max()) > 1e-3
    for kw, want, fz in zip(calls, before, fused):
        for m, ym in ((ba, ya), (bb, yb), (ba, ya)):                          # two biases on one handle, alternately
            assert torch.equal(_bits(enc(x, mask=m)), _bits(ym))
            assert not enc.last_forward_fused and enc.last_attn_kernel == BIASED
        assert torch.equal(_bits(enc(x, **kw)), _bits(want)), kw
        assert enc.last_forward_fused == fz, kw
    assert enc.last_attn_kernel == MASKED, "the plain mask after the biases still runs tf_attn_masked"
    # options "causal" / "window" are neither read nor written by a biased call
    enc(x, is_causal=True, window=4)
    enc(x, mask=ba)
    enc.attention(torch.zeros(6, L, 3 * TOY[1], device="cuda"), mask=bb)
    assert enc.last_attn_kernel == BIASED
    assert enc.lib.flope_tf_last_forward(enc.handle) == 0
    assert enc.set_option("window", 4) == 4 and enc.set_option("causal", 1) == 1
    enc(x)
    enc(x, mask=ba)
    assert enc.set_option("causal", 0) == 0 and enc.set_option("window", 0) == 0
    assert enc.last_forward_fused is False and enc(x) is not None and enc.last_forward_fused is True
    bb.close()
    assert torch.equal(_bits(enc(x, mask=ba)), _bits(ya)), "closing one bias leaves the other"


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_make_bias_refusals(sds):
    L = 15
    enc = _encoder(TOY, sds["toy"], "f32", 4 * L)
    x = _x(4, L, TOY[0]).cuda()
    good_bias = BB.make_bias("holes", L, 4)
    m = enc.make_bias(good_bias)
    good = enc(x, mask=m).clone()
    for bad in (torch.zeros(3, 4), torch.zeros(2, 2, 3, 3), torch.zeros(3, 3, dtype=torch.int32), torch.zeros(3, 3, dtype=torch.bool),
                torch.zeros(0, 0), torch.zeros(3)):
        with pytest.raises(ValueError, match="bias must be"):
            enc.make_bias(bad)
    b = good_bias.clone()
    b[2, 7, 3] = float("inf")
    with pytest.raises(ValueError, match=r"\(plane 2, row 7, col 3\) is \+inf or NaN"):
        enc.make_bias(b)
    b[1, 14, 14] = float("nan")
    with pytest.raises(ValueError, match=r"\(plane 1, row 14, col 14\) is \+inf or NaN"):
        enc.make_bias(b)
    with pytest.raises(ValueError, match=r"\(plane 0, row 0, col 1\)"):
        enc.make_bias(torch.zeros(L, L).index_put((torch.tensor(0), torch.tensor(1)), torch.tensor(float("nan"))))
    for planes in (2, 3, 5):
        with pytest.raises(ValueError, match=f"planes = {planes} is neither 1 nor num_heads = 4"):
            enc.make_bias(torch.zeros(planes, L, L))
    b = good_bias.clone()
    b[3, 5, 5] = NINF                                                        # the diagonal is allowed in plane 0
    with pytest.raises(ValueError, match=r"\(plane 3, row 5, col 5\).*large negative finite value"):
        enc.make_bias(b)
    b = torch.zeros(L, L)
    b[6] = NINF
    with pytest.raises(ValueError, match="row 6 has no allowed key"):
        enc.make_bias(b)
    with pytest.raises(ValueError, match="max_tokens"):
        enc.make_bias(torch.zeros(4 * L + 1, 4 * L + 1))
    # the C entry point itself
    lib, out = enc.lib, C.c_void_p()
    one = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)
    assert lib.flope_tf_bias_create(enc.handle, 1, 1, None, C.byref(out)) == EINVAL
    assert lib.flope_tf_bias_create(enc.handle, 1, 1, one, None) == EINVAL
    assert lib.flope_tf_bias_create(enc.handle, 0, 1, one, C.byref(out)) == EINVAL
    assert lib.flope_tf_bias_create(enc.handle, 1, 0, one, C.byref(out)) == EINVAL and not out.value
    assert lib.flope_tf_bias_create(enc.handle, 1, 4, one, C.byref(out)) == 0 and out.value
    n, pairs = C.c_int(), C.c_longlong()
    assert lib.flope_tf_mask_info(out, C.byref(n), C.byref(pairs)) == 0 and (n.value, pairs.value) == (1, 1)
    plain_mask = enc.make_mask(torch.zeros(3, 3))
    assert lib.flope_tf_mask_bias_planes(out) == 4 and lib.flope_tf_mask_bias_planes(plain_mask.handle) == 0 and plain_mask.planes == 0
    assert lib.flope_tf_mask_destroy(out) == 0
    assert torch.equal(_bits(enc(x, mask=m)), _bits(good)), "the next valid call"
    # make_mask keeps refusing what make_bias takes
    with pytest.raises(ValueError, match="additive biases have no kernel"):
        enc.make_mask(good_bias[0])
    with pytest.raises(ValueError, match="mask must be"):
        enc.make_mask(good_bias)


def test_call_refusals_leave_the_buffers_alone(sds):
    L = 15
    enc = _encoder(TOY, sds["toy"], "f32", 4 * L)
    other = _encoder(TOY, sds["toy"], "f32", 4 * L)
    bias = BB.make_bias("alibi", L, 4)
    m, mo = enc.make_bias(bias), other.make_bias(bias)
    x = _x(4, L, TOY[0]).cuda()
    qkv = torch.zeros(4, L, 3 * TOY[1], device="cuda")
    good = enc(x, mask=m).clone()
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
    edge = enc.make_bias(BB.make_bias("edge", L, 4))                          # row 0 sees key L - 1 only
    with pytest.raises(ValueError, match=r"b = 1, row 0 has no allowed key below 9"):
        enc(x, lengths=[15, 9, 15, 15], mask=edge)
    # the C entry points, with sentinels around y and out
    lib = enc.lib
    ybuf = torch.full((4 * L + 2, TOY[2]), SENTINEL, device="cuda")
    obuf = torch.full((4 * L + 2, TOY[1]), SENTINEL, device="cuda")
    y, out = ybuf[1:-1], obuf[1:-1]
    fwd = lambda h, xp, B, Ls, lens, mh, yp: lib.flope_tf_forward_masked(h, xp, B, Ls, lens, mh, yp, None)
    att = lambda h, qp, B, Ls, lens, mh, op: lib.flope_tf_attention_masked(h, qp, B, Ls, lens, mh, op, None)
    for call, src, dst in ((fwd, x, y), (att, qkv, out)):
        assert call(enc.handle, src.data_ptr(), 4, 14, None, m.handle, dst.data_ptr()) == EINVAL
        assert call(enc.handle, src.data_ptr(), 5, L, None, m.handle, dst.data_ptr()) == EINVAL
        assert call(enc.handle, src.data_ptr(), 4, L, None, mo.handle, dst.data_ptr()) == EINVAL
        assert b"another handle" in lib.flope_tf_last_error(enc.handle)
        assert call(enc.handle, src.data_ptr(), 2, L, (C.c_int * 2)(15, 9), edge.handle, dst.data_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((ybuf == SENTINEL).all()) and bool((obuf == SENTINEL).all()), "a refused call wrote something"
    assert fwd(enc.handle, x.data_ptr(), 4, L, None, m.handle, y.data_ptr()) == 0
    assert att(enc.handle, qkv.data_ptr(), 4, L, None, m.handle, out.data_ptr()) == BIASED
    assert lib.flope_tf_last_forward_masked(enc.handle) == BIASED
    torch.cuda.synchronize()
    for buf in (ybuf, obuf):
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()) and not bool((buf[1:-1] == SENTINEL).any())
    assert torch.equal(_bits(y.reshape(4, L, -1)), _bits(good))
    with pytest.raises(ValueError, match="has a kernel"):                    # a plain float tensor as mask= goes where it always went
        enc(x, mask=bias[0])


def test_closed_bias_and_closed_encoder(sds):
    L = 15
    enc = _encoder(TOY, sds["toy"], "f32", L)
    x = _x(1, L, TOY[0]).cuda()
    m, keep = enc.make_bias(BB.make_bias("alibi", L, 4)), enc.make_bias(BB.make_bias("holes", L, 4, 1))
    enc(x, mask=m)
    m.close()
    m.close()
    with pytest.raises(RuntimeError, match="mask has been closed"):
        enc(x, mask=m)
    with pytest.raises(RuntimeError, match="mask has been closed"):
        enc.attention(torch.zeros(1, L, 3 * TOY[1], device="cuda"), mask=m)
    handle, lib = keep.handle, enc.lib
    enc.close()
    with pytest.raises(RuntimeError, match="encoder of this mask has been closed"):
        enc(x, mask=keep)
    with pytest.raises(RuntimeError, match="closed"):
        enc.make_bias(torch.zeros(L, L))
    assert lib.flope_tf_mask_bias_planes(handle) == ESTATE                   # the biases ended with the handle
    keep.close()                                                             # frees the host part only
