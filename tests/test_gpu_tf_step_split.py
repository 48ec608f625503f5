"""Option step_split on the device (tf_attn_step_split / tf_attn_extend_split).

Under the option a step's attention splits the token's visible keys over the four waves of a workgroup.  The result is no longer the
causal forward's bits; it is held (1) element-wise to fp64 within the bound tests/tf_step_split_bound.py derives from the row's
operation counts, through st.attention, which runs the step's attention launch alone; (2) as whole steps to the fp64 restatement of
the causal forward within the stream tests' tolerances; (3) in bits to itself: the same call twice, a row whatever else the call
holds, extend against steps for any chunking, a ring at any capacity and against a linear state while p < W, and option 0's bits
where the shape keeps the row kernel; (4) the option's hygiene.
"""
import os

import numpy as np
import pytest
import torch

import tf_attn_causal_bound as CB
import tf_step_split_bound as SB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = SB.TDT
ROW, SPLIT = 0, 1
SENTINEL = 1234.0
TOY = (16, 32, 9, 4, 2, 64)          # head_dim 8
WIDE = (16, 128, 9, 2, 2, 256)       # head_dim 64
ODD = (5, 30, 3, 5, 1, 20)           # head_dim 6: no whole 16-byte vectors, the option keeps tf_attn_step
TOL = {"f32": 2e-4, "f32m": 2e-4, "f16": 1.5e-2, "bf16": 1.2e-1}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sd_t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _encoder(dims, sd, dtype, max_tokens, step_split=0):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, step_split=step_split)
    if sd is not None:
        enc.load_state_dict(_sd_t(sd))
    return enc


def _attn_encoder(H, hd, dtype, n, step_split):
    """an encoder whose only use is st.attention: one layer, no weights"""
    return _encoder((4, H * hd, 3, H, 1, 8), None, dtype, max(n, 8), step_split)


@pytest.fixture(scope="module")
def shapes():
    """name -> (dims, state dict, x [n, L, in], fp64 causal restatement of x); computed once, never changed"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_causal_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    tx = np.random.default_rng(3).standard_normal((2, 300, TOY[0])).astype(np.float32)
    wsd = T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)
    wx = np.random.default_rng(1).standard_normal((3, 50, WIDE[0])).astype(np.float32)
    osd = T.synthetic_state_dict(ODD[0], ODD[1], ODD[2], ODD[4], ODD[5], seed=6)
    res = {"toy": (TOY, sd, tx), "wide": (WIDE, wsd, wx)}
    out = {k: v + (CB.causal_forward(v[1], v[2], v[0][3]),) for k, v in res.items()}
    out["odd"] = (ODD, osd, np.random.default_rng(2).standard_normal((2, 40, ODD[0])).astype(np.float32), None)
    return out


# ---- 1. attention alone, element-wise ---------------------------------------------------------------------------------------------------
def _attention_case(dtype, n, L, H, hd, lengths=None, window=0, capacity=None):
    qkv = SB.make_qkv(n, L, H, hd, dtype)
    ref, bound = SB.reference(n, L, H, hd, dtype, None if lengths is None else tuple(lengths), window)
    enc = _attn_encoder(H, hd, dtype, n, 0)
    st = enc.open_stream(n, capacity or L, window=window)
    qg = qkv.cuda()
    ratios = {}
    for opt in (1, 0):
        enc.set_option("step_split", opt)
        got = st.attention(qg, lengths=lengths)
        want = SPLIT if opt and SB.step_split_ok(hd, dtype) else ROW
        assert st.last_attn_kernel == want and st.step_plan == ("split" if want == SPLIT else "row")
        ratios[opt], where = SB.ratio(got, ref, bound)
        assert st.positions == [0] * n
    print(f"{dtype} n={n} L={L} H={H} hd={hd} lengths={lengths} W={window} cap={capacity}: max |err| / bound  split {ratios[1]:.3f}  row {ratios[0]:.3f}")
    st.close(); enc.close()
    assert ratios[1] <= 1.0, f"step_split: {ratios[1]:.3f} of the bound"
    if dtype == "f32":
        assert ratios[0] <= 1.0, f"the row kernel through the hook: {ratios[0]:.3f} of the bound"


@pytest.mark.parametrize("case", SB.CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_attention_within_the_bound(dtype, case):
    assert SB.step_split_ok(case[3], dtype)
    _attention_case(dtype, *case)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_attention_ragged_lengths(dtype):
    _attention_case(dtype, *SB.RAGGED[0], lengths=SB.RAGGED[1])


@pytest.mark.parametrize("capacity", SB.WINDOW_CASE[5])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_attention_on_a_ring(dtype, capacity):
    n, L, H, hd, W, _ = SB.WINDOW_CASE
    _attention_case(dtype, n, L, H, hd, window=W, capacity=capacity)


# ---- 2. whole steps against fp64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pre", [("toy", 255), ("wide", 0)])
@pytest.mark.parametrize("dtype", ["f32", "f32m", "f16", "bf16"])
def test_steps_follow_the_fp64_forward(shapes, dtype, shape, pre):
    dims, sd, x, full = shapes[shape]
    n, L = x.shape[0], x.shape[1]
    xg = torch.from_numpy(x).cuda()
    errs = {}
    for opt in (0, 1):
        enc = _encoder(dims, sd, dtype, n * L, opt)
        st = enc.open_stream(n, L)
        assert st.step_plan == ("split" if opt else "row")
        if pre:
            st.prefill(xg[:, :pre])
        rows = torch.stack([st.step(xg[:, t]).clone() for t in range(pre, L)], dim=1)
        assert st.positions == [L] * n
        errs[opt] = float(np.abs(rows.cpu().numpy() - full[:, pre:]).max())
        st.close(); enc.close()
    print(f"{dtype} {shape}: steps {pre} .. {L - 1}: |y - fp64|max  option 0 {errs[0]:.3e}  option 1 {errs[1]:.3e}  tolerance {TOL[dtype]}")
    assert errs[0] < TOL[dtype] and errs[1] < TOL[dtype]


# ---- 3. bits -------------------------------------------------------------------------------------------------------------------------------
def _feed(st, x, chunks, tracks=None):
    """tokens of x [n, L, in] in extend() calls of the given chunk lengths (1: a step()) -> [n, sum(chunks), out]"""
    out, t = [], 0
    for c in chunks:
        out.append(st.step(x[:, t], tracks).clone()[:, None] if c == 1 else st.extend(x[:, t:t + c], tracks=tracks).clone())
        t += c
    return torch.cat(out, dim=1)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_same_call_twice(shapes, dtype):
    dims, sd, x, _ = shapes["toy"]
    xg = torch.from_numpy(x[:, :80]).cuda()
    enc = _encoder(dims, sd, dtype, 256, 1)
    a, b = enc.open_stream(2, 128), enc.open_stream(2, 128)
    assert torch.equal(_bits(_feed(a, xg, [70] + [1] * 10)), _bits(_feed(b, xg, [70] + [1] * 10)))
    qkv = SB.make_qkv(2, 100, dims[3], dims[1] // dims[3], dtype).cuda()
    assert torch.equal(_bits(a.attention(qkv).clone()), _bits(a.attention(qkv)))
    a.close(); b.close(); enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_row_knows_nothing_of_the_call(shapes, dtype):
    """tracks=[2, 0, 5] of a six-track state against each track alone in a fresh state, and in another row order"""
    dims, sd, x, _ = shapes["toy"]
    x3 = torch.from_numpy(np.concatenate([x[:, :75], x[:1, 100:175]])).cuda()          # three different tracks
    enc = _encoder(dims, sd, dtype, 512, 1)
    big = enc.open_stream(6, 128)
    chunks = [70, 1, 1, 2, 1]
    got = _feed(big, x3, chunks, [2, 0, 5])
    assert big.positions == [75, 0, 75, 0, 0, 75]
    for r in range(3):
        one = enc.open_stream(1, 100)
        assert torch.equal(_bits(_feed(one, x3[r:r + 1], chunks)[0]), _bits(got[r])), f"row {r} alone"
        one.close()
    perm = enc.open_stream(6, 77)
    back = _feed(perm, x3[[2, 0, 1]], chunks, [5, 2, 0])
    assert torch.equal(_bits(back[[1, 2, 0]]), _bits(got))
    big.close(); perm.close(); enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_extend_equals_steps_for_any_chunking(shapes, dtype):
    dims, sd, x, _ = shapes["toy"]
    chunks = [1, 7, 64, 65]
    T = sum(chunks)
    xg = torch.from_numpy(x[:, :T + 3]).cuda()
    enc = _encoder(dims, sd, dtype, 512, 1)
    a, s, c = enc.open_stream(2, 160), enc.open_stream(2, 160), enc.open_stream(2, 160)
    assert a.step_plan == "split"
    ya, ys, yc = _feed(a, xg[:, :T], chunks), _feed(s, xg[:, :T], [1] * T), _feed(c, xg[:, :T], [65, 64, 7, 1])
    assert torch.equal(_bits(ya), _bits(ys)) and torch.equal(_bits(yc), _bits(ys))
    tail = [_feed(t, xg[:, T:], [1, 1, 1]) for t in (a, s, c)]                     # the caches hold the same bits
    assert torch.equal(_bits(tail[0]), _bits(tail[1])) and torch.equal(_bits(tail[2]), _bits(tail[1]))
    a.close(); s.close(); c.close(); enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_ring_of_any_capacity_and_a_linear_state_while_young(shapes, dtype):
    dims, sd, x, _ = shapes["toy"]
    W = 70
    xg = torch.from_numpy(x[:, :160]).cuda()
    enc = _encoder(dims, sd, dtype, 512, 1)
    r70, r96, lin = enc.open_stream(2, 70, window=W), enc.open_stream(2, 96, window=W), enc.open_stream(2, 160)
    young = [60, 1, 1, 8]                                                          # positions 0 .. 69: p < W
    y70, y96, yl = (_feed(t, xg[:, :70], young) for t in (r70, r96, lin))
    assert torch.equal(_bits(y70), _bits(y96)) and torch.equal(_bits(y70), _bits(yl))
    later = [1, 1, 30, 1, 50, 1, 1, 5]                                             # the window slides, both rings wrap, a chunk wraps
    z70, z96 = (_feed(t, xg[:, 70:160], later) for t in (r70, r96))
    assert torch.equal(_bits(z70), _bits(z96))
    zl = _feed(lin, xg[:, 70:72], [1, 1])                                          # ... and the linear state has left them: more keys
    assert not torch.equal(_bits(zl[:, 1]), _bits(z70[:, 1]))
    for t in (r70, r96, lin):
        t.close()
    enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_an_ineligible_head_dim_keeps_the_row_kernel_and_its_bits(shapes, dtype):
    dims, sd, x, _ = shapes["odd"]
    xg = torch.from_numpy(x).cuda()
    out = []
    for opt in (0, 1):
        enc = _encoder(dims, sd, dtype, 256, opt)
        st = enc.open_stream(2, 64)
        assert st.step_plan == "row" and not SB.step_split_ok(dims[1] // dims[3], dtype)
        out.append(_feed(st, xg, [1, 1, 20, 1, 17]))
        st.close(); enc.close()
    assert torch.equal(_bits(out[0]), _bits(out[1]))


# ---- 4. option hygiene -------------------------------------------------------------------------------------------------------------------
def test_the_option_takes_zero_or_one(shapes):
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, "f32", 64)
    assert enc.set_option("step_split", 1) == 0 and enc.set_option("step_split", 1) == 1      # the old value comes back
    for bad in (2, -1):
        with pytest.raises(ValueError):
            enc.set_option("step_split", bad)
    assert enc.set_option("step_split", 0) == 1
    with pytest.raises(ValueError):
        TransformerEncoder(*dims, dtype="f32", max_tokens=64, step_split=2)
    enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_flipped_mid_track(shapes, dtype):
    dims, sd, x, full = shapes["toy"]
    xg = torch.from_numpy(x[:, :90]).cuda()
    enc = _encoder(dims, sd, dtype, 256)
    st = enc.open_stream(2, 128)
    rows = []
    for lo, hi, opt in ((0, 40, 0), (40, 70, 1), (70, 80, 0), (80, 90, 1)):
        enc.set_option("step_split", opt)
        assert st.step_plan == ("split" if opt else "row")
        rows.append(_feed(st, xg[:, lo:hi], [hi - lo - 2, 1, 1]))
        assert st.positions == [hi, hi]
    err = float(np.abs(torch.cat(rows, dim=1).cpu().numpy() - full[:, :90]).max())
    print(f"{dtype}: option flipped at 40, 70, 80: |y - fp64|max {err:.3e}, tolerance {TOL[dtype]}")
    assert err < TOL[dtype]
    st.close(); enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_forward_and_prefill_keep_their_bits(shapes, dtype):
    dims, sd, x, _ = shapes["toy"]
    xg = torch.from_numpy(x[:, :100]).cuda()
    enc = _encoder(dims, sd, dtype, 256)
    st = enc.open_stream(2, 128)
    want_f, want_p = enc(xg, is_causal=True).clone(), st.prefill(xg).clone()
    want_a = enc.attention(SB.make_qkv(2, 100, dims[3], dims[1] // dims[3], dtype).cuda(), is_causal=True).clone()
    enc.set_option("step_split", 1)
    st.reset()
    assert torch.equal(_bits(enc(xg, is_causal=True)), _bits(want_f)) and torch.equal(_bits(st.prefill(xg)), _bits(want_p))
    assert torch.equal(_bits(enc.attention(SB.make_qkv(2, 100, dims[3], dims[1] // dims[3], dtype).cuda(), is_causal=True)), _bits(want_a))
    st.close(); enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_sentinels_around_y_and_att(shapes, dtype):
    dims, sd, x, _ = shapes["toy"]
    n, o, d = 2, dims[2], dims[1]
    xg = torch.from_numpy(x[:, :70]).cuda()
    enc = _encoder(dims, sd, dtype, 256, 1)
    st = enc.open_stream(n, 128)
    st.extend(xg[:, :66])
    big = torch.full((64 + n * o + 64,), SENTINEL, device="cuda")
    y = st.step(xg[:, 66], out=big[64:64 + n * o].view(n, o))
    assert (big[:64] == SENTINEL).all() and (big[64 + n * o:] == SENTINEL).all() and torch.isfinite(y).all()
    big = torch.full((64 + n * 3 * o + 64,), SENTINEL, device="cuda")
    y = st.extend(xg[:, 67:70], out=big[64:64 + n * 3 * o].view(n, 3, o))
    assert (big[:64] == SENTINEL).all() and (big[64 + n * 3 * o:] == SENTINEL).all() and torch.isfinite(y).all()
    biga = torch.full((64 + n * d + 64,), SENTINEL, device="cuda", dtype=TDT[dtype])
    att = st.attention(SB.make_qkv(n, 100, dims[3], d // dims[3], dtype).cuda(), lengths=[100, 3], out=biga[64:64 + n * d].view(n, d))
    assert (biga[:64] == SENTINEL).all() and (biga[64 + n * d:] == SENTINEL).all() and torch.isfinite(att.float()).all()
    assert st.last_attn_kernel == SPLIT
    st.close(); enc.close()


def test_closed_stream_and_closed_encoder_raise(shapes):
    dims, sd, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, "f32", 64, 1)
    st, st2 = enc.open_stream(2, 16), enc.open_stream(2, 16)
    qkv = torch.zeros(2, 4, 3 * dims[1], device="cuda")
    st.close()
    with pytest.raises(RuntimeError):
        st.step_plan
    with pytest.raises(RuntimeError):
        st.attention(qkv)
    enc.close()
    with pytest.raises(RuntimeError):
        st2.step_plan
    with pytest.raises(RuntimeError):
        st2.attention(qkv)
    st2.close()


def test_attention_refusals_leave_the_state_usable(shapes):
    dims, sd, x, _ = shapes["toy"]
    d = dims[1]
    enc = _encoder(dims, sd, "f32", 64, 1)
    st = enc.open_stream(2, 16)
    xg = torch.from_numpy(x[:, :5]).cuda()
    _feed(st, xg[:, :3], [3])
    ok = torch.zeros(2, 8, 3 * d, device="cuda")
    with pytest.raises(ValueError):
        st.attention(torch.zeros(3, 8, 3 * d, device="cuda"))                      # n above the state's tracks
    with pytest.raises(ValueError):
        st.attention(ok, lengths=[0, 3])                                           # a length below 1
    with pytest.raises(ValueError):
        st.attention(ok, lengths=[9, 3])                                           # ... above seq_len
    with pytest.raises(ValueError):
        st.attention(torch.zeros(2, 17, 3 * d, device="cuda"))                     # a linear state: above capacity
    assert enc.lib.flope_tf_stream_attention(st.state, None, 2, 8, None, None, None) == -1      # NULL buffers
    with pytest.raises(ValueError):
        st.attention(torch.zeros(0, 8, 3 * d, device="cuda"))                      # n below 1
    assert st.positions == [3, 3]
    other = enc.open_stream(2, 16)
    _feed(other, xg[:, :3], [3])
    assert torch.equal(_bits(_feed(st, xg[:, 3:], [1, 1])), _bits(_feed(other, xg[:, 3:], [1, 1])))
    assert st.attention(ok).shape == (2, d) and st.positions == [0, 0]             # the hook itself puts its tracks back to 0
    st.close(); other.close(); enc.close()
