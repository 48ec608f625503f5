"""Encoder streams under a distance table on the device (enc.open_stream(..., bias=table), flope_tf_stream_open_bias).

The contract: a stream opened with a table [planes, D] returns, from step(), extend() and prefill(), the rows of the forward under
enc.make_bias(distance_bias(table, L, window)) IN BITS -- in every dtype and under every option, because a compiled bias sends each of
them to tf_attn_masked's BIASED form (last_attn_kernel == 6, read, not assumed), whose order over a contiguous key range is the
streamed row's.  Against the fp64 restatement (tests/tf_attn_bias_bound.py) the rows keep DESIGN.md 39's tolerances, and the attention
launches alone (st.attention, st.attention_extend) its element-wise bound; nothing is fitted here.

  1. steps, every mode on two shapes            6. options do not reach a biased state
  2. prefill, then steps on permuted tracks     7. element-wise against fp64 within the derived bound
  3. rings: the wrap at every phase             8. isolation: NaN in rows a track does not hold, sentinels, other calls' bits
  4. extend = the same steps; any split         9. order is visible
  5. a zero table is the unbiased stream       10. refusals
"""
import os

import numpy as np
import pytest
import torch

import tf_attn_bias_bound as BB
import tf_attn_mask_bound as MB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = MB.TDT
BIASED = 6
STEP_BIASED, EXTEND_BIASED = 2, 3
SENTINEL = 1234.0
TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)
ODD = (5, 30, 3, 5, 1, 20)           # head_dim 6: scalar loads
MID = (5, 24, 3, 2, 1, 20)           # head_dim 12
MODES = [("f32", 0, 2e-4), ("f32m", 0, 2e-4), ("f16", 0, 1.5e-2), ("f16", 1, 1.5e-2), ("bf16", 0, 1.2e-1), ("bf16", 1, 1.2e-1)]
KINDS = ("alibi_h", "alibi_1", "rand_1", "rand_h")


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _encoder(dims, sd, dtype, max_tokens, **kw):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, **kw)
    if sd is not None:
        enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return enc


def _table(kind, H, D):
    """float32 [planes, D]: per-head ALiBi 2^-(h + 1), a one-plane ALiBi, randn tables with one plane and with H"""
    from flope_amd.tf_encoder import alibi_distances
    if kind == "alibi_h":
        return alibi_distances(D, [2.0 ** -(h + 1) for h in range(H)])
    if kind == "alibi_1":
        return alibi_distances(D, [0.25])
    g = torch.Generator().manual_seed(17 + D)
    return 2 * torch.randn(1 if kind == "rand_1" else H, D, generator=g)


def _expanded(table, L, window=0):
    from flope_amd.tf_encoder import distance_bias
    return distance_bias(table, L, window=window)


def _forward(enc, x, table, window=0, lengths=None):
    """the forward under the table's compiled bias; the attention kernel is read"""
    m = enc.make_bias(_expanded(table, x.shape[1], window))
    y = enc(x, lengths=lengths, mask=m).clone()
    assert enc.last_attn_kernel == BIASED, enc.last_attn_kernel
    m.close()
    return y


def _walk(st, x, tracks=None):
    return torch.stack([st.step(x[:, t].contiguous(), tracks) for t in range(x.shape[1])], dim=1)


@pytest.fixture(scope="module")
def shapes():
    """name -> (dims, state dict, x [B, L, in], lengths); computed once, never changed"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_causal_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    wsd = T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)
    wx = np.random.default_rng(1).standard_normal((3, 50, 16)).astype(np.float32)
    return {"toy": (TOY, sd, f["x"], [int(v) for v in f["lengths"]]), "wide": (WIDE, wsd, wx, [50, 1, 33]),
            "odd": (ODD, T.synthetic_state_dict(ODD[0], ODD[1], ODD[2], ODD[4], ODD[5], seed=7), None, None),
            "mid": (MID, T.synthetic_state_dict(MID[0], MID[1], MID[2], MID[4], MID[5], seed=7), None, None)}


_REFS = {}


def _ref64(shapes, shape, kind):
    """the fp64 restatement of the biased forward of a shape's x under a table kind; computed once and shared"""
    if (shape, kind) not in _REFS:
        dims, sd, x, _ = shapes[shape]
        _REFS[shape, kind] = BB.biased_forward(sd, x, _expanded(_table(kind, dims[3], x.shape[1]), x.shape[1]).numpy(), num_heads=dims[3])
    return _REFS[shape, kind]


# ---- 1. steps are the biased forward's rows, in bits, in every mode -------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "toy"])
@pytest.mark.parametrize("kind", ["alibi_h", "rand_1"])
@pytest.mark.parametrize("dtype,tiled,tol", MODES, ids=lambda v: str(v))
def test_all_steps(shapes, shape, kind, dtype, tiled, tol):
    dims, sd, x, _ = shapes[shape]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L, attn_tiled=tiled)
    xg = torch.from_numpy(x).cuda()
    table = _table(kind, dims[3], L)
    want = _forward(enc, xg, table)
    st = enc.open_stream(B, L, bias=table)
    assert st.bias_planes == table.shape[0] and st.step_plan == "biased" and st.extend_plan() == "biased"
    got = _walk(st, xg)
    torch.cuda.synchronize()
    assert st.positions == [L] * B and torch.isfinite(got).all()
    diff = int((_bits(got) != _bits(want)).sum())
    full = _ref64(shapes, shape, kind)
    err, ferr = float(np.abs(got.cpu().numpy() - full).max()), float(np.abs(want.cpu().numpy() - full).max())
    print(f"{dtype} attn_tiled={tiled} {shape} {kind}: {diff} elements differ in bits; steps |y - fp64|max {err:.3e}, the forward's {ferr:.3e}, tolerance {tol}")
    assert diff == 0, f"{diff} elements of the stepped rows differ in bits from the biased forward"
    assert err < tol
    st.close(); enc.close()


# ---- 2. prefill, then steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", [("toy", "rand_h"), ("toy", "alibi_1"), ("wide", "alibi_h")])
@pytest.mark.parametrize("dtype,tiled", [("f32", 0), ("f32m", 0), ("f16", 1), ("bf16", 0)])
def test_prefill_then_steps(shapes, shape, kind, dtype, tiled):
    dims, sd, x, lens = shapes[shape]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L, attn_tiled=tiled)
    xg = torch.from_numpy(x).cuda()
    table = _table(kind, dims[3], L)
    want = _forward(enc, xg, table)
    half = [max(1, n // 2) for n in lens]
    st = enc.open_stream(B, L, bias=table)
    pre = st.prefill(xg, lengths=half)
    assert torch.equal(_bits(pre), _bits(_forward(enc, xg, table, lengths=half))), "prefill is not the ragged biased forward"
    assert st.positions == half
    for t in range(min(half), L):
        rows = [b for b in reversed(range(B)) if half[b] <= t < lens[b]]            # permuted track subsets
        if not rows:
            continue
        y = st.step(torch.stack([xg[b, t] for b in rows]), rows)
        assert torch.equal(_bits(y), _bits(torch.stack([want[b, t] for b in rows]))), f"step {t} behind the prefill"
    assert st.positions == lens
    # ... on tracks given in another order than the sequences
    perm = list(reversed(range(B)))
    pre2 = st.prefill(xg, lengths=half, tracks=perm)
    assert torch.equal(_bits(pre2), _bits(pre)) and [st.position(perm[b]) for b in range(B)] == half
    b = max(range(B), key=lambda i: lens[i] - half[i])
    if half[b] < L:
        y = st.step(xg[b:b + 1, half[b]].contiguous(), [perm[b]])
        assert torch.equal(_bits(y[0]), _bits(want[b, half[b]]))
    st.close(); enc.close()


# ---- 3. rings -------------------------------------------------------------------------------------------------------------------------
def _ring_rows(enc, xg, table, W, positions):
    """row p of the forward of the track so far (p + 1 tokens) under the windowed expansion, for each p"""
    return {p: _forward(enc, xg[:, :p + 1].contiguous(), table, window=W)[:, p].clone() for p in positions}


@pytest.mark.parametrize("shape", ["odd", "mid"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_rings(shapes, shape, dtype):
    dims, sd = shapes[shape][:2]
    H, n = dims[3], 2
    enc = _encoder(dims, sd, dtype, n * 91)
    xg = torch.randn(n, 91, dims[0], generator=torch.Generator().manual_seed(6)).cuda()
    # (capacity 8, W 5) walked to position 20: both runs short, the wrap at every phase
    table = _table("rand_h", H, 5)
    want = _ring_rows(enc, xg, table, 5, range(21))
    st = enc.open_stream(n, 8, window=5, bias=table)
    assert st.bias_planes == H and st.step_plan == "biased"
    for p in range(21):
        y = st.step(xg[:, p].contiguous())
        assert torch.equal(_bits(y), _bits(want[p])), f"(8, 5) position {p}"
    st.close()
    # (capacity 40, W 36) prefilled and walked through positions 35, 55 - 60, 79, 90
    table = _table("alibi_h", H, 36)
    check = [35, 55, 56, 57, 58, 59, 60, 79, 90]
    want = _ring_rows(enc, xg, table, 36, check)
    st = enc.open_stream(n, 40, window=36, bias=table)
    pre = st.prefill(xg[:, :30].contiguous(), lengths=[30, 17])
    assert torch.equal(_bits(pre), _bits(_forward(enc, xg[:, :30].contiguous(), table, window=36, lengths=[30, 17])))
    for p in range(17, 30):
        st.step(xg[1:2, p].contiguous(), [1])
    for p in range(30, 91):
        y = st.step(xg[:, p].contiguous())
        if p in want:
            assert torch.equal(_bits(y), _bits(want[p])), f"(40, 36) position {p}"
    assert st.positions == [91, 91]
    # a ring may be prefilled with more tokens than its capacity
    pre = st.prefill(xg[:, :60].contiguous())
    assert torch.equal(_bits(pre), _bits(_forward(enc, xg[:, :60].contiguous(), table, window=36)))
    assert torch.equal(_bits(st.step(xg[:, 60].contiguous())), _bits(want[60]))
    st.close(); enc.close()


# ---- 4. extend ------------------------------------------------------------------------------------------------------------------------
POSITIONS = [0, 1, 15, 16, 17, 33, 63, 64, 65]


@pytest.mark.parametrize("shape,dtype", [("toy", "f32"), ("toy", "f16"), ("odd", "bf16"), ("mid", "f32")])
def test_extend_is_the_same_steps(shapes, shape, dtype):
    dims, sd = shapes[shape][:2]
    H, n, cap = dims[3], len(POSITIONS), 72
    enc = _encoder(dims, sd, dtype, n * cap)
    xg = torch.randn(n, cap, dims[0], generator=torch.Generator().manual_seed(8)).cuda()
    table = _table("rand_h" if shape == "toy" else "alibi_h", H, cap)
    want = _forward(enc, xg, table)
    held = [b for b in range(n) if POSITIONS[b]]

    def state():
        st = enc.open_stream(n, cap, bias=table)
        st.prefill(xg[held, :65].contiguous(), lengths=[POSITIONS[b] for b in held], tracks=held)
        assert st.positions == POSITIONS
        return st

    for k in (1, 2, 8):
        lens = [min(k, cap - 1 - p) for p in POSITIONS]                      # room for the step behind the chunk
        chunk = torch.zeros(n, k, dims[0], device="cuda")
        for b, p in enumerate(POSITIONS):
            chunk[b, :lens[b]] = xg[b, p:p + lens[b]]
        a, s = state(), state()
        assert a.extend_plan() == "biased"
        ya = a.extend(chunk, lengths=lens)
        for i in range(k):
            rows = [b for b in range(n) if i < lens[b]]
            ys = s.step(torch.stack([chunk[b, i] for b in rows]), rows)
            for r, b in enumerate(rows):
                assert torch.equal(_bits(ya[b, i]), _bits(ys[r])), f"extend of {k}: track at {POSITIONS[b]}, token {i}"
                assert torch.equal(_bits(ys[r]), _bits(want[b, POSITIONS[b] + i])), f"step at {POSITIONS[b] + i} is not the forward's row"
        assert a.positions == s.positions == [p + l for p, l in zip(POSITIONS, lens)]
        nxt = torch.stack([xg[b, POSITIONS[b] + lens[b]] for b in range(n)])      # the cache, by a following step
        assert torch.equal(_bits(a.step(nxt)), _bits(s.step(nxt))), f"the cache behind an extend of {k}"
        a.close(); s.close()
    # two different splits of one track give the same bits, and the steps'
    outs = []
    for split in ([13, 27], [1, 8, 31], [1] * 40):
        st = enc.open_stream(n, cap, bias=table)
        rows, p = [], 0
        for ln in split:
            rows.append(st.extend(xg[3:4, p:p + ln].contiguous(), tracks=[5])[0])
            p += ln
        outs.append(torch.cat(rows))
        st.close()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
    assert torch.equal(_bits(outs[0]), _bits(want[3, :40]))
    enc.close()


@pytest.mark.parametrize("shape,dtype", [("odd", "f32"), ("mid", "f16"), ("odd", "bf16")])
@pytest.mark.parametrize("cap,W,chunks", [(8, 5, [3, 6, 1, 5, 6]), (40, 36, [30, 9, 1, 12, 39])])
def test_extend_on_rings(shapes, shape, dtype, cap, W, chunks):
    """chunks longer than capacity - W + 1 among them: the append runs behind the attention"""
    dims, sd = shapes[shape][:2]
    H, n, total = dims[3], 2, sum(chunks)
    assert max(chunks) > cap - W + 1
    enc = _encoder(dims, sd, dtype, n * total)
    xg = torch.randn(n, total, dims[0], generator=torch.Generator().manual_seed(9)).cuda()
    table = _table("rand_1" if cap == 8 else "alibi_h", H, W)
    want = _forward(enc, xg, table, window=W)
    a, s = enc.open_stream(n, cap, window=W, bias=table), enc.open_stream(n, cap, window=W, bias=table)
    steps = _walk(s, xg)
    assert torch.equal(_bits(steps), _bits(want))
    p = 0
    for ln in chunks:
        y = a.extend(xg[:, p:p + ln].contiguous())
        assert torch.equal(_bits(y), _bits(steps[:, p:p + ln])), f"chunk of {ln} at {p}"
        p += ln
    assert a.positions == s.positions == [total] * n
    a.close(); s.close(); enc.close()


# ---- 5. a zero table is the unbiased stream -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("cap,W", [(15, 0), (8, 5)])
def test_zero_table_is_the_unbiased_stream(shapes, dtype, cap, W):
    dims, sd, x, lens = shapes["toy"]
    B, L, H = x.shape[0], x.shape[1], dims[3]
    enc = _encoder(dims, sd, dtype, B * L)
    xg = torch.from_numpy(x).cuda()
    short = [min(n, 7) for n in lens]

    def run(st):
        out = [st.prefill(xg, lengths=short).clone() if not W else st.prefill(xg, lengths=lens).clone()]
        st.reset()
        out.append(_walk(st, xg[:, :9].contiguous()).clone())
        out.append(st.extend(xg[:, 9:15].contiguous(), lengths=[6, 1, 3, 6, 2, 5]).clone())
        return out

    plain = enc.open_stream(B, cap, window=W)
    want = run(plain)
    assert plain.bias_planes == 0 and plain.step_plan == "row"
    for planes in (1, H):
        st = enc.open_stream(B, cap, window=W, bias=torch.zeros(planes, W or cap))
        assert st.bias_planes == planes and st.step_plan == "biased"
        for g, w, what in zip(run(st), want, ("prefill", "steps", "extend")):
            assert torch.equal(_bits(g), _bits(w)), f"{what}, {planes} plane(s)"
        st.close()
    plain.close(); enc.close()


# ---- 6. options do not reach a biased state -------------------------------------------------------------------------------------------
def test_options_do_not_reach_a_biased_state(shapes):
    dims, sd, x, _ = shapes["wide"]                                           # head_dim 64: step_split and extend_mfma are both eligible
    B, L, H = x.shape[0], x.shape[1], dims[3]
    enc = _encoder(dims, sd, "f16", B * L)
    xg = torch.from_numpy(x).cuda()
    table = _table("alibi_h", H, L)

    def run():
        st = enc.open_stream(B, L, bias=table)
        plans = (st.step_plan, st.extend_plan())
        y = torch.cat([_walk(st, xg[:, :20].contiguous()), st.extend(xg[:, 20:].contiguous())], dim=1).clone()
        qkv = MB.make_qkv(B, L, H, dims[1] // H, "f16").cuda()
        a = st.attention(qkv).clone()
        ka = st.last_attn_kernel
        e = st.attention_extend(qkv, [L] * B, [L - 9] * B).clone()
        ke = st.last_attn_kernel
        st.close()
        return plans, y, a, e, (ka, ke)

    off = run()
    assert off[0] == ("biased", "biased") and off[4] == (STEP_BIASED, EXTEND_BIASED)
    assert torch.equal(_bits(off[1]), _bits(_forward(enc, xg, table)))
    plain = enc.open_stream(B, L)
    for name, step_plan, extend_plan in (("step_split", "split", "split"), ("extend_mfma", "row", "mfma")):
        enc.set_option(name, 1)
        on = run()
        assert on[0] == ("biased", "biased") and on[4] == (STEP_BIASED, EXTEND_BIASED), name
        for g, w in zip(on[1:4], off[1:4]):
            assert torch.equal(_bits(g), _bits(w)), name
        # an unbiased state on the same handle still reports and runs the option's kernels
        assert (plain.step_plan, plain.extend_plan()) == (step_plan, extend_plan), name
        qkv = MB.make_qkv(B, L, H, dims[1] // H, "f16").cuda()
        plain.attention(qkv)
        assert plain.last_attn_kernel == (1 if step_plan == "split" else 0)
        plain.attention_extend(qkv, [L] * B, [L - 9] * B)
        assert plain.last_attn_kernel == (2 if extend_plan == "mfma" else 1)
        enc.set_option(name, 0)
    plain.close(); enc.close()


# ---- 7. element-wise against fp64 within the derived bound ----------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("hd", [6, 64])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("W", [0, 36])
def test_attention_within_the_derived_bound(dtype, hd, W):
    H, L = 2, 130
    lens = [1, 15, 65, 130]
    B, d = len(lens), H * hd
    enc = _encoder((4, d, 3, H, 1, 8), None, dtype, B * L)
    qkv = MB.make_qkv(B, L, H, hd, dtype).cuda()
    worst = 0.0
    for kind in ("alibi_h", "rand_h", "rand_1"):
        table = _table(kind, H, W or L)
        O, bound = BB.reference_of(qkv, _expanded(table, L, window=W), H, dtype, lengths=lens)
        st = enc.open_stream(B, 40 if W else L, window=W, bias=table)
        got = st.attention(qkv, lengths=lens)
        assert st.last_attn_kernel == STEP_BIASED
        cached = [0, 7, 60, 100]
        ext = st.attention_extend(qkv, lens, cached)
        assert st.last_attn_kernel == EXTEND_BIASED
        torch.cuda.synchronize()
        for b, n in enumerate(lens):
            err = (got[b].cpu().double() - O[b, n - 1]).abs()
            assert (err <= bound[b, n - 1]).all(), (kind, "step", n)
            worst = max(worst, float((err / bound[b, n - 1]).max()))
            err = (ext[b, cached[b]:n].cpu().double() - O[b, cached[b]:n]).abs()
            assert (err <= bound[b, cached[b]:n]).all(), (kind, "extend", n)
            worst = max(worst, float((err / bound[b, cached[b]:n]).max()))
            assert torch.equal(_bits(ext[b, n - 1]), _bits(got[b])), "the extend's last row is the step's"
        st.close()
    WORST[dtype] = max(WORST.get(dtype, 0.0), worst)
    print(f"{dtype} head_dim {hd} W {W}: worst |err| / bound {worst:.3f}; per dtype so far {({k: round(v, 3) for k, v in WORST.items()})}")
    enc.close()


# ---- 8. isolation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("cap,W", [(12, 0), (8, 5)])
def test_rows_a_track_does_not_hold_may_be_nan(shapes, dtype, cap, W):
    dims, sd, x, _ = shapes["toy"]
    H, o = dims[3], dims[2]
    enc = _encoder(dims, sd, dtype, 64)
    xg = torch.from_numpy(x).cuda()[:3, :12].contiguous()
    table = _table("rand_h", H, W or cap)
    clean, st = enc.open_stream(3, cap, window=W, bias=table), enc.open_stream(3, cap, window=W, bias=table)
    nan = torch.full((3, cap, dims[0]), float("nan"), device="cuda")
    assert torch.isnan(st.prefill(nan)).all()                                 # every cache row of every track holds NaN
    st.reset()

    def run(s):
        big = torch.full((64 + 3 * o + 64,), SENTINEL, device="cuda")
        out = [s.prefill(xg[:, :4].contiguous(), lengths=[4, 1, 2]).clone()]
        for t in range(4, 10):
            y = s.step(xg[:, t].contiguous(), out=big[64:64 + 3 * o].view(3, o))
            torch.cuda.synchronize()
            assert (big[:64] == SENTINEL).all() and (big[64 + 3 * o:] == SENTINEL).all()
            out.append(y.clone())
        big5 = torch.full((64 + 3 * 2 * o + 64,), SENTINEL, device="cuda")
        out.append(s.extend(xg[:, 10:12].contiguous(), out=big5[64:64 + 6 * o].view(3, 2, o)).clone())
        torch.cuda.synchronize()
        assert (big5[:64] == SENTINEL).all() and (big5[64 + 6 * o:] == SENTINEL).all()
        return out

    want, got = run(clean), run(st)
    for g, w in zip(got, want):
        assert torch.isfinite(g).all() and torch.equal(_bits(g), _bits(w)), "a cache row the track does not hold was read"
    clean.close(); st.close(); enc.close()


@pytest.mark.parametrize("dtype,fused", [("f32", 0), ("f32", 1), ("f16", 0)])
def test_other_calls_keep_their_bits_around_biased_streams(shapes, dtype, fused):
    dims, sd, x, lens = shapes["toy"]
    B, L, H = x.shape[0], x.shape[1], dims[3]
    enc = _encoder(dims, sd, dtype, B * L, fused=fused)
    xg = torch.from_numpy(x).cuda()
    band = MB.make_allowed("random", L).clone()
    band[torch.arange(L), torch.arange(L)] = True
    m, mb = enc.make_mask(~band), enc.make_bias(BB.make_bias("alibi", L, H))
    plain_st = enc.open_stream(B, L)

    def others():
        out = [enc(xg).clone(), enc(xg, is_causal=True).clone(), enc(xg, is_causal=True, window=4).clone(), enc(xg, mask=m).clone(), enc(xg, mask=mb).clone(),
               enc(xg, lengths=lens).clone()]
        fused_seen = enc.last_forward_fused
        plain_st.reset()
        out.append(plain_st.prefill(xg, lengths=[max(1, n - 1) for n in lens]).clone())
        out.append(plain_st.step(xg[:1, 3].contiguous(), [1]).clone())
        return out, fused_seen, enc.forward_plan(B, L)

    before = others()
    ta, tb = _table("alibi_h", H, L), _table("rand_1", H, L)
    for causal_before in (0, 1):
        enc.set_option("causal", causal_before)
        sa, sb = enc.open_stream(B, L, bias=ta), enc.open_stream(B, L, window=L, bias=tb)
        sa.prefill(xg, lengths=[max(1, n - 1) for n in lens])
        sb.extend(xg[:, :5].contiguous())
        sa.step(xg[:1, 3].contiguous(), [1])
        assert enc.set_option("causal", causal_before) == causal_before, "a biased stream call changed option causal"
        sa.close(); sb.close()
    enc.set_option("causal", 0)
    after = others()
    assert before[1:] == after[1:] and before[2] == ("fused" if fused else "launches")
    for i, (g, w) in enumerate(zip(after[0], before[0])):
        assert torch.equal(_bits(g), _bits(w)), f"call {i} changed its bits around biased stream calls"
    plain_st.close(); m.close(); mb.close(); enc.close()


def test_states_stepped_alternately(shapes):
    dims, sd, x, _ = shapes["toy"]
    H = dims[3]
    enc = _encoder(dims, sd, "f32", 64)
    xg = torch.from_numpy(x).cuda()
    xa, xb = xg[:2, :7].contiguous(), xg[2:5, :7].flip(1).contiguous()
    ta, tb = _table("alibi_h", H, 7), _table("rand_h", H, 9)
    for open_a, open_b in ((lambda: enc.open_stream(2, 7, bias=ta), lambda: enc.open_stream(3, 9)),           # biased and unbiased
                           (lambda: enc.open_stream(2, 7, bias=ta), lambda: enc.open_stream(3, 9, bias=tb))):  # two tables
        sa, sb = open_a(), open_b()
        ya, yb = [], []
        for t in range(7):
            ya.append(sa.step(xa[:, t].contiguous()))
            yb.append(sb.step(xb[:, t].contiguous()))
        ya, yb = torch.stack(ya, 1), torch.stack(yb, 1)
        s1, s2 = open_a(), open_b()
        assert torch.equal(_bits(ya), _bits(_walk(s1, xa))) and torch.equal(_bits(yb), _bits(_walk(s2, xb)))
        assert torch.equal(_bits(ya), _bits(_forward(enc, xa, ta)))
        assert torch.equal(_bits(yb), _bits(_forward(enc, xb, tb[:, :7]) if sb.bias_planes else enc(xb, is_causal=True)))
        for s in (sa, sb, s1, s2):
            s.close()
    enc.close()


# ---- 9. order is visible --------------------------------------------------------------------------------------------------------------
def test_order_is_visible(shapes):
    """the feature's purpose: swapping two poses of the history moves the last step's row under ALiBi, and only by rounding without"""
    from oracle import tf_encoder_ref as T
    dims = (16, 32, 9, 4, 1, 64)                                              # one layer: a deeper encoder sees the order through its own causal rows
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=11)
    enc = _encoder(dims, sd, "f32", 32)
    x = torch.randn(1, 15, dims[0], generator=torch.Generator().manual_seed(2)).cuda()
    sw = x.clone()
    sw[0, 2], sw[0, 9] = x[0, 9], x[0, 2]
    delta = {}
    for name, bias in (("unbiased", None), ("alibi", _table("alibi_h", dims[3], 15))):
        last = []
        for seq in (x, sw):
            st = enc.open_stream(1, 15, bias=bias)
            last.append(_walk(st, seq)[0, -1].clone())
            st.close()
        delta[name] = float((last[0] - last[1]).abs().max())
    print(f"|delta| of the last step's row after swapping poses 2 and 9: unbiased {delta['unbiased']:.3e}, per-head ALiBi {delta['alibi']:.3e}")
    assert delta["alibi"] > delta["unbiased"]
    enc.close()


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(shapes):
    dims, sd, x, _ = shapes["toy"]
    H = dims[3]
    enc = _encoder(dims, sd, "f32", 64)
    xg = torch.from_numpy(x).cuda()[:2, :6].contiguous()
    good = _table("rand_h", H, 6)
    want = _forward(enc, xg, good)

    def bad(value, plane, dist):
        t = good.clone()
        t[plane, dist] = value
        return t

    refused = [
        (lambda: enc.open_stream(2, 6, bias=bad(float("nan"), 2, 3)), r"table\[2\]\[3\] = .*nan.* is not finite"),
        (lambda: enc.open_stream(2, 6, bias=bad(float("inf"), 0, 5)), r"table\[0\]\[5\] = inf.* is not finite"),
        (lambda: enc.open_stream(2, 6, bias=bad(float("-inf"), 3, 0)), r"table\[3\]\[0\] = -inf.* is not finite"),
        (lambda: enc.open_stream(2, 6, bias=torch.zeros(2, 6)), r"planes = 2 is neither 1 nor num_heads = 4"),
        (lambda: enc.open_stream(2, 6, bias=torch.zeros(5, 6)), r"planes = 5 is neither 1 nor num_heads = 4"),
        (lambda: enc.open_stream(2, 6, bias=torch.zeros(H, 5)), r"distances = 5, but this state needs 6 \(its capacity\)"),
        (lambda: enc.open_stream(2, 6, window=4, bias=torch.zeros(H, 6)), r"distances = 6, but this state needs 4 \(its window\)"),
        (lambda: enc.open_stream(2, 6, window=4, bias=torch.zeros(5)), r"distances = 5, but this state needs 4"),
        (lambda: enc.open_stream(2, 6, bias=torch.zeros(H, 6, dtype=torch.int32)), r"bias must be a floating tensor"),
        (lambda: enc.open_stream(2, 6, bias=torch.zeros(1, H, 6)), r"bias must be a floating tensor"),
        (lambda: enc.open_stream(2, 6, bias=[0.0] * 6), r"bias must be a floating tensor"),
        (lambda: enc.open_stream(0, 6, bias=good), r"tracks must be positive"),
        (lambda: enc.open_stream(2, 6, window=7, bias=torch.zeros(H, 7)), r"window = 7 is outside 1 \.\. capacity = 6"),
    ]
    if torch.cuda.device_count() > 1:
        refused.append((lambda: enc.open_stream(2, 6, bias=good.to("cuda:1")), r"bias lives on cuda:1"))
    for call, msg in refused:
        with pytest.raises(ValueError, match=msg):
            call()
        st = enc.open_stream(2, 6, bias=good.cuda())                           # the next call's bits are right (a table on the handle's device is taken)
        assert torch.equal(_bits(_walk(st, xg)), _bits(want)), msg
        st.close()
    # the C entry points themselves: NULL arguments, and the planes of a state without a table
    import ctypes as C
    out = C.c_void_p()
    t = good.contiguous()
    ptr = C.cast(t.data_ptr(), C.POINTER(C.c_float))
    assert enc.lib.flope_tf_stream_open_bias(enc.handle, 2, 6, 0, H, 6, None, C.byref(out)) == -1 and not out.value
    assert b"NULL table" in enc.lib.flope_tf_last_error(enc.handle)
    assert enc.lib.flope_tf_stream_open_bias(enc.handle, 2, 6, 0, H, 6, ptr, None) == -1
    assert enc.lib.flope_tf_stream_open_bias(None, 2, 6, 0, H, 6, ptr, C.byref(out)) == -1 and not out.value
    assert enc.lib.flope_tf_stream_open_bias(enc.handle, 2, 6, -1, H, 6, ptr, C.byref(out)) == -1 and not out.value
    assert enc.lib.flope_tf_stream_bias_planes(None) == -1
    plain = enc.open_stream(2, 6)
    assert plain.bias_planes == 0 and enc.lib.flope_tf_stream_bias_planes(plain.state) == 0
    plain.close()
    # a closed state, and a state whose encoder is closed
    st = enc.open_stream(2, 6, bias=good)
    st.close()
    for call in (lambda: st.step(xg[:, 0].contiguous()), lambda: st.extend(xg), lambda: st.prefill(xg), lambda: st.step_plan, lambda: st.extend_plan()):
        with pytest.raises(RuntimeError, match="stream has been closed"):
            call()
    st2 = enc.open_stream(1, 2, bias=torch.zeros(2))
    enc.close()
    with pytest.raises(RuntimeError, match="encoder of this stream has been closed"):
        st2.step(xg[:1, 0].contiguous())
    st2.close()
