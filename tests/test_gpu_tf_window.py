"""Sliding-window causal attention and the ring cache of a windowed stream state on the device (forward(..., window=W),
enc.open_stream(tracks, capacity, window=W)).

The contract: a windowed forward runs tf_attn_generic's WINDOW instantiation for every dtype and shape, so a windowed step() at
absolute position t returns row t of enc(track[: t + 1], is_causal=True, window=W) IN BITS for every dtype, alone or behind a
prefill(), for any capacity >= W.  Against the fp64 restatement (tests/tf_attn_window_bound.py) the tolerances are DESIGN.md 24's:
2e-4 (f32, f32m), 1.5e-2 (f16), 1.2e-1 (bf16).  Shapes are the smallest at which the loops can go wrong:

  TOY   fixture dims, B 6, L 15, W 4, capacities 4 and 6: the ring wraps three times; capacity 6 wraps out of phase with W
  LONG  fixture dims, B 2, L 150, W 70, capacities 70 and 96: two trips of the 64-lane loop, unrolled trips plus singles in the value
        pass, the ring seam inside an unrolled group at some positions
  WIDE  (16, 128, 9, 2, 2, 256), B 3, L 50, W 8, capacities 8 and 11: head_dim 64, vector loads, a forward whose un-windowed pick is
        an MFMA kernel
  odd   head dims 6 and 12: element-wise loads

  1. the forward      2. steps      3. state      4. refusals
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tf_attn_window_bound as WB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f32m": torch.float32}
GENERIC = 0
SENTINEL = 1234.0
TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)
ODD = (5, 30, 3, 5, 1, 20)           # head_dim 6: element-wise loads in float32 and in 16 bits, and in tf_cache_append; one layer
MID = (5, 24, 3, 2, 1, 20)           # head_dim 12: three 16-byte vectors in float32, element-wise in 16 bits; one layer
MODES = [("f32", 2e-4), ("f32m", 2e-4), ("f16", 1.5e-2), ("bf16", 1.2e-1)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sd_t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _encoder(dims, sd, dtype, max_tokens, fused=0):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, fused=fused)
    enc.load_state_dict(_sd_t(sd))
    return enc


def _attn_kernel(enc, dims, dtype, B, L, window=0):
    """the attention kernel a causal forward of (B, L) launches on this handle"""
    enc.attention(torch.zeros(B, L, 3 * dims[1], dtype=TDT[dtype], device="cuda"), is_causal=True, window=window)
    return enc.last_attn_kernel


@pytest.fixture(scope="module")
def shapes():
    """name -> (dims, state dict, x [B, L, in], W, capacities, lengths, fp64 windowed restatement of x); computed once, never changed"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_window_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    wsd = T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)
    wx = np.random.default_rng(1).standard_normal((3, 50, 16)).astype(np.float32)
    lx = np.random.default_rng(2).standard_normal((2, 150, 16)).astype(np.float32)
    res = {"toy": (TOY, sd, f["x"], int(f["W"]), (4, 6), [15, 1, 7, 12, 3, 15]),
           "long": (TOY, sd, lx, 70, (70, 96), [150, 141]),
           "wide": (WIDE, wsd, wx, 8, (8, 11), [50, 1, 33])}
    out = {k: v + (WB.window_forward(v[1], v[2], v[3], num_heads=v[0][3]),) for k, v in res.items()}
    out["fixture_y"] = f["y_window"]
    return out


def _walk(st, x, tracks=None, start=0):
    """x [n, L, in] one column at a time from column `start` -> [n, L - start, out]"""
    return torch.stack([st.step(x[:, t].contiguous(), tracks) for t in range(start, x.shape[1])], dim=1)


# ---- 1. the forward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["toy", "wide"])
@pytest.mark.parametrize("dtype,tol", MODES, ids=lambda v: str(v))
def test_forward(shapes, shape, dtype, tol):
    dims, sd, x, W, _, lens, ref = shapes[shape]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L, fused=1)                    # "fused" is stored and ignored by every handle but f32's
    xg = torch.from_numpy(x).cuda()
    plain, causal = enc(xg).clone(), enc(xg, is_causal=True).clone()
    fused_plain = enc.last_forward_fused
    plan_causal = enc.forward_plan(B, L, is_causal=True)
    assert fused_plain == (plan_causal == "fused") and (dtype == "f32" or not fused_plain)
    if dtype == "f32" and shape == "toy":
        assert plan_causal == "fused", "the un-windowed forward of this shape is the single launch: the window must leave it"
    kernel_causal = _attn_kernel(enc, dims, dtype, B, L)
    assert (kernel_causal == GENERIC) == (dtype == "f32" or (shape == "toy" and dtype != "f32m")), kernel_causal

    y = enc(xg, is_causal=True, window=W).clone()
    assert not enc.last_forward_fused and enc.forward_plan(B, L, is_causal=True, window=W) == "launches"
    assert enc.forward_plan(B, L, lens, is_causal=True, window=W) == "launches"
    assert _attn_kernel(enc, dims, dtype, B, L, window=W) == GENERIC, "under a window every attention launch is the generic kernel"
    assert enc.set_option("window", W) == W, "the option reads back what the last call stated"
    err = float(np.abs(y.cpu().numpy() - ref).max())
    print(f"{dtype} {shape} W={W}: |y - fp64|max {err:.3e}, tolerance {tol}")
    assert torch.isfinite(y).all() and err < tol
    assert float((y - causal).abs().max()) > 1e-3, "the window changed nothing"
    if dtype == "f32" and shape == "toy":
        e = float(np.abs(y.cpu().numpy() - shapes["fixture_y"]).max())
        print(f"f32 toy vs the reference module under the banded mask: {e:.3e}")
        assert e < 1e-5
    # torch's spelling: the banded mask, float or bool, on the host or on the device
    for dt in (torch.float32, torch.bool):
        for dev in ("cpu", "cuda"):
            m = WB.band_mask(L, W, dt).to(dev)
            assert torch.equal(_bits(enc(xg, mask=m)), _bits(y)), (dt, dev)
            assert torch.equal(_bits(enc(xg, mask=m, is_causal=True, window=W)), _bits(y)), (dt, dev)
    # a window that holds the whole sequence is causal attention: the generic kernel's bits
    for big in (L, L + 5):
        yb = enc(xg, is_causal=True, window=big)
        if kernel_causal == GENERIC:
            assert torch.equal(_bits(yb), _bits(causal)), big
        else:
            assert float(np.abs(yb.cpu().numpy() - WB.window_forward(sd, x, 0, num_heads=dims[3])).max()) < tol
    # the prefix property
    for n in sorted({1, W, W + 1, L - 1}):
        assert torch.equal(_bits(enc(xg[:, :n].contiguous(), is_causal=True, window=W)), _bits(y[:, :n])), n
    # ragged: each sequence is itself alone, the window inside it; padded rows are never read
    xn = xg.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    yr = enc(xn, lengths=lens, is_causal=True, window=W)
    bias = torch.from_numpy(np.asarray(sd["out_layer.bias"], dtype=np.float32)).cuda()
    for b, n in enumerate(lens):
        assert torch.equal(_bits(yr[b, :n]), _bits(enc(xg[b:b + 1, :n].contiguous(), is_causal=True, window=W)[0])), b
        assert torch.equal(_bits(yr[b, :n]), _bits(y[b, :n])), b
        assert torch.equal(yr[b, n:], bias.expand(L - n, -1)), b
    # FLOP counts: attention over sum_t min(t + 1, W) keys per sequence
    i, d, o, H, nl, ff = dims
    lin = lambda M: M * i * d + M * d * o + nl * (M * d * 3 * d + M * d * d + 2 * M * d * ff)
    pairs = lambda n, w: sum(min(t + 1, w) for t in range(n))
    assert enc.flops(B, L, is_causal=True, window=W) == 2.0 * (lin(B * L) + nl * 2 * d * B * pairs(L, W))
    assert enc.flops(B, L, lengths=lens, is_causal=True, window=W) == 2.0 * (lin(sum(lens)) + nl * 2 * d * sum(pairs(n, W) for n in lens))
    assert enc.flops(B, L, is_causal=True, window=L) == enc.flops(B, L, is_causal=True) < enc.flops(B, L)
    # a plain call after a windowed one is un-windowed
    enc(xg, is_causal=True, window=W)
    assert torch.equal(_bits(enc(xg)), _bits(plain)) and enc.last_forward_fused == fused_plain
    assert enc.set_option("window", 0) == 0
    enc(xg, is_causal=True, window=W)
    assert torch.equal(_bits(enc(xg, is_causal=True)), _bits(causal)) and enc.forward_plan(B, L, is_causal=True) == plan_causal
    assert enc.set_option("window", 0) == 0 and enc.set_option("causal", 0) == 1
    enc.close()


# ---- 2. steps -------------------------------------------------------------------------------------------------------------------------
STEP_CASES = [(s, d) for s in ("toy", "wide") for d, _ in MODES] + [("long", "f32"), ("long", "f16")]


@pytest.mark.parametrize("shape,dtype", STEP_CASES, ids=lambda v: str(v))
def test_steps(shapes, shape, dtype):
    dims, sd, x, W, caps, lens, ref = shapes[shape]
    tol = dict(MODES)[dtype]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L)
    xg = torch.from_numpy(x).cuda()
    want = enc(xg, is_causal=True, window=W).clone()
    err = float(np.abs(want.cpu().numpy() - ref).max())
    print(f"{dtype} {shape} W={W}: the windowed forward |y - fp64|max {err:.3e}, tolerance {tol}")
    assert err < tol
    walked = []
    for cap in caps:                                                   # every token through a windowed state, far past its capacity
        st = enc.open_stream(B, cap, window=W)
        assert (st.window, st.capacity) == (W, cap)
        got = _walk(st, xg)
        torch.cuda.synchronize()
        assert st.positions == [L] * B, "positions are absolute"
        diff = int((_bits(got) != _bits(want)).sum())
        first = int((_bits(got) != _bits(want)).any(dim=2).any(dim=0).nonzero()[0]) if diff else -1
        assert diff == 0, f"capacity {cap}: {diff} elements differ in bits from the windowed forward, first at position {first}"
        walked.append(got)
        st.close()
    assert torch.equal(_bits(walked[0]), _bits(walked[1])), "two capacities, two answers"
    # while t < W the rows are those of a state without a window, wherever DESIGN.md 25 has bits: the un-windowed forward is generic
    if _attn_kernel(enc, dims, dtype, B, L) == GENERIC:
        un = enc.open_stream(B, W)
        assert torch.equal(_bits(_walk(un, xg[:, :W].contiguous())), _bits(walked[0][:, :W]))
        un.close()
    # behind a ragged prefill of half of each track: its output is the ragged windowed forward, the steps continue the tracks
    cap = caps[1]
    st = enc.open_stream(B, cap, window=W)
    half = [max(1, n // 2) for n in lens]
    enc(xg[:1, :1].contiguous())                                       # states causal = 0, window = 0
    pre = st.prefill(xg, lengths=half)
    assert enc.set_option("window", 0) == 0 and enc.set_option("causal", 0) == 0, "prefill left an option changed"
    assert torch.equal(_bits(pre), _bits(enc(xg, lengths=half, is_causal=True, window=W)))
    assert st.positions == half
    for t in range(min(half), L):
        rows = [b for b in range(B) if half[b] <= t < lens[b]]
        if rows:
            y = st.step(torch.stack([xg[b, t] for b in rows]), rows)
            assert torch.equal(_bits(y), _bits(torch.stack([want[b, t] for b in rows]))), f"step {t} behind the prefill"
    assert st.positions == lens
    # a prefill longer than the capacity (the ring keeps its last tokens), then steps
    n0 = L - max(3, W // 2)
    assert n0 > caps[0]
    st2 = enc.open_stream(B, caps[0], window=W)
    pre = st2.prefill(xg[:, :n0].contiguous())
    assert torch.equal(_bits(pre), _bits(want[:, :n0])) and st2.positions == [n0] * B
    assert torch.equal(_bits(_walk(st2, xg, start=n0)), _bits(want[:, n0:]))
    st.close(); st2.close(); enc.close()


@pytest.mark.parametrize("dims", [ODD, MID], ids=["hd6", "hd12"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_head_dims_without_whole_vectors(dims, dtype):
    from oracle import tf_encoder_ref as T
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=7)
    B, L, W = 3, 23, 5
    enc = _encoder(dims, sd, dtype, B * L)
    xg = torch.randn(B, L, dims[0], generator=torch.Generator().manual_seed(4)).cuda()
    want = enc(xg, is_causal=True, window=W).clone()
    ref = WB.window_forward(sd, xg.cpu().numpy(), W, num_heads=dims[3])
    assert float(np.abs(want.cpu().numpy() - ref).max()) < dict(MODES)[dtype]
    for cap in (5, 7):
        st = enc.open_stream(B, cap, window=W)
        assert torch.equal(_bits(_walk(st, xg)), _bits(want)), cap
        st.reset()
        lens = [L - 1, 1, 10]
        pre = st.prefill(xg, lengths=lens)
        assert torch.equal(_bits(pre), _bits(enc(xg, lengths=lens, is_causal=True, window=W)))
        for b, n in enumerate(lens):
            assert torch.equal(_bits(st.step(xg[b:b + 1, n].contiguous(), [b])[0]), _bits(want[b, n])), f"track {b} behind a prefill of {n}"
        st.close()
    enc.close()


# ---- 3. state -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_subsets_of_tracks_equal_the_tracks_alone(shapes, dtype):
    dims, sd, x, W, caps, lens, _ = shapes["toy"]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L)
    xg = torch.from_numpy(x).cuda()
    want = enc(xg, is_causal=True, window=W).clone()
    st = enc.open_stream(B, caps[1], window=W)
    groups = [[2, 0, 5], [4, 1, 3]]
    held = [0] * B
    for t in range(L):                                                 # group 0 runs two tokens ahead of group 1
        for g, lag in zip(groups, (0, 2)):
            if 0 <= t - lag:
                y = st.step(xg[g, t - lag].contiguous(), g)
                assert torch.equal(_bits(y), _bits(want[g, t - lag])), (t, g)
                for b in g:
                    held[b] += 1
        assert st.positions == held
    st.close(); enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_nan_is_forgotten_by_reset_and_by_the_window(shapes, dtype):
    """A row of the ring that holds NaN is never read again once it is outside the window: 0 * NaN would show.  Without a reset the
    output at position t depends on the tokens t - num_layers (W - 1) .. t (each layer looks W - 1 tokens back), so with one layer W
    clean tokens behind the NaN ones give a finite row, with two layers 2 (W - 1) + 1 -- and that row is, in bits, the last row of the
    windowed forward of the clean tokens alone (every window of it is full, so the summation order is the same)."""
    from oracle import tf_encoder_ref as T
    dims, sd, x, W, caps, _, _ = shapes["toy"]
    xg = torch.from_numpy(x).cuda()[:2].contiguous()
    for dm, s, xs, w, cap in ((TOY, sd, xg, W, caps[1]), (ODD, T.synthetic_state_dict(ODD[0], ODD[1], ODD[2], ODD[4], ODD[5], seed=7),
                                                           torch.randn(2, 15, ODD[0], generator=torch.Generator().manual_seed(8)).cuda(), 5, 5)):
        enc = _encoder(dm, s, dtype, 64)
        nl = dm[4]
        need = nl * (w - 1) + 1
        want = enc(xs, is_causal=True, window=w).clone()
        st = enc.open_stream(2, cap, window=w)
        nan = torch.full((1, dm[0]), float("nan"), device="cuda")
        for _ in range(2 * cap + 1):                                   # every ring row of track 1 holds NaN
            y = st.step(nan, [1])
        assert torch.isnan(y).all() and st.positions == [0, 2 * cap + 1]
        got = []
        for t in range(need):                                          # no reset: clean tokens behind the NaN ones
            got.append(st.step(xs[1:2, t].contiguous(), [1]))
        assert torch.isnan(got[need - 2]).any(), "the receptive field is num_layers (W - 1) + 1 tokens"
        assert torch.isfinite(got[need - 1]).all(), "a stale row was read"
        assert torch.equal(_bits(got[need - 1][0]), _bits(want[1, need - 1])), (dm, "the window has forgotten the NaN tokens")
        nxt = st.step(xs[1:2, need].contiguous(), [1])
        assert torch.equal(_bits(nxt[0]), _bits(enc(xs[1:2, 1:need + 1].contiguous(), is_causal=True, window=w)[0, -1]))
        assert st.positions == [0, 2 * cap + 1 + need + 1]
        st.reset([1])                                                  # a reset forgets everything at once
        assert st.positions == [0, 0]
        assert torch.equal(_bits(_walk(st, xs)), _bits(want))
        st.close(); enc.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_sentinels_around_y(shapes, dtype):
    dims, sd, x, W, caps, lens, _ = shapes["toy"]
    B, L, o = x.shape[0], x.shape[1], dims[2]
    enc = _encoder(dims, sd, dtype, B * L)
    xg = torch.from_numpy(x).cuda()
    st = enc.open_stream(B, caps[0], window=W)
    big = torch.full((64 + B * L * o + 64,), SENTINEL, device="cuda")
    y = st.prefill(xg, lengths=lens, out=big[64:64 + B * L * o].view(B, L, o))
    torch.cuda.synchronize()
    assert (big[:64] == SENTINEL).all() and (big[64 + B * L * o:] == SENTINEL).all() and torch.isfinite(y).all()
    assert torch.equal(_bits(y), _bits(enc(xg, lengths=lens, is_causal=True, window=W)))
    rows = [3, 0, 5]                                                   # positions 12, 15, 15: past the capacity
    for t in range(3):
        big.fill_(SENTINEL)
        y = st.step(xg[rows, t].contiguous(), rows, out=big[64:64 + 3 * o].view(3, o))
        torch.cuda.synchronize()
        assert (big[:64] == SENTINEL).all() and (big[64 + 3 * o:] == SENTINEL).all() and torch.isfinite(y).all()
    st.close(); enc.close()


def test_an_unwindowed_state_on_the_same_handle_is_undisturbed(shapes):
    dims, sd, x, W, caps, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, "f32", 64)
    xg = torch.from_numpy(x).cuda()
    xa, xb = xg[:2, :9].contiguous(), xg[2:5, :9].flip(1).contiguous()
    want_a, want_b = enc(xa, is_causal=True).clone(), enc(xb, is_causal=True, window=W).clone()
    sa, sb = enc.open_stream(2, 9), enc.open_stream(3, caps[0], window=W)
    assert (sa.window, sb.window) == (0, W)
    ya, yb = [], []
    for t in range(9):
        ya.append(sa.step(xa[:, t].contiguous()))
        yb.append(sb.step(xb[:, t].contiguous()))
        if t == 4:
            enc(xa, is_causal=True, window=2)                          # and a windowed forward between the steps
    assert torch.equal(_bits(torch.stack(ya, 1)), _bits(want_a)) and torch.equal(_bits(torch.stack(yb, 1)), _bits(want_b))
    with pytest.raises(ValueError, match="already holds capacity = 9"):
        sa.step(xa[:, 0].contiguous())                                 # the linear state is still full at its capacity
    sb.step(xb[:, 0].contiguous())                                     # the ring never is
    # an un-windowed prefill on a handle whose last call stated a window is still the plain causal forward
    enc(xa, is_causal=True, window=2)
    sa.reset()
    assert torch.equal(_bits(sa.prefill(xa)), _bits(want_a)) and enc.set_option("window", 0) == 2
    sa.close(); sb.close(); enc.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(shapes):
    from flope_amd import _lib
    dims, sd, x, W, caps, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, "f32", 128)
    xg = torch.from_numpy(x).cuda()
    L = xg.shape[1]
    want = enc(xg[:3], is_causal=True, window=W).clone()
    st = enc.open_stream(3, 6, window=W)
    for t in range(3):
        st.step(xg[:3, t].contiguous())
    held = [3, 3, 3]
    two = WB.band_mask(L, 2, torch.bool)
    two[8:] = WB.band_mask(L, 3, torch.bool)[8:]
    refused = [
        (lambda: enc.open_stream(3, 6, window=7), r"window = 7 is outside 1 \.\. capacity = 6"),
        (lambda: enc.open_stream(3, 6, window=-1), r"window must be 0 \(a linear cache\) or 1 \.\. capacity"),
        (lambda: enc.open_stream(3, 4097, window=5), r"capacity 1 \.\. 4096"),
        (lambda: enc.open_stream(0, 6, window=2), r"tracks must be positive"),
        (lambda: enc(xg, window=W), r"window=4 needs is_causal=True"),
        (lambda: enc(xg, mask=torch.zeros(L, L), window=W), r"window=4 needs is_causal=True"),
        (lambda: enc(xg, is_causal=True, window=-2), r"window must be 0 \(none\) or a positive"),
        (lambda: enc.attention(torch.zeros(1, 4, 96, device="cuda"), window=2), r"window=2 needs is_causal=True"),
        (lambda: enc.flops(2, 5, window=2), r"window=2 needs is_causal=True"),
        (lambda: enc.forward_plan(2, 5, window=2), r"window=2 needs is_causal=True"),
        (lambda: enc(xg, mask=WB.band_mask(L, 3), window=W), r"window=4 with a banded mask of window 3"),
        (lambda: enc(xg, mask=WB.band_mask(L, 3).cuda(), is_causal=True, window=5), r"window=5 with a banded mask of window 3"),
        (lambda: enc(xg, mask=two), r"mask\[8, 6\].*window 2"),
        (lambda: enc(xg, mask=WB.band_mask(L, 3).t().contiguous()), r"mask\[0, 1\]"),
        (lambda: enc(xg, mask=WB.band_mask(L + 1, 3)), "mask must be"),
        (lambda: enc(xg, mask=torch.zeros(L, L), is_causal=True), "is_causal=True with a mask"),
        (lambda: st.step(xg[:2, 3].contiguous(), [1, 1]), r"tracks\[1\] = 1 names a track"),
        (lambda: st.step(xg[:2, 3].contiguous(), [1, 3]), r"tracks\[1\] = 3 is outside 0 \.\. 2"),
        (lambda: st.prefill(xg[:2, :9].contiguous(), tracks=[2, 2]), r"tracks\[1\] = 2 names a track"),
        (lambda: st.prefill(xg[:2, :9].contiguous(), lengths=[9, 0], tracks=[1, 2]), r"lengths\[1\] = 0 is outside"),
    ]
    for call, msg in refused:
        with pytest.raises(ValueError, match=msg):
            call()
        assert st.positions == held, msg
    # the C entry points refuse the pair (window > 0, causal = 0) themselves
    assert enc.set_option("window", -1) == _lib.EINVAL and "window is 0" in enc.lib.flope_tf_last_error(enc.handle).decode()
    enc.set_option("causal", 0)
    assert enc.set_option("window", 3) >= 0
    y = torch.full((3, L, dims[2]), SENTINEL, device="cuda")
    x3 = xg[:3].contiguous()
    assert enc.lib.flope_tf_forward(enc.handle, x3.data_ptr(), 3, L, y.data_ptr(), None) == _lib.EINVAL
    assert "window = 3 needs option causal = 1" in enc.lib.flope_tf_last_error(enc.handle).decode()
    lh = (C.c_int * 3)(L, 2, 5)
    assert enc.lib.flope_tf_forward_varlen(enc.handle, x3.data_ptr(), 3, L, lh, y.data_ptr(), None) == _lib.EINVAL
    assert enc.lib.flope_tf_forward_plan(enc.handle, 3, L, None) == _lib.EINVAL and enc.lib.flope_tf_forward_plan(enc.handle, 3, L, lh) == _lib.EINVAL
    q = torch.zeros(3, L, 3 * dims[1], device="cuda")
    a = torch.full((3, L, dims[1]), SENTINEL, device="cuda")
    assert enc.lib.flope_tf_attention(enc.handle, q.data_ptr(), 3, L, a.data_ptr(), None) == _lib.EINVAL
    assert enc.lib.flope_tf_attention_varlen(enc.handle, q.data_ptr(), 3, lh, a.data_ptr(), None) == _lib.EINVAL
    torch.cuda.synchronize()
    assert (y == SENTINEL).all() and (a == SENTINEL).all(), "a refused call wrote"
    assert enc.set_option("window", 0) == 3
    assert st.positions == held
    # the next valid calls return the right bits
    assert torch.equal(_bits(st.step(x3[:, 3].contiguous())), _bits(want[:, 3]))
    assert torch.equal(_bits(enc(x3, mask=WB.band_mask(L, W, torch.bool))), _bits(want))
    # a stream outlives neither its close() nor its encoder's
    st.close()
    with pytest.raises(RuntimeError, match="stream has been closed"):
        st.step(x3[:, 0].contiguous())
    st2 = enc.open_stream(1, 2, window=2)
    enc.close()
    for call in (lambda: st2.step(xg[:1, 0].contiguous()), lambda: st2.prefill(xg[:1, :2].contiguous()), lambda: st2.reset(), lambda: st2.position(0)):
        with pytest.raises(RuntimeError, match="encoder of this stream has been closed"):
            call()
    with pytest.raises(RuntimeError, match="encoder of this stream has been closed"):
        enc.open_stream(1, 2, window=2)
    st2.close()
