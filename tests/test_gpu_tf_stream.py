"""The streaming causal forward of the encoder on the device (enc.open_stream, flope_tf_stream_*).

The contract: where the forward's attention kernel for a shape is the generic one (read from enc.attention's last_attn_kernel, not
guessed), step()'s row for the token at position t of a track is row t of enc(track, is_causal=True) IN BITS, alone or after a
prefill(), and prefill()'s own output is the bits of enc(x, lengths=.., is_causal=True).  Elsewhere (tf_attn_f32m, tf_attn_mfma,
tf_attn_tiled) the linears are the forward's but the attention order is not, and the rows are held to DESIGN.md 24's tolerances
against the fp64 causal restatement: 2e-4 f32m, 1.5e-2 f16, 1.2e-1 bf16.

  1. all steps, every mode on two shapes          5. capacity and refusals
  2. a long walk (three trips of the key loop)    6. a sentinel around y
  3. ragged prefill, permuted tracks              7. nothing else of the handle moves (option fused included)
  4. reset over a cache full of NaN               8. two states on one handle
  9. head dims that take the element-wise loads
"""
import os

import numpy as np
import pytest
import torch

import tf_attn_causal_bound as CB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f32m": torch.float32}
GENERIC = 0
SENTINEL = 1234.0
TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)
ODD = (5, 30, 3, 5, 1, 20)           # head_dim 6: element-wise loads in float32 and in 16 bits, and in tf_cache_append
MID = (5, 24, 3, 2, 1, 20)           # head_dim 12: three 16-byte vectors in float32, element-wise in 16 bits
MODES = [("f32", 0, 2e-4), ("f32m", 0, 2e-4), ("f16", 0, 1.5e-2), ("f16", 1, 1.5e-2), ("bf16", 0, 1.2e-1), ("bf16", 1, 1.2e-1)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sd_t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _encoder(dims, sd, dtype, max_tokens, tiled=0, fused=0):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, attn_tiled=tiled, fused=fused)
    enc.load_state_dict(_sd_t(sd))
    return enc


def _attn_kernel(enc, dims, dtype, B, L):
    """the attention kernel a forward of (B, L) launches on this handle"""
    enc.attention(torch.zeros(B, L, 3 * dims[1], dtype=TDT[dtype], device="cuda"), is_causal=True)
    return enc.last_attn_kernel


@pytest.fixture(scope="module")
def shapes():
    """name -> (dims, state dict, x [B, L, in], lengths, fp64 causal restatement of x)"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_causal_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    wsd = T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)
    wx = np.random.default_rng(1).standard_normal((3, 50, 16)).astype(np.float32)
    res = {"toy": (TOY, sd, f["x"], [int(v) for v in f["lengths"]]), "wide": (WIDE, wsd, wx, [50, 1, 33])}
    return {k: v + (CB.causal_forward(v[1], v[2], v[0][3]),) for k, v in res.items()}


def _walk(st, x, tracks=None):
    """x [n, L, in] one column at a time -> [n, L, out]"""
    return torch.stack([st.step(x[:, t].contiguous(), tracks) for t in range(x.shape[1])], dim=1)


# ---- 1. all steps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "toy"])
@pytest.mark.parametrize("dtype,tiled,tol", MODES, ids=lambda v: str(v))
def test_all_steps(shapes, shape, dtype, tiled, tol):
    dims, sd, x, lens, full = shapes[shape]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L, tiled)
    xg = torch.from_numpy(x).cuda()
    kernel = _attn_kernel(enc, dims, dtype, B, L)
    assert (kernel == GENERIC) == (dtype == "f32" or (shape == "toy" and dtype != "f32m")), kernel
    want = enc(xg, is_causal=True).clone()
    st = enc.open_stream(B, L)
    got = _walk(st, xg)
    torch.cuda.synchronize()
    assert st.positions == [L] * B
    assert torch.isfinite(got).all()
    err = float(np.abs(got.cpu().numpy() - full).max())
    ferr = float(np.abs(want.cpu().numpy() - full).max())
    print(f"{dtype} attn_tiled={tiled} {shape} (attention kernel {kernel}): steps |y - fp64|max {err:.3e}, the forward's {ferr:.3e}, tolerance {tol}")
    if kernel == GENERIC:
        diff = int((_bits(got) != _bits(want)).sum())
        assert diff == 0, f"{diff} elements of the stepped rows differ in bits from the causal forward"
    assert err < tol
    # ... and behind a prefill: its own output is the ragged causal forward's, the rows after it continue the tracks
    st.reset()
    half = [max(1, n // 2) for n in lens]
    pre = st.prefill(xg, lengths=half)
    assert torch.equal(_bits(pre), _bits(enc(xg, lengths=half, is_causal=True)))
    assert st.positions == half
    worst = 0.0
    for t in range(min(half), L):
        rows = [b for b in range(B) if half[b] <= t < lens[b]]
        if not rows:
            continue
        y = st.step(torch.stack([xg[b, t] for b in rows]), rows)
        worst = max(worst, float(np.abs(y.cpu().numpy() - np.stack([full[b, t] for b in rows])).max()))
        if kernel == GENERIC:
            assert torch.equal(_bits(y), _bits(torch.stack([want[b, t] for b in rows]))), f"step {t} behind the prefill"
    assert st.positions == lens
    print(f"{dtype} attn_tiled={tiled} {shape}: steps behind a prefill |y - fp64|max {worst:.3e}")
    assert worst < tol
    st.close()
    enc.close()


# ---- 2. a long walk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_long_walk(shapes, dtype):
    dims, sd = shapes["toy"][:2]
    n, L = 2, 130
    enc = _encoder(dims, sd, dtype, n * L)
    xg = torch.randn(n, L, dims[0], generator=torch.Generator().manual_seed(3)).cuda()
    assert _attn_kernel(enc, dims, dtype, n, L) == GENERIC
    want = enc(xg, is_causal=True).clone()
    a = enc.open_stream(n, L)
    pre = a.prefill(xg[:, :L - 1].contiguous())
    last_a = a.step(xg[:, L - 1].contiguous()).clone()
    b = enc.open_stream(n, L)
    walked = _walk(b, xg)
    torch.cuda.synchronize()
    assert torch.equal(_bits(pre), _bits(want[:, :L - 1]))
    assert torch.equal(_bits(walked), _bits(want))
    assert torch.equal(_bits(last_a), _bits(want[:, L - 1])) and torch.equal(_bits(last_a), _bits(walked[:, L - 1]))
    assert a.positions == [L, L] and b.positions == [L, L]
    a.close(); b.close(); enc.close()


# ---- 3. ragged and permuted -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ragged_prefill_then_permuted_steps(shapes, dtype):
    dims, sd, x, lens, _ = shapes["toy"]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L)
    assert _attn_kernel(enc, dims, dtype, B, L) == GENERIC
    xg = torch.from_numpy(x).cuda()
    new = torch.randn(B, 2, dims[0], generator=torch.Generator().manual_seed(9)).cuda()

    def alone(b, k):
        """track b in a fresh stream, token by token, then its first k new tokens: the last row"""
        s1 = enc.open_stream(1, L + 2)
        for t in range(lens[b]):
            s1.step(xg[b:b + 1, t].contiguous())
        for j in range(k):
            y = s1.step(new[b:b + 1, j].contiguous())
        s1.close()
        return y[0].clone()

    st = enc.open_stream(B, L + 2)
    st.prefill(xg, lengths=lens)
    assert st.positions == lens
    order = [2, 0, 5]
    y = st.step(new[order, 0].contiguous(), order)
    for r, b in enumerate(order):
        assert torch.equal(_bits(y[r]), _bits(alone(b, 1))), f"row {r} (track {b})"
    assert st.positions == [n + (b in order) for b, n in enumerate(lens)]
    rest = [4, 1, 3]                                                   # the untouched tracks: their next step is unaffected
    y = st.step(new[rest, 0].contiguous(), rest)
    for r, b in enumerate(rest):
        assert torch.equal(_bits(y[r]), _bits(alone(b, 1))), f"row {r} (track {b})"
    y = st.step(new[:, 1].contiguous())                                # every track, second new token
    for b in range(B):
        assert torch.equal(_bits(y[b]), _bits(alone(b, 2))), f"track {b}"
    assert st.positions == [n + 2 for n in lens]
    st.close(); enc.close()


# ---- 4. reset -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_reset_over_a_cache_of_nan(shapes, dtype):
    dims, sd, x, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, dtype, 64)
    xg = torch.from_numpy(x).cuda()[:2, :6].contiguous()
    clean = enc.open_stream(2, 8)
    want = _walk(clean, xg)
    st = enc.open_stream(2, 8)
    for _ in range(8):                                                 # every cache row of track 1 holds NaN
        y = st.step(torch.full((1, dims[0]), float("nan"), device="cuda"), [1])
    assert torch.isnan(y).all() and st.positions == [0, 8]
    st.reset([1])
    assert st.positions == [0, 0]
    got = _walk(st, xg)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), "a stale cache row was read"
    st.reset()
    assert st.positions == [0, 0]
    assert torch.equal(_bits(_walk(st, xg)), _bits(want))
    clean.close(); st.close(); enc.close()


# ---- 5. capacity and refusals ---------------------------------------------------------------------------------------------------------
def test_capacity_and_refusals(shapes):
    dims, sd, x, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, "f32", 64)
    xg = torch.from_numpy(x).cuda()
    want = enc(xg[:3, :4].contiguous(), is_causal=True)
    st = enc.open_stream(3, 3)
    for t in range(3):
        st.step(xg[:3, t].contiguous())
    st.reset([1, 2])
    st.step(xg[1:3, 0].contiguous(), [1, 2])
    held = [3, 1, 1]
    assert st.positions == held
    refused = [
        (lambda: st.step(xg[:3, 3].contiguous()), r"row 0: track 0 already holds capacity = 3"),
        (lambda: st.step(xg[:2, 3].contiguous(), [1, 0]), r"row 1: track 0 already holds"),
        (lambda: st.step(xg[:2, 1].contiguous(), [1, 1]), r"tracks\[1\] = 1 names a track"),
        (lambda: st.step(xg[:2, 1].contiguous(), [1, 3]), r"tracks\[1\] = 3 is outside 0 \.\. 2"),
        (lambda: st.step(xg[:2, 1].contiguous(), [-1, 2]), r"tracks\[0\] = -1 is outside"),
        (lambda: st.step(xg[:0, 1].contiguous(), []), r"n = 0 is outside"),
        (lambda: st.step(xg[:4, 1].contiguous(), [0, 1, 2, 1]), r"n = 4 is outside"),
        (lambda: st.step(xg[:2, 1].contiguous()), r"n = 2 is outside .* tracks_host is NULL"),
        (lambda: st.step(xg[:2, 1].contiguous(), [1]), r"tracks has 1 values for 2 rows"),
        (lambda: st.step(xg[:2, 1, :5].contiguous(), [1, 2]), r"expected \[n, 16\]"),
        (lambda: st.step(xg[:2, :2].contiguous(), [1, 2]), r"expected \[n, 16\]"),
        (lambda: st.prefill(xg[:2, :4].contiguous(), tracks=[1, 2]), r"lengths\[0\] = 4 exceeds capacity = 3"),
        (lambda: st.prefill(xg[:2, :4].contiguous(), lengths=[3, 4], tracks=[1, 2]), r"lengths\[1\] = 4 exceeds capacity = 3"),
        (lambda: st.prefill(xg[:2, :3].contiguous(), lengths=[3, 0], tracks=[1, 2]), r"lengths\[1\] = 0 is outside"),
        (lambda: st.prefill(xg[:2, :3].contiguous(), tracks=[2, 2]), r"tracks\[1\] = 2 names a track"),
        (lambda: st.reset([3]), r"tracks\[0\] = 3 is outside"),
        (lambda: st.position(3), r"track 3 is outside"),
        (lambda: enc.open_stream(0, 4), r"tracks must be positive"),
        (lambda: enc.open_stream(2, 4097), r"capacity 1 \.\. 4096"),
    ]
    for call, msg in refused:
        with pytest.raises(ValueError, match=msg):
            call()
        assert st.positions == held, msg
    with pytest.raises(RuntimeError, match="must live on"):
        st.step(xg[:2, 1].cpu(), [1, 2])
    assert st.positions == held
    y = st.step(xg[1:3, 1].contiguous(), [1, 2])                       # the next valid step returns the right bits
    assert torch.equal(_bits(y), _bits(want[1:3, 1])) and st.positions == [3, 2, 2]
    # a stream outlives neither its close() nor its encoder's
    st.close()
    with pytest.raises(RuntimeError, match="stream has been closed"):
        st.step(xg[:3, 0].contiguous())
    st2 = enc.open_stream(1, 2)
    enc.close()
    for call in (lambda: st2.step(xg[:1, 0].contiguous()), lambda: st2.prefill(xg[:1, :2].contiguous()), lambda: st2.reset(), lambda: st2.position(0)):
        with pytest.raises(RuntimeError, match="encoder of this stream has been closed"):
            call()
    st2.close()


# ---- 6. sentinel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_sentinels_around_y(shapes, dtype):
    dims, sd, x, lens, _ = shapes["toy"]
    B, L, o = x.shape[0], x.shape[1], dims[2]
    enc = _encoder(dims, sd, dtype, B * L)
    xg = torch.from_numpy(x).cuda()
    st = enc.open_stream(B, L)
    big = torch.full((64 + B * L * o + 64,), SENTINEL, device="cuda")
    y = st.prefill(xg, lengths=lens, out=big[64:64 + B * L * o].view(B, L, o))
    torch.cuda.synchronize()
    assert (big[:64] == SENTINEL).all() and (big[64 + B * L * o:] == SENTINEL).all() and torch.isfinite(y).all()
    assert torch.equal(_bits(y), _bits(enc(xg, lengths=lens, is_causal=True)))
    st.reset()
    big.fill_(SENTINEL)
    rows = [3, 1, 4]
    y = st.step(xg[rows, 0].contiguous(), rows, out=big[64:64 + 3 * o].view(3, o))
    torch.cuda.synchronize()
    assert (big[:64] == SENTINEL).all() and (big[64 + 3 * o:] == SENTINEL).all() and torch.isfinite(y).all()
    st.close(); enc.close()


# ---- 7. nothing else moves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,fused", [("f32", 0), ("f32", 1), ("f16", 0)])
def test_forwards_around_a_stream_keep_their_bits(shapes, dtype, fused):
    dims, sd, x, lens, _ = shapes["toy"]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L, fused=fused)
    xg = torch.from_numpy(x).cuda()
    plain, causal = enc(xg).clone(), enc(xg, is_causal=True).clone()
    assert enc.last_forward_fused == bool(fused)
    plan = enc.forward_plan(B, L)
    st = enc.open_stream(B, L)
    for causal_before in (0, 1):
        enc.set_option("causal", causal_before)
        st.reset()
        y = st.prefill(xg, lengths=[max(1, n - 1) for n in lens])
        assert enc.set_option("causal", causal_before) == causal_before, "prefill left option causal changed"
        for t in range(3):
            st.step(xg[:1, t].contiguous(), [1])
        assert enc.set_option("causal", causal_before) == causal_before, "step changed option causal"
        assert enc.last_forward_fused == bool(fused)
        assert torch.equal(_bits(y[0, :lens[0] - 1]), _bits(causal[0, :lens[0] - 1]))      # (under fused = 1: the launch sequence gave the single launch's bits)
    enc.set_option("causal", 0)
    assert enc.forward_plan(B, L) == plan == ("fused" if fused else "launches")
    assert torch.equal(_bits(enc(xg)), _bits(plain)) and enc.last_forward_fused == bool(fused)
    assert torch.equal(_bits(enc(xg, is_causal=True)), _bits(causal)) and enc.last_forward_fused == bool(fused)
    st.close(); enc.close()


# ---- 8. two states on one handle ------------------------------------------------------------------------------------------------------
def test_two_states_stepped_alternately(shapes):
    dims, sd, x, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, "f32", 64)
    xg = torch.from_numpy(x).cuda()
    xa, xb = xg[:2, :7].contiguous(), xg[2:5, :7].flip(1).contiguous()
    sa, sb = enc.open_stream(2, 7), enc.open_stream(3, 9)
    ya, yb = [], []
    for t in range(7):
        ya.append(sa.step(xa[:, t].contiguous()))
        yb.append(sb.step(xb[:, t].contiguous()))
    ya, yb = torch.stack(ya, 1), torch.stack(yb, 1)
    s1, s2 = enc.open_stream(2, 7), enc.open_stream(3, 9)
    assert torch.equal(_bits(ya), _bits(_walk(s1, xa))) and torch.equal(_bits(yb), _bits(_walk(s2, xb)))
    assert torch.equal(_bits(ya), _bits(enc(xa, is_causal=True)))
    for s in (sa, sb, s1, s2):
        s.close()
    enc.close()


# ---- 9. the element-wise loads --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [ODD, MID], ids=["hd6", "hd12"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_head_dims_without_whole_vectors(dims, dtype):
    from oracle import tf_encoder_ref as T
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=7)
    B, L = 3, 21
    enc = _encoder(dims, sd, dtype, B * L)
    assert _attn_kernel(enc, dims, dtype, B, L) == GENERIC
    xg = torch.randn(B, L, dims[0], generator=torch.Generator().manual_seed(4)).cuda()
    want = enc(xg, is_causal=True).clone()
    st = enc.open_stream(B, L)
    lens = [L - 1, 1, 10]
    pre = st.prefill(xg, lengths=lens)
    assert torch.equal(_bits(pre), _bits(enc(xg, lengths=lens, is_causal=True)))
    for b, n in enumerate(lens):
        y = st.step(xg[b:b + 1, n].contiguous(), [b])
        assert torch.equal(_bits(y[0]), _bits(want[b, n])), f"track {b} behind a prefill of {n}"
    st.reset()
    got = _walk(st, xg)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))
    st.close(); enc.close()
