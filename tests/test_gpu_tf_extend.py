"""Several tokens per track in one call on the device (st.extend, flope_tf_stream_extend).

The contract, in every dtype and under every option: extend() of a chunk is, IN BITS, the same tokens fed by step() one column at a
time -- the rows it returns and what it leaves in the cache (held here by the bits of later steps) --, and any split of a track into
chunks gives one set of bits.  Where the forward's attention kernel for the shape is the generic one (read from enc.attention's
last_attn_kernel, not guessed) those are rows pos .. pos + len - 1 of enc(track, is_causal=True, window=W) in bits; elsewhere
(tf_attn_f32m, tf_attn_mfma, tf_attn_tiled) the rows are held to the fp64 restatements within the stream tests' tolerances:
2e-4 f32 / f32m, 1.5e-2 f16, 1.2e-1 bf16.

  1. extend == steps, every mode on two shapes     6. head dims that take the element-wise loads
  2. chunkings of one track                        7. NaN: reset, and the window forgets
  3. a mixed call                                  8. refusals (the INT_MAX refusal of a ring needs 2^31 tokens: tests/test_tf_extend_host.py)
  4. long: three trips of the key loop             9. sentinels around y, the rows behind a length
  5. windowed states, the ring wraps in a chunk   10. nothing else of the handle moves
 11. an extend of ONE token == a step at the same position: both are tf_attn_stream_row, the step with the promise that the chunk is
     one row
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tf_attn_causal_bound as CB
import tf_attn_window_bound as WB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f32m": torch.float32}
GENERIC = 0
SENTINEL = 1234.0
TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)
ODD = (5, 30, 3, 5, 1, 20)           # head_dim 6: element-wise loads in float32 and in 16 bits, and in tf_cache_append
MID = (5, 24, 3, 2, 1, 20)           # head_dim 12: three 16-byte vectors in float32, element-wise in 16 bits
HD16 = (5, 32, 3, 2, 1, 20)          # head_dim 16: whole 16-byte vectors in all three dtypes
MODES = [("f32", 0, 2e-4), ("f32m", 0, 2e-4), ("f16", 0, 1.5e-2), ("f16", 1, 1.5e-2), ("bf16", 0, 1.2e-1), ("bf16", 1, 1.2e-1)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sd_t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _encoder(dims, sd, dtype, max_tokens, tiled=0, fused=0, window_mfma=0):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, attn_tiled=tiled, fused=fused, window_mfma=window_mfma)
    enc.load_state_dict(_sd_t(sd))
    return enc


def _attn_kernel(enc, dims, dtype, B, L, window=0):
    """the attention kernel a causal forward of (B, L) launches on this handle"""
    enc.attention(torch.zeros(B, L, 3 * dims[1], dtype=TDT[dtype], device="cuda"), is_causal=True, window=window)
    return enc.last_attn_kernel


@pytest.fixture(scope="module")
def shapes():
    """name -> (dims, state dict, x [B, L, in], lengths, fp64 causal restatement of x); computed once, never changed"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_causal_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    wsd = T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)
    wx = np.random.default_rng(1).standard_normal((3, 50, 16)).astype(np.float32)
    res = {"toy": (TOY, sd, f["x"], [int(v) for v in f["lengths"]]), "wide": (WIDE, wsd, wx, [50, 1, 33])}
    return {k: v + (CB.causal_forward(v[1], v[2], v[0][3]),) for k, v in res.items()}


def _steps(st, x, start, stop, tracks=None):
    """tokens x[b, start[b] : stop[b]] of every sequence, one step() per column -> {b: [stop[b] - start[b], out]}"""
    n = x.shape[0]
    tracks = list(range(n)) if tracks is None else tracks
    got = {b: [] for b in range(n)}
    for k in range(max(e - s for s, e in zip(start, stop))):
        rows = [b for b in range(n) if start[b] + k < stop[b]]
        y = st.step(torch.stack([x[b, start[b] + k] for b in rows]), [tracks[b] for b in rows])
        for r, b in enumerate(rows):
            got[b].append(y[r].clone())
    return {b: torch.stack(v) for b, v in got.items() if v}


def _extend(st, x, start, stop, tracks=None):
    """the same tokens in ONE extend(): the sequences with stop > start, right-padded -> {b: [stop[b] - start[b], out]}"""
    n = x.shape[0]
    tracks = list(range(n)) if tracks is None else tracks
    seqs = [b for b in range(n) if stop[b] > start[b]]
    lens = [stop[b] - start[b] for b in seqs]
    xs = torch.zeros(len(seqs), max(lens), x.shape[2], device=x.device)
    for r, b in enumerate(seqs):
        xs[r, :lens[r]] = x[b, start[b]:stop[b]]
    y = st.extend(xs, lengths=lens, tracks=[tracks[b] for b in seqs])
    return {b: y[r, :lens[r]].clone() for r, b in enumerate(seqs)}


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        diff = int((_bits(a[k]) != _bits(b[k])).sum())
        assert diff == 0, f"{what}: sequence {k}: {diff} of {a[k].numel()} elements differ in bits"


# ---- 1. extend == steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["wide", "toy"])
@pytest.mark.parametrize("dtype,tiled,tol", MODES, ids=lambda v: str(v))
def test_extend_equals_steps(shapes, shape, dtype, tiled, tol):
    dims, sd, x, lens, full = shapes[shape]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L, tiled)
    xg = torch.from_numpy(x).cuda()
    kernel = _attn_kernel(enc, dims, dtype, B, L)
    tracks = [(b * 2 + 1) % B for b in range(B)] if B % 2 else [B - 1 - b for b in range(B)]       # a permutation
    assert sorted(tracks) == list(range(B)) and tracks != list(range(B))
    a, s = enc.open_stream(B, L + 2), enc.open_stream(B, L + 2)
    zero, half = [0] * B, [n // 2 for n in lens]                        # a chunk on empty tracks, then a ragged one behind it (lengths of 1 among them)
    ya, ys = _extend(a, xg, zero, half, tracks), _steps(s, xg, zero, half, tracks)
    _same(ya, ys, "the first chunk")
    yb, yt = _extend(a, xg, half, lens, tracks), _steps(s, xg, half, lens, tracks)
    _same(yb, yt, "the chunk behind it")
    assert 1 in [n - h for n, h in zip(lens, half)]
    torch.cuda.synchronize()
    assert a.positions == s.positions == [lens[tracks.index(t)] for t in range(B)]
    got = {b: torch.cat([ya[b], yb[b]]) if b in ya else yb[b] for b in yb}
    err = max(float(np.abs(got[b].cpu().numpy() - full[b, :lens[b]]).max()) for b in got)
    print(f"{dtype} attn_tiled={tiled} {shape} (attention kernel {kernel}): extend |y - fp64|max {err:.3e}, tolerance {tol}")
    if kernel == GENERIC:
        want = enc(xg, is_causal=True)
        for b in got:
            assert torch.equal(_bits(got[b]), _bits(want[b, :lens[b]])), f"sequence {b} against the causal forward"
    assert err < tol
    # the caches hold the same bits: two further steps of every track on both states
    new = torch.randn(B, 2, dims[0], generator=torch.Generator().manual_seed(9)).cuda()
    _same(_steps(a, new, zero, [2] * B, tracks), _steps(s, new, zero, [2] * B, tracks), "two further steps")
    a.close(); s.close(); enc.close()


# ---- 2. chunkings ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tiled,tol", MODES, ids=lambda v: str(v))
def test_chunkings_of_one_track(shapes, dtype, tiled, tol):
    dims, sd, x, lens, full = shapes["toy"]
    L = x.shape[1]
    xg = torch.from_numpy(x).cuda()[[0, 5]].contiguous()               # the two tracks of 15 tokens
    ref = full[[0, 5]]
    enc = _encoder(dims, sd, dtype, 2 * L, tiled)
    kernel = _attn_kernel(enc, dims, dtype, 2, L)
    outs = []
    for split in ([15], [4, 1, 7, 3], [1] * 15):
        st = enc.open_stream(2, L)
        at, rows = 0, []
        for m in split:
            rows.append(st.extend(xg[:, at:at + m].contiguous()).clone())
            at += m
        assert st.positions == [L, L]
        outs.append(torch.cat(rows, dim=1))
        st.close()
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2])), "a split changed the bits"
    err = float(np.abs(outs[0].cpu().numpy() - ref).max())
    print(f"{dtype} attn_tiled={tiled} (attention kernel {kernel}): |y - fp64|max {err:.3e}, tolerance {tol}")
    assert err < tol
    if kernel == GENERIC:
        assert torch.equal(_bits(outs[0]), _bits(enc(xg, is_causal=True))), "against the causal forward"
        st = enc.open_stream(2, L)
        assert torch.equal(_bits(outs[0]), _bits(st.prefill(xg))), "against prefill"
        st.close()
    enc.close()


# ---- 3. a mixed call ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_a_mixed_call_equals_each_track_alone(shapes, dtype):
    dims, sd, x, _, _ = shapes["toy"]
    B, L = x.shape[0], x.shape[1]
    enc = _encoder(dims, sd, dtype, B * L)
    assert _attn_kernel(enc, dims, dtype, B, L) == GENERIC
    xg = torch.from_numpy(x).cuda()
    held = [0, 0, 3, 6, 5, 9]                                           # tracks 0, 1 empty; 2, 3 mid-way by extend; 4, 5 behind a prefill
    take = [4, 1, 7, 2, 10, 1]                                          # this call's lengths
    order = [3, 0, 5, 1, 4, 2]

    def history(st, b, track):
        if b in (2, 3):
            st.extend(xg[b:b + 1, :held[b]].contiguous(), tracks=[track])
        elif b in (4, 5):
            st.prefill(xg[b:b + 1, :held[b]].contiguous(), tracks=[track])

    st = enc.open_stream(B, L)
    st.extend(torch.stack([xg[2], xg[3]])[:, :6].contiguous(), lengths=[3, 6], tracks=[2, 3])
    st.prefill(torch.stack([xg[4], xg[5]])[:, :9].contiguous(), lengths=[5, 9], tracks=[4, 5])
    assert st.positions == held
    xs = torch.zeros(B, max(take), dims[0], device="cuda")
    for r, b in enumerate(order):
        xs[r, :take[b]] = xg[b, held[b]:held[b] + take[b]]
    y = st.extend(xs, lengths=[take[b] for b in order], tracks=order)
    assert st.positions == [h + t for h, t in zip(held, take)]
    for r, b in enumerate(order):
        one = enc.open_stream(1, L)
        history(one, b, 0)
        alone = one.extend(xg[b:b + 1, held[b]:held[b] + take[b]].contiguous())
        assert torch.equal(_bits(y[r, :take[b]]), _bits(alone[0])), f"track {b} in the mixed call against itself alone"
        one.close()
    st.close(); enc.close()


# ---- 4. long --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_long_cache_60_then_chunk_70(shapes, dtype):
    """queries with up to 130 keys: three trips of the 64-lane key loop, the split between cache and chunk inside a trip (key 60) and
    inside an unrolled group of the value pass (60 = 3 x 16 + 12)"""
    dims, sd = shapes["toy"][:2]
    n, L = 2, 130
    enc = _encoder(dims, sd, dtype, n * L)
    xg = torch.randn(n, L, dims[0], generator=torch.Generator().manual_seed(3)).cuda()
    assert _attn_kernel(enc, dims, dtype, n, L) == GENERIC
    want = enc(xg, is_causal=True).clone()
    a, s = enc.open_stream(n, L), enc.open_stream(n, L)
    first = a.extend(xg[:, :60].contiguous()).clone()
    second = a.extend(xg[:, 60:].contiguous()).clone()
    walked = _steps(s, xg, [0, 0], [L, L])
    torch.cuda.synchronize()
    got = torch.cat([first, second], dim=1)
    assert a.positions == s.positions == [L, L]
    assert torch.equal(_bits(got), _bits(torch.stack([walked[0], walked[1]]))), "against 130 steps"
    assert torch.equal(_bits(got), _bits(want)), "against the causal forward"
    a.close(); s.close(); enc.close()


# ---- 5. windowed states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,W", [(8, 8), (8, 5), (16, 1)])
@pytest.mark.parametrize("dtype", ["f32", "f32m", "f16", "bf16"])
def test_windowed_states(shapes, dtype, capacity, W):
    """chunks of 1, 2, 7 and 20 (> capacity) per track, in another order on every track: the ring wraps inside a chunk, the runs of
    cached rows wrap, and at capacity == W every chunk of two tokens overwrites a key its first query still sees"""
    dims, sd = shapes["toy"][:2]
    n, chunks = 3, [1, 2, 7, 20]
    L = sum(chunks)
    enc = _encoder(dims, sd, dtype, n * L)
    assert _attn_kernel(enc, dims, dtype, n, L, window=W) == GENERIC
    xg = torch.randn(n, L, dims[0], generator=torch.Generator().manual_seed(6)).cuda()
    want = enc(xg, is_causal=True, window=W).clone()
    a, s = enc.open_stream(n, capacity, window=W), enc.open_stream(n, capacity, window=W)
    at = [0] * n
    for k in range(len(chunks)):
        stop = [at[b] + chunks[(k + b) % len(chunks)] for b in range(n)]
        ya, ys = _extend(a, xg, at, stop), _steps(s, xg, at, stop)
        _same(ya, ys, f"call {k} against steps")
        for b in range(n):
            assert torch.equal(_bits(ya[b]), _bits(want[b, at[b]:stop[b]])), f"call {k}, track {b} against the windowed forward"
        at = stop
    assert a.positions == s.positions == [L] * n
    new = torch.randn(n, 2, dims[0], generator=torch.Generator().manual_seed(9)).cuda()
    _same(_steps(a, new, [0] * n, [2] * n), _steps(s, new, [0] * n, [2] * n), "two further steps")
    a.close(); s.close(); enc.close()


def test_windowed_state_on_a_handle_that_keeps_its_mfma_kernel(shapes):
    dims, sd, x, lens, _ = shapes["wide"]
    B, L, W, capacity = x.shape[0], x.shape[1], 8, 11
    enc = _encoder(dims, sd, "f16", B * L, window_mfma=1)
    xg = torch.from_numpy(x).cuda()
    full = WB.window_forward(sd, x, W, num_heads=dims[3])
    a, s = enc.open_stream(B, capacity, window=W), enc.open_stream(B, capacity, window=W)
    half = [n // 2 for n in lens]
    ya, ys = _extend(a, xg, [0] * B, half), _steps(s, xg, [0] * B, half)
    _same(ya, ys, "the first chunk")
    yb, yt = _extend(a, xg, half, lens), _steps(s, xg, half, lens)
    _same(yb, yt, "the chunk behind it")
    err = max(float(np.abs(torch.cat([ya[b], yb[b]] if b in ya else [yb[b]]).cpu().numpy() - full[b, :lens[b]]).max()) for b in yb)
    print(f"f16 window_mfma=1 wide: extend |y - fp64|max {err:.3e}, tolerance 1.5e-2")
    assert err < 1.5e-2
    a.close(); s.close(); enc.close()


# ---- 6. the element-wise loads --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 5], ids=["linear", "ring"])
@pytest.mark.parametrize("dims", [ODD, MID], ids=["hd6", "hd12"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_head_dims_without_whole_vectors(dims, dtype, window):
    from oracle import tf_encoder_ref as T
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=7)
    B, L = 3, 21
    enc = _encoder(dims, sd, dtype, B * L)
    assert _attn_kernel(enc, dims, dtype, B, L, window=window) == GENERIC
    xg = torch.randn(B, L, dims[0], generator=torch.Generator().manual_seed(4)).cuda()
    want = enc(xg, is_causal=True, window=window).clone()
    capacity = 7 if window else L
    a, s = enc.open_stream(B, capacity, window=window), enc.open_stream(B, capacity, window=window)
    cut, lens = [9, 1, 5], [L, 2, L - 1]
    for start, stop in (([0] * B, cut), (cut, lens)):
        ya, ys = _extend(a, xg, start, stop), _steps(s, xg, start, stop)
        _same(ya, ys, "against steps")
        for b in ya:
            assert torch.equal(_bits(ya[b]), _bits(want[b, start[b]:stop[b]])), f"track {b} against the forward"
    assert a.positions == s.positions == lens
    a.close(); s.close(); enc.close()


# ---- 7. NaN ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_nan_is_forgotten_by_reset_and_by_the_window(shapes, dtype):
    dims, sd, x, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, dtype, 64)
    xg = torch.from_numpy(x).cuda()[:2].contiguous()
    clean = enc.open_stream(2, 8)
    want = clean.extend(xg[:, :6].contiguous()).clone()
    st = enc.open_stream(2, 8)
    y = st.extend(torch.full((1, 8, dims[0]), float("nan"), device="cuda"), tracks=[1])      # every cache row of track 1 holds NaN
    assert torch.isnan(y).all() and st.positions == [0, 8]
    st.reset([1])
    got = st.extend(xg[:, :6].contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), "a stale cache row was read"
    clean.close(); st.close()
    # a ring: the output at position t depends on tokens t - num_layers (W - 1) .. t, so that many clean tokens behind the NaN ones
    # plus one give a finite row, which is the last row of the windowed forward of the clean tokens (every window of it is full)
    W, cap, nl = 4, 6, dims[4]
    need = nl * (W - 1) + 1
    wantw = enc(xg, is_causal=True, window=W).clone()
    st = enc.open_stream(2, cap, window=W)
    y = st.extend(torch.full((1, 2 * cap + 1, dims[0]), float("nan"), device="cuda"), tracks=[1])
    assert torch.isnan(y).all() and st.positions == [0, 2 * cap + 1]
    got = st.extend(xg[1:2, :need].contiguous(), tracks=[1])
    assert torch.isnan(got[0, need - 2]).any(), "the receptive field is num_layers (W - 1) + 1 tokens"
    assert torch.isfinite(got[0, need - 1]).all(), "a stale row was read"
    assert torch.equal(_bits(got[0, need - 1]), _bits(wantw[1, need - 1])), "the window has forgotten the NaN tokens"
    assert st.positions == [0, 2 * cap + 1 + need]
    st.reset([1])
    assert torch.equal(_bits(st.extend(xg)), _bits(wantw))
    st.close(); enc.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(shapes):
    from flope_amd import _lib
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, x, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, "f32", 16)
    xg = torch.from_numpy(x).cuda()
    want = enc(xg[:1, :6].contiguous(), is_causal=True).clone()
    want3 = enc(xg[:3, :4].contiguous(), is_causal=True).clone()
    st = enc.open_stream(3, 6)
    y = st.extend(xg[:3, :4].contiguous(), lengths=[4, 2, 1])
    held = [4, 2, 1]
    assert st.positions == held
    c = lambda t: t.contiguous()
    refused = [
        (lambda: st.extend(c(xg[:1, :3]), tracks=[0]), r"lengths\[0\] = 3: track 0 holds 4 tokens, and the chunk would pass capacity = 6"),
        (lambda: st.extend(c(xg[:2, :5]), lengths=[1, 5], tracks=[2, 1]), r"lengths\[1\] = 5: track 1 holds 2 tokens.*capacity = 6"),
        (lambda: st.extend(c(xg[:3, :3])), r"lengths\[0\] = 3: track 0 holds 4"),
        (lambda: st.extend(c(xg[:2, :1]), tracks=[1, 1]), r"tracks\[1\] = 1 names a track an earlier sequence names \(one sequence per track and call\)"),
        (lambda: st.extend(c(xg[:2, :1]), tracks=[1, 3]), r"tracks\[1\] = 3 is outside 0 \.\. 2"),
        (lambda: st.extend(c(xg[:2, :1]), tracks=[-1, 2]), r"tracks\[0\] = -1 is outside"),
        (lambda: st.extend(c(xg[:0, :1]), tracks=[]), r"NULL buffer|batch must be positive"),
        (lambda: st.extend(c(xg[:4, :1]), tracks=[0, 1, 2, 1]), r"n = 4 is outside"),
        (lambda: st.extend(c(xg[:2, :1])), r"n = 2 is outside .* tracks_host is NULL"),
        (lambda: st.extend(c(xg[:2, :1]), tracks=[1]), r"tracks has 1 values for 2 sequences"),
        (lambda: st.extend(c(xg[:2, :2]), lengths=[2, 0], tracks=[1, 2]), r"lengths\[1\] = 0 is outside 1 \.\. 2"),
        (lambda: st.extend(c(xg[:2, :2]), lengths=[3, 1], tracks=[1, 2]), r"lengths\[0\] = 3 is outside 1 \.\. 2"),
        (lambda: st.extend(c(xg[:2, :2]), lengths=[1], tracks=[1, 2]), r"lengths has 1 values"),
        (lambda: st.extend(c(xg[:2, :1, :5]), tracks=[1, 2]), r"expected \[n, L, 16\]"),
        (lambda: st.extend(c(xg[:2, 1]), tracks=[1, 2]), r"expected \[n, L, 16\]"),
        (lambda: st.extend(c(xg[:2, :1]), tracks=[1, 2], out=torch.empty(2, 2, dims[2], device="cuda")), r"out must be a contiguous float32"),
    ]
    for call, msg in refused:
        with pytest.raises(ValueError, match=msg):
            call()
        assert st.positions == held, msg
    with pytest.raises(RuntimeError, match="must live on"):
        st.extend(xg[:2, :1].cpu(), tracks=[1, 2])
    # NULL buffers, straight at the entry point
    assert enc.lib.flope_tf_stream_extend(st.state, None, 1, 1, None, (C.c_int * 1)(1), None, None) == _lib.EINVAL
    assert "NULL buffer" in enc.lib.flope_tf_last_error(enc.handle).decode() and st.positions == held
    # sum(lengths) > max_tokens = 16: refused on a state with room for it
    big = enc.open_stream(3, 64)
    with pytest.raises(ValueError, match="sum of lengths exceeds max_tokens"):
        big.extend(xg[:3, :6].contiguous())
    assert big.positions == [0, 0, 0]
    big.close()
    # track 0 filled exactly to capacity: accepted, and the right bits; the next call on it is refused
    y = st.extend(xg[:1, 4:6].contiguous(), tracks=[0])
    assert torch.equal(_bits(y[0]), _bits(want[0, 4:6])) and st.positions == [6, 2, 1]
    with pytest.raises(ValueError, match=r"lengths\[0\] = 1: track 0 holds 6 tokens, and the chunk would pass capacity = 6"):
        st.extend(xg[:1, :1].contiguous(), tracks=[0])
    y = st.extend(torch.stack([xg[1, 2:4], xg[2, 1:3]]), lengths=[2, 2], tracks=[1, 2])      # the next valid call returns the right bits
    assert torch.equal(_bits(y[0]), _bits(want3[1, 2:4])) and torch.equal(_bits(y[1]), _bits(want3[2, 1:3])) and st.positions == [6, 4, 3]
    # a stream outlives neither its close() nor its encoder's; a handle without weights refuses
    st.close()
    with pytest.raises(RuntimeError, match="stream has been closed"):
        st.extend(xg[:3, :1].contiguous())
    st2 = enc.open_stream(1, 2)
    enc.close()
    with pytest.raises(RuntimeError, match="encoder of this stream has been closed"):
        st2.extend(xg[:1, :2].contiguous())
    st2.close()
    bare = TransformerEncoder(*dims, dtype="f32", max_tokens=16)
    st3 = bare.open_stream(1, 4)
    with pytest.raises(RuntimeError, match="weights not loaded"):
        st3.extend(xg[:1, :2].contiguous())
    assert st3.positions == [0]
    st3.close(); bare.close()


# ---- 9. sentinels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 4], ids=["linear", "ring"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_sentinels_around_y_and_the_rows_behind_a_length(shapes, dtype, window):
    dims, sd, x, lens, _ = shapes["toy"]
    B, L, o = x.shape[0], x.shape[1], dims[2]
    enc = _encoder(dims, sd, dtype, B * L)
    xg = torch.from_numpy(x).cuda()
    bias = torch.from_numpy(np.asarray(sd["out_layer.bias"])).cuda()
    st = enc.open_stream(B, 6 if window else 2 * L, window=window)
    big = torch.full((64 + B * L * o + 64,), SENTINEL, device="cuda")
    for _ in range(2):                                                  # on empty tracks, then behind what they hold
        big.fill_(SENTINEL)
        y = st.extend(xg, lengths=lens, out=big[64:64 + B * L * o].view(B, L, o))
        torch.cuda.synchronize()
        assert (big[:64] == SENTINEL).all() and (big[64 + B * L * o:] == SENTINEL).all() and torch.isfinite(y).all()
        for b, n in enumerate(lens):
            assert torch.equal(_bits(y[b, n:]), _bits(bias.expand(L - n, o))), f"rows behind length {n} of sequence {b}"
    assert st.positions == [2 * n for n in lens]
    st.close(); enc.close()


# ---- 10. nothing else moves -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,fused", [("f32", 0), ("f32", 1), ("f16", 0)])
def test_forwards_around_extends_keep_their_bits(shapes, dtype, fused):
    dims, sd, x, lens, _ = shapes["toy"]
    B, L, W = x.shape[0], x.shape[1], 4
    enc = _encoder(dims, sd, dtype, B * L, fused=fused)
    xg = torch.from_numpy(x).cuda()
    plain, causal, windowed = enc(xg).clone(), enc(xg, is_causal=True).clone(), enc(xg, is_causal=True, window=W).clone()
    enc(xg)
    assert enc.last_forward_fused == bool(fused)
    plan = enc.forward_plan(B, L)
    st, sw = enc.open_stream(B, L), enc.open_stream(B, 6, window=W)
    for causal_before, window_before in ((0, 0), (1, 0), (1, 3)):
        enc.set_option("window", 0)
        enc.set_option("causal", causal_before)
        enc.set_option("window", window_before)
        st.reset(); sw.reset()
        y = st.extend(xg, lengths=lens)
        yw = sw.extend(xg, lengths=lens)
        assert enc.set_option("causal", causal_before) == causal_before, "extend changed option causal"
        assert enc.set_option("window", window_before) == window_before, "extend changed option window"
        assert enc.last_forward_fused == bool(fused)
        for b, n in enumerate(lens):                                    # (under fused = 1: the launch sequence gave the single launch's bits)
            assert torch.equal(_bits(y[b, :n]), _bits(causal[b, :n])) and torch.equal(_bits(yw[b, :n]), _bits(windowed[b, :n]))
    enc.set_option("window", 0)
    enc.set_option("causal", 0)
    assert enc.forward_plan(B, L) == plan == ("fused" if fused else "launches")
    assert torch.equal(_bits(enc(xg)), _bits(plain)) and enc.last_forward_fused == bool(fused)
    assert torch.equal(_bits(enc(xg, is_causal=True)), _bits(causal)) and enc.last_forward_fused == bool(fused)
    assert torch.equal(_bits(enc(xg, is_causal=True, window=W)), _bits(windowed))
    st.close(); sw.close(); enc.close()


def test_two_states_extended_alternately(shapes):
    dims, sd, x, _, _ = shapes["toy"]
    enc = _encoder(dims, sd, "f32", 64)
    xg = torch.from_numpy(x).cuda()
    xa, xb = xg[:2, :8].contiguous(), xg[2:5, :8].flip(1).contiguous()
    sa, sb = enc.open_stream(2, 8), enc.open_stream(3, 5, window=3)
    ya, yb = [], []
    for t in (0, 3, 4):                                                 # chunks of 3, 1 and 4
        m = {0: 3, 3: 1, 4: 4}[t]
        ya.append(sa.extend(xa[:, t:t + m].contiguous()))
        yb.append(sb.extend(xb[:, t:t + m].contiguous()))
    ya, yb = torch.cat(ya, 1), torch.cat(yb, 1)
    assert torch.equal(_bits(ya), _bits(enc(xa, is_causal=True))) and torch.equal(_bits(yb), _bits(enc(xb, is_causal=True, window=3)))
    s1, s2 = enc.open_stream(2, 8), enc.open_stream(3, 5, window=3)
    assert torch.equal(_bits(ya), _bits(s1.extend(xa))) and torch.equal(_bits(yb), _bits(s2.extend(xb)))
    for s in (sa, sb, s1, s2):
        s.close()
    enc.close()


# ---- 11. an extend of one token is a step ---------------------------------------------------------------------------------------------
def _wrapping_positions(capacity, W, last, run):
    """positions <= last of a full window whose W - 1 cached keys wrap in the ring with at least `run` rows on each side of the wrap"""
    out = []
    for p in range(W, last + 1):
        first = min(W - 1, capacity - (p - W + 1) % capacity)          # rows from the first visible key's row to the end of the ring
        if first >= run and W - 1 - first >= run:
            out.append(p)
    return out


ONE_TOKEN_STATES = {
    # no trip of the unrolled value loop (16 keys a trip), one trip, two trips and a tail, the score pass's second trip (64 keys a trip)
    "linear": (72, 0, [0, 1, 15, 16, 17, 33, 63, 64, 65]),
    # both runs of cached rows short, the wrap met at every phase
    "ringA": (8, 5, list(range(21))),
    # an unrolled trip in both runs of cached rows, and the positions around them up to 90
    "ringB": (40, 36, sorted(set([35, 55, 60, 79, 90] + _wrapping_positions(40, 36, 90, 16)))),
}


@pytest.mark.parametrize("state", list(ONE_TOKEN_STATES))
@pytest.mark.parametrize("dims", [ODD, HD16], ids=["hd6", "hd16"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_extend_of_one_token_equals_a_step(dims, dtype, state):
    """one track per position, filled by a prefill; then ONE step() of every track on one state and ONE extend() of one token per
    track on the other: the same raw bits, and the same cache behind them (a further step of every track)"""
    from oracle import tf_encoder_ref as T
    capacity, W, positions = ONE_TOKEN_STATES[state]
    if state == "ringB":
        assert _wrapping_positions(40, 36, 90, 16) == [56, 57, 58, 59]
    sd = T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=7)
    n, L = len(positions), max(positions)
    enc = _encoder(dims, sd, dtype, sum(positions) + n)
    x = torch.randn(n, L + 2, dims[0], generator=torch.Generator().manual_seed(11)).cuda()
    held = [t for t in range(n) if positions[t] > 0]
    a, s = enc.open_stream(n, capacity, window=W), enc.open_stream(n, capacity, window=W)
    for st in (a, s):
        st.prefill(x[held, :L].contiguous(), lengths=[positions[t] for t in held], tracks=held)
        assert st.positions == positions
    for k in range(2):                                                  # the token at each track's position, then the one behind it
        tok = torch.stack([x[t, positions[t] + k] for t in range(n)])
        ys, ya = s.step(tok), a.extend(tok[:, None].contiguous())[:, 0]
        bad = [positions[t] + k for t in range(n) if not torch.equal(_bits(ys[t]), _bits(ya[t]))]
        assert not bad, f"{dtype} head_dim {dims[1] // dims[3]} {state}: extend of one token differs from the step at positions {bad}"
    assert a.positions == s.positions == [p + 2 for p in positions]
    a.close(); s.close(); enc.close()
