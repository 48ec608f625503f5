"""extend() on the 16-bit MFMA attention step on the device (option "extend_mfma", tf_attn16_extend).

  (a) the kernel alone through st.attention_extend, every chunk element within the derived bound of fp64 attention over the whole track
      (tf_attn_causal_bound / tf_attn_window16_bound.reference_of), the shapes of tests/tf_extend_mfma_emul.py, option 1 and option 0
      through the same hook, sentinels around the result and on the rows the call must not touch;
  (b) bits: with the option on, extend()'s rows are the rows of enc(track, is_causal=True[, window=W]) where that forward's attention is
      an MFMA kernel, for any split of the track, and the caches are prefill()'s (held by the bits of later steps);
  (c) whole calls against the fp64 restatements within the stream tests' tolerances (1.5e-2 f16, 1.2e-1 bf16), both options printed;
  (d) nothing else moves: NaN and reset, the option flipped on a live state, refused values, every other call's bits, refusals.
"""
import numpy as np
import pytest
import torch

import tf_attn_bound as AB
import tf_attn_causal_bound as CB
import tf_attn_window16_bound as W16
import tf_attn_window_bound as WB
import tf_extend_mfma_emul as EM

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
TOL = {"f16": 1.5e-2, "bf16": 1.2e-1}
GENERIC, MFMA64, TILED = 0, 1, 2
ROW, SPLIT, MFMA = 0, 1, 2
SENTINEL = 1234.0
TOY = (16, 32, 9, 4, 2, 64)              # head_dim 8: no MFMA form
WIDE = (16, 128, 9, 2, 2, 256)           # head_dim 64
HD32 = (16, 64, 9, 2, 2, 128)            # head_dim 32
HD128 = (16, 256, 9, 2, 2, 256)          # head_dim 128


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _bare(H, hd, dtype, max_tokens, extend_mfma=1):
    """a handle without weights: the hooks need none"""
    from flope_amd.tf_encoder import TransformerEncoder
    return TransformerEncoder(16, H * hd, 9, H, 1, 64, dtype=dtype, max_tokens=max_tokens, extend_mfma=extend_mfma)


@pytest.fixture(scope="module")
def sds():
    from oracle import tf_encoder_ref as T
    return {dims: T.synthetic_state_dict(dims[0], dims[1], dims[2], dims[4], dims[5], seed=5) for dims in (TOY, WIDE, HD32, HD128)}


def _encoder(sds, dims, dtype, max_tokens, **opts):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, **opts)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sds[dims].items()})
    return enc


def _forward_kernel(enc, dims, dtype, L, window=0):
    enc.attention(torch.zeros(1, L, 3 * dims[1], dtype=TDT[dtype], device="cuda"), is_causal=True, window=window)
    return enc.last_attn_kernel


def _x(n, L, seed=1):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, L, 16)).astype(np.float32)).cuda()


def _chunks(st, x, split, track=0, start=0):
    """tokens x[0, start:] of one track in extend() calls of the given lengths -> [sum(split), out]"""
    rows, at = [], start
    for m in split:
        rows.append(st.extend(x[:, at:at + m].contiguous(), tracks=[track])[0].clone())
        at += m
    return torch.cat(rows)


# ---- (a) the kernel alone ---------------------------------------------------------------------------------------------------------------
def _hook_case(dtype, W, capacity, seqs, H, hd):
    """seqs: [(cached, chunk)] of one call.  Runs the hook under option 1 and option 0, returns the worst err / bound of each."""
    n, L = len(seqs), max(c + m for c, m in seqs)
    d = H * hd
    enc = _bare(H, hd, dtype, sum(m for _, m in seqs) + 3)
    st = enc.open_stream(n, capacity, window=W)
    qkv = torch.full((n, L, 3 * d), float("nan"), dtype=TDT[dtype])                  # the padding behind a sequence is never read
    refs = []
    for b, (c, m) in enumerate(seqs):
        t = EM.track_qkv(c, m, H, hd, dtype)
        qkv[b, :c + m] = t[0]
        refs.append(W16.reference_of(t, H, dtype, W) if W else CB.reference_of(t, H, dtype))
    qg = qkv.cuda()
    worst = {}
    for opt, want_id in ((1, MFMA), (0, ROW)):
        assert enc.set_option("extend_mfma", opt) >= 0
        assert st.extend_plan() == ("mfma" if opt else "row")
        pad = 64
        big = torch.full((n * L * d + 2 * pad,), SENTINEL, dtype=TDT[dtype], device="cuda")
        out = big[pad:pad + n * L * d].view(n, L, d)
        got = st.attention_extend(qg, [c + m for c, m in seqs], [c for c, _ in seqs], out=out)
        torch.cuda.synchronize()
        assert st.last_attn_kernel == want_id and got.data_ptr() == out.data_ptr()
        assert (big[:pad] == SENTINEL).all() and (big[-pad:] == SENTINEL).all(), "wrote outside att"
        w = 0.0
        for b, (c, m) in enumerate(seqs):
            assert (out[b, :c] == SENTINEL).all() and (out[b, c + m:] == SENTINEL).all(), "wrote a row outside the chunk"
            O, bound = refs[b]
            r, where = AB.ratio(out[b:b + 1, c:c + m], O[:, c:], bound[:, c:])
            print(f"{dtype} option {opt} W={W} capacity={capacity} cached={c} chunk={m} H={H} hd={hd}: err / bound {r:.3g} at {where}")
            assert r <= 1.0, (opt, b, r, where)
            w = max(w, r)
        worst[opt] = w
        assert st.positions == [0] * n
    st.close(); enc.close()
    return worst


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", EM.LINEAR, ids=str)
def test_kernel_alone_linear(case, dtype):
    c, m, H, hd = case
    _hook_case(dtype, 0, c + m, [(c, m)], H, hd)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_kernel_alone_ragged_batch(dtype):
    cached, chunk, H, hd = EM.RAGGED
    _hook_case(dtype, 0, max(c + m for c, m in zip(cached, chunk)) + 5, list(zip(cached, chunk)), H, hd)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", EM.WINDOWED, ids=str)
def test_kernel_alone_windowed(case, dtype):
    W, capacity, c, m, H, hd = case
    _hook_case(dtype, W, capacity, [(c, m)], H, hd)


def test_kernel_alone_never_reads_a_stale_row():
    """the cache rows of a ring that hold no visible key are NaN (an older lap fed NaN): the chunk rows stay the clean call's bits"""
    W, capacity, c, m, H, hd = EM.WINDOWED[1]
    enc = _bare(H, hd, "f16", 256)
    st = enc.open_stream(1, capacity, window=W)
    t = EM.track_qkv(c, m, H, hd, "f16").cuda()
    clean = st.attention_extend(t, [c + m], [c]).clone()
    dirty = t.clone()
    dirty[0, :c - W + 1] = float("nan")                                               # keys below the first chunk query's window
    got = st.attention_extend(dirty, [c + m], [c])
    assert st.last_attn_kernel == MFMA
    assert torch.isfinite(got.float()).all() and torch.equal(_bits(got), _bits(clean))
    st.close(); enc.close()


# ---- (b) bits against the forward -------------------------------------------------------------------------------------------------------
CONFIGS = [(WIDE, "f16", 0), (WIDE, "f16", 1), (WIDE, "f16", 2), (WIDE, "bf16", 0), (HD32, "f16", 1), (HD128, "f16", 1), (HD128, "bf16", 1)]


@pytest.mark.parametrize("dims,dtype,tiled", CONFIGS, ids=str)
def test_any_split_gives_the_forwards_rows_in_bits(sds, dims, dtype, tiled):
    L = 70
    enc = _encoder(sds, dims, dtype, 256, attn_tiled=tiled, extend_mfma=1)
    kernel = _forward_kernel(enc, dims, dtype, L)
    assert kernel in (MFMA64, TILED), "the contract is stated where the forward's attention is an MFMA kernel"
    x = _x(1, L)
    want = enc(x, is_causal=True)[0].clone()
    pre = enc.open_stream(1, L + 2)
    assert torch.equal(_bits(pre.prefill(x)[0]), _bits(want))
    new = _x(1, 2, seed=9)
    after_prefill = torch.stack([pre.step(new[:, k].contiguous())[0].clone() for k in range(2)])
    for split in ([70], [31, 1, 33, 5], [1] * 70):
        st = enc.open_stream(1, L + 2)
        assert st.extend_plan() == "mfma"
        got = _chunks(st, x, split)
        diff = int((_bits(got) != _bits(want)).sum())
        assert diff == 0, f"forward kernel {kernel}, split {split[:4]}: {diff} of {got.numel()} elements differ from enc(x, is_causal=True)"
        assert st.positions == [L]
        # the caches agree: two further steps behind the extends and behind the prefill
        after = torch.stack([st.step(new[:, k].contiguous())[0].clone() for k in range(2)])
        assert torch.equal(_bits(after), _bits(after_prefill)), split[:4]
        st.close()
    pre.close(); enc.close()


def test_a_mixed_call_on_permuted_tracks(sds):
    enc = _encoder(sds, WIDE, "f16", 256, extend_mfma=1)
    lens, half, tracks = [50, 1, 33], [25, 0, 16], [2, 0, 1]
    x = _x(3, 50)
    st = enc.open_stream(3, 64)
    got = {}
    for start, stop in ((([0] * 3), half), (half, lens)):
        seqs = [b for b in range(3) if stop[b] > start[b]]
        ms = [stop[b] - start[b] for b in seqs]
        xs = torch.zeros(len(seqs), max(ms), 16, device="cuda")
        for r, b in enumerate(seqs):
            xs[r, :ms[r]] = x[b, start[b]:stop[b]]
        y = st.extend(xs, lengths=ms, tracks=[tracks[b] for b in seqs])
        for r, b in enumerate(seqs):
            got.setdefault(b, []).append(y[r, :ms[r]].clone())
    assert st.positions == [lens[tracks.index(t)] for t in range(3)]
    for b in range(3):
        alone = enc.open_stream(1, 64)
        want = _chunks(alone, x[b:b + 1], [m for m in (half[b], lens[b] - half[b]) if m])
        assert torch.equal(_bits(torch.cat(got[b])), _bits(want)), f"sequence {b} against the track alone"
        assert torch.equal(_bits(want), _bits(enc(x[b:b + 1, :lens[b]].contiguous(), is_causal=True)[0])), f"sequence {b} against the forward"
        alone.close()
    st.close(); enc.close()


@pytest.mark.parametrize("capacity,W", [(11, 8), (8, 8)])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_windowed_splits_give_the_windowed_forwards_rows_in_bits(sds, capacity, W, dtype):
    L = 30
    enc = _encoder(sds, WIDE, dtype, 256, window_mfma=1, extend_mfma=1)
    kernel = _forward_kernel(enc, WIDE, dtype, L, window=W)
    assert kernel in (MFMA64, TILED)
    x = _x(1, L, seed=3)
    want = enc(x, is_causal=True, window=W)[0].clone()
    for split in ([1, 2, 7, 20], [20, 7, 2, 1]):
        st = enc.open_stream(1, capacity, window=W)
        assert st.extend_plan() == "mfma"
        got = _chunks(st, x, split)
        diff = int((_bits(got) != _bits(want)).sum())
        assert diff == 0, f"capacity {capacity}, W {W}, split {split}: {diff} of {got.numel()} elements differ from the windowed forward"
        assert st.positions == [L]
        st.close()
    enc.close()


@pytest.mark.parametrize("dims,dtype", [(TOY, "f16"), (WIDE, "f32")], ids=str)
def test_shapes_the_kernel_does_not_take_keep_option_zeros_bits(sds, dims, dtype):
    x = _x(1, 40)
    rows = []
    for opt in (0, 1):
        enc = _encoder(sds, dims, dtype, 128, extend_mfma=opt)
        st = enc.open_stream(1, 48)
        assert st.extend_plan() == "row"
        rows.append(_chunks(st, x, [13, 1, 26]).clone())
        enc.set_option("step_split", 1)
        assert st.extend_plan() == ("split" if dims == TOY or dtype == "f32" else "row")
        st.close(); enc.close()
    assert torch.equal(_bits(rows[0]), _bits(rows[1]))


def test_extend_mfma_wins_over_step_split_for_extend_only(sds):
    enc = _encoder(sds, WIDE, "f16", 128, extend_mfma=1, step_split=1)
    st = enc.open_stream(1, 48)
    assert st.extend_plan() == "mfma" and st.step_plan == "split"
    enc.set_option("extend_mfma", 0)
    assert st.extend_plan() == "split"
    st.close(); enc.close()


# ---- (c) whole calls against fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("W", [0, 8])
def test_whole_calls_against_fp64(sds, dtype, W):
    lens, L = [50, 1, 33], 50
    x = _x(3, L)
    xn = x.cpu().numpy()
    ref = WB.window_forward(sds[WIDE], xn, W, lens, num_heads=WIDE[3]) if W else CB.causal_forward(sds[WIDE], xn, WIDE[3])
    errs = {}
    for opt in (0, 1):
        enc = _encoder(sds, WIDE, dtype, 256, extend_mfma=opt)
        st = enc.open_stream(3, 64 if not W else 11, window=W)
        half = [n // 2 for n in lens]
        got = {b: [] for b in range(3)}
        seqs = [b for b in range(3) if half[b]]
        pre = st.prefill(torch.stack([x[b] for b in seqs])[:, :max(half)].contiguous(), lengths=[half[b] for b in seqs], tracks=seqs)
        for r, b in enumerate(seqs):
            got[b].append(pre[r, :half[b]].clone())
        at = list(half)
        for step in (3, 100):                                                        # a ragged chunk of up to 3 tokens, then all that is left
            ms = [min(step, lens[b] - at[b]) for b in range(3)]
            seqs = [b for b in range(3) if ms[b] > 0]
            xs = torch.zeros(len(seqs), max(ms), 16, device="cuda")
            for r, b in enumerate(seqs):
                xs[r, :ms[b]] = x[b, at[b]:at[b] + ms[b]]
            y = st.extend(xs, lengths=[ms[b] for b in seqs], tracks=seqs)
            for r, b in enumerate(seqs):
                got[b].append(y[r, :ms[b]].clone())
                at[b] += ms[b]
        assert st.positions == lens
        errs[opt] = max(float(np.abs(torch.cat(got[b]).cpu().numpy() - ref[b, :lens[b]]).max()) for b in range(3))
        st.close(); enc.close()
    print(f"{dtype} W={W}: prefill of half + ragged extends |y - fp64|max: option 0 {errs[0]:.3e}, option 1 {errs[1]:.3e}, tolerance {TOL[dtype]}")
    assert errs[0] < TOL[dtype] and errs[1] < TOL[dtype]


# ---- (d) nothing else moves -------------------------------------------------------------------------------------------------------------
def test_nan_tokens_and_reset(sds):
    enc = _encoder(sds, WIDE, "f16", 256, extend_mfma=1)
    x = _x(1, 40)
    st = enc.open_stream(1, 48)
    clean = _chunks(st, x, [17, 23]).clone()
    st.reset()
    bad = st.extend(torch.full((1, 30, 16), float("nan"), device="cuda"))
    assert torch.isnan(bad).all() and st.positions == [30]
    st.reset()
    assert torch.equal(_bits(_chunks(st, x, [17, 23])), _bits(clean))
    st.close(); enc.close()


def test_a_ring_forgets_nan_tokens(sds):
    """2 capacity + 1 NaN tokens, then num_layers (W - 1) + 1 clean ones, one per call: the last row sees clean tokens only, and it is the
    row of the windowed forward over finite tokens at the same absolute positions.  One per call, because a matrix instruction multiplies
    a masked probability of exactly 0 by the key's value, and 0 x NaN is NaN: a query is NaN when a NaN key lies in a 32-key step its
    WAVE takes, at or above the first key its workgroup sees.  Fed as one chunk, these clean tokens therefore stay NaN; at
    these 38 positions the forward of the same tokens, NaN ones included, has the same steps and the same NaN rows -- the second half
    of this test, which claims no more than this case."""
    capacity, W = 11, 8
    enc = _encoder(sds, WIDE, "f16", 256, window_mfma=1, extend_mfma=1)
    n_bad, n_clean = 2 * capacity + 1, WIDE[4] * (W - 1) + 1
    x = _x(1, n_bad + n_clean, seed=4)
    assert _forward_kernel(enc, WIDE, "f16", n_bad + n_clean, window=W) in (MFMA64, TILED)
    want = enc(x, is_causal=True, window=W)[0, -1].clone()
    st = enc.open_stream(1, capacity, window=W)
    assert st.extend_plan() == "mfma"
    nan = torch.full((1, n_bad, 16), float("nan"), device="cuda")
    assert torch.isnan(st.extend(nan)).all()
    got = _chunks(st, x, [1] * n_clean, start=n_bad)
    assert torch.isnan(got[0]).all(), "the first clean token still sees NaN keys"
    assert torch.isnan(got[-2]).any(), "the receptive field is num_layers (W - 1) + 1 tokens"
    assert torch.isfinite(got[-1]).all(), "a stale row was read"
    assert torch.equal(_bits(got[-1]), _bits(want)), "the window has forgotten the NaN tokens"
    assert st.positions == [n_bad + n_clean]
    # ... and as one chunk: here NaN where the forward of the very same tokens is NaN, its bits elsewhere
    xn = torch.cat([nan, x[:, n_bad:]], dim=1)
    fwd = enc(xn, is_causal=True, window=W)[0, n_bad:].clone()
    st.reset()
    st.extend(nan)
    one = st.extend(x[:, n_bad:].contiguous())[0]
    assert torch.equal(torch.isnan(one), torch.isnan(fwd))
    assert torch.equal(_bits(torch.nan_to_num(one)), _bits(torch.nan_to_num(fwd)))
    st.close(); enc.close()


def test_option_flipped_on_a_live_state(sds):
    lens = [50]
    x = _x(1, 50)
    ref = CB.causal_forward(sds[WIDE], x.cpu().numpy(), WIDE[3])
    enc = _encoder(sds, WIDE, "f16", 256)
    st = enc.open_stream(1, 64)
    rows, at = [], 0
    for opt, m in ((1, 20), (0, 7), (1, 23)):
        assert enc.set_option("extend_mfma", opt) == (0 if not rows else 1 - opt)
        assert st.extend_plan() == ("mfma" if opt else "row")
        rows.append(st.extend(x[:, at:at + m].contiguous())[0].clone())
        at += m
        assert st.positions == [at]
    err = float(np.abs(torch.cat(rows).cpu().numpy() - ref[0]).max())
    print(f"f16: option flipped at positions 0, 20, 27: |y - fp64|max {err:.3e}, tolerance {TOL['f16']}")
    assert err < TOL["f16"] and st.positions == lens
    st.close(); enc.close()


def test_refused_values():
    from flope_amd.tf_encoder import TransformerEncoder
    for bad in (2, -1):
        with pytest.raises(ValueError, match="extend_mfma must be 0 or 1"):
            TransformerEncoder(*WIDE, dtype="f16", max_tokens=64, extend_mfma=bad)
    enc = _bare(2, 64, "f16", 64, extend_mfma=1)
    with pytest.raises(ValueError, match="extend_mfma is 0 or 1"):
        enc.set_option("extend_mfma", 2)
    assert enc.set_option("extend_mfma", 1) == 1, "a refused value changed the option"
    f32 = _bare(2, 64, "f32", 64, extend_mfma=1)                                     # stored and ignored
    st = f32.open_stream(1, 8)
    assert st.extend_plan() == "row" and f32.set_option("extend_mfma", 0) == 1
    st.close(); f32.close(); enc.close()


def test_every_other_call_keeps_its_bits(sds):
    x = _x(2, 40)
    q = EM.track_qkv(10, 30, 2, 64, "f16").cuda()
    runs = []
    for opt in (0, 1):
        enc = _encoder(sds, WIDE, "f16", 256, extend_mfma=opt)
        st = enc.open_stream(2, 48)
        out = [enc(x), enc(x, is_causal=True), enc.attention(q, is_causal=True), st.prefill(x, lengths=[40, 13]),
               st.step(x[:, 0].contiguous(), [1, 0]), st.attention(q.expand(2, -1, -1).contiguous(), lengths=[40, 9])]
        runs.append([t.clone() for t in out])
        assert st.step_plan == "row"
        st.close(); enc.close()
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


def test_refusals_of_extend_are_unchanged(sds):
    enc = _encoder(sds, WIDE, "f16", 64, extend_mfma=1)
    st = enc.open_stream(2, 16)
    st.extend(_x(2, 5))
    calls = [(lambda: st.extend(_x(2, 3), tracks=[1, 1]), "names a track an earlier"),
             (lambda: st.extend(_x(2, 12)), "would pass capacity"),
             (lambda: st.extend(_x(2, 3), lengths=[0, 3]), "outside 1"),
             (lambda: st.extend(_x(1, 3), tracks=[2]), "outside 0"),
             (lambda: st.extend(_x(2, 40), lengths=[40, 40]), "max_tokens")]
    for call, msg in calls:
        with pytest.raises(ValueError, match=msg):
            call()
        assert st.positions == [5, 5]
    st.close(); enc.close()


def test_refusals_of_the_hook():
    enc = _bare(2, 64, "f16", 31)
    st = enc.open_stream(2, 16)
    q = torch.zeros(2, 12, 3 * 128, dtype=torch.float16, device="cuda")
    out = torch.full((2, 12, 128), SENTINEL, dtype=torch.float16, device="cuda")
    bad = [(q, [12, 12], [0, 12], "cached\\[1\\] = 12"), (q, [12, 12], [-1, 0], "cached\\[0\\] = -1"), (q, [13, 12], [0, 0], "lengths\\[0\\] = 13"),
           (q, [0, 12], [0, 0], "lengths\\[0\\] = 0"), (q, [12, 12], [0, 0, 0], "3 values"),
           (torch.zeros(3, 12, 384, dtype=torch.float16, device="cuda"), [12] * 3, [0] * 3, "n = 3"),
           (torch.zeros(2, 20, 384, dtype=torch.float16, device="cuda"), [20, 3], [0, 0], "above capacity"),
           (torch.zeros(2, 16, 384, dtype=torch.float16, device="cuda"), [16, 16], [0, 0], "max_tokens"),
           (q.float(), [12, 12], [0, 0], "expected a contiguous")]
    for qq, lens, cached, msg in bad:
        with pytest.raises(ValueError, match=msg):
            st.attention_extend(qq, lens, cached, out=out if qq.shape[:2] == (2, 12) and qq.dtype == torch.float16 else None)
    with pytest.raises(ValueError, match="out must be"):
        st.attention_extend(q, [12, 12], [0, 0], out=out[:, :6])
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a refused call wrote"
    from flope_amd import _lib
    assert enc.lib.flope_tf_stream_attention_extend(st.state, q.data_ptr() + 2, 2, 12, (_lib.C.c_int * 2)(12, 12), (_lib.C.c_int * 2)(0, 0), out.data_ptr(), None) == _lib.EINVAL
    assert "not aligned" in enc.lib.flope_tf_last_error(enc.handle).decode()
    assert enc.lib.flope_tf_stream_attention_extend(st.state, None, 2, 12, (_lib.C.c_int * 2)(12, 12), (_lib.C.c_int * 2)(0, 0), out.data_ptr(), None) == _lib.EINVAL
    st.attention_extend(q, [12, 3], [4, 2], out=out)                                  # the next valid call
    torch.cuda.synchronize()
    assert st.last_attn_kernel == MFMA and (out[0, :4] == SENTINEL).all() and (out[0, 4:] == 0).all() and (out[1, 3:] == SENTINEL).all()
    st.close(); enc.close()


def test_closed_stream_and_closed_encoder_raise():
    enc = _bare(2, 64, "f16", 32)
    st, st2 = enc.open_stream(1, 16), enc.open_stream(1, 16)
    q = torch.zeros(1, 4, 384, dtype=torch.float16, device="cuda")
    st.close()
    for call in (lambda: st.extend_plan(), lambda: st.attention_extend(q, [4], [0])):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    enc.close()
    for call in (lambda: st2.extend_plan(), lambda: st2.attention_extend(q, [4], [0])):
        with pytest.raises(RuntimeError, match="closed"):
            call()
    st2.close()
