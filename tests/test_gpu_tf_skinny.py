"""Option "skinny" on the device (tf_gemm_skinny, flope_tf_linear_plan): a 16-bit MFMA linear of 1 .. 32 rows with one wave
per 16-row feature tile of tf_gemm_mfma's packed image.  The contract is bits: each output element takes the same MFMAs over the same
operands in the same order as in tf_gemm_mfma, so nothing any caller returns changes.

Handles: WIDE (16, 128, 9, 2, 2, 256) -- packed linears of N = 384, 128, 256 and K = 64 (the padded embedding), 128, 256 -- and CFG1,
cfg5's layer (d 384, 6 heads, ff 1536) once: K = 384 and K = 1536 (24 chunks: the prefetch ring of 8 wraps three times).

  1. every packed linear alone, M in {1, 15, 16, 17, 31, 32}: id 5, the bits of id 3; M = 33 and 128: id 3; linear_plan agrees
  2. NaN in the pad rows of x and the residual; a sentinel in y from row 16 MT on and behind the buffer
  3. against fp64 within tests/tf_linear_bound.py's bound at M = 31 (implied by 1; kept so the file reads on its own)
  4. through every caller: step (linear and windowed, step_split, per-head ALiBi), step_assoc, extend, prefill, the forward
  5. float32 handles store and ignore it; a refused value leaves the handle usable
"""
import numpy as np
import pytest
import torch

import tf_linear_bound as LB

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
GENERIC, ROWWAVE, ROWWAVE_VEC, MFMA, F32M, SKINNY = 0, 1, 2, 3, 4, 5
WIDE = (16, 128, 9, 2, 2, 256)
CFG1 = (24, 384, 9, 6, 1, 1536)
ROWS = (1, 15, 16, 17, 31, 32)
ROWS_FALLBACK = (33, 128)
SENTINEL = 0x5A5A


def _forms(dims):
    """(name, relu, res, x_f32) of every packed linear in the form the forward runs it"""
    out = [("embedding", False, False, True)]
    for i in range(dims[4]):
        out += [(f"layers.{i}.in_proj", False, False, False), (f"layers.{i}.out_proj", False, True, False),
                (f"layers.{i}.linear1", True, False, False), (f"layers.{i}.linear2", False, True, False)]
    return out


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _bits32(t):
    return t.contiguous().view(torch.int32)


_ENC = {}


@pytest.fixture(scope="module")
def encoders():
    """(dims, dtype) -> a loaded encoder, made once per module; every test leaves option skinny at 0"""
    from flope_amd.tf_encoder import TransformerEncoder

    def get(dims, dtype, **kw):
        key = (dims, dtype, tuple(sorted(kw.items())))
        if key not in _ENC:
            enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=256, **kw)
            enc.load_state_dict(LB.state_dict(dims))
            _ENC[key] = enc
        return _ENC[key]

    yield get
    for enc in _ENC.values():
        enc.close()
    _ENC.clear()


def _inputs(dims, name, M, dtype, x_f32, res, pad=None):
    """x [M, K] and r [M, N] or None as views of 128-row storage whose rows >= M hold `pad` (None: zero)"""
    x, r = LB.linear_inputs(dims, name, M, dtype, x_f32, res)

    def room(t):
        if t is None:
            return None
        big = torch.zeros(128, t.shape[1], dtype=t.dtype, device="cuda")
        if pad is not None:
            big.fill_(pad)
        big[:M] = t.cuda()
        return big[:M]
    return room(x), room(r)


def _run(enc, skinny, name, x, r, relu, out=None):
    enc.set_option("skinny", skinny)
    try:
        y = enc.linear(name, x, res=r, relu=relu, out=out)
        plan = enc.linear_plan(name, x.shape[0])
        return y, enc.last_linear_kernel, plan
    finally:
        enc.set_option("skinny", 0)


# ---- 1. the linears alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [WIDE, CFG1], ids=["wide", "cfg1"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_linears_alone_are_tf_gemm_mfma_in_bits(encoders, dtype, dims):
    enc = encoders(dims, dtype)
    bad = []
    for name, relu, res, x_f32 in _forms(dims):
        for M in ROWS + ROWS_FALLBACK:
            x, r = _inputs(dims, name, M, dtype, x_f32, res)
            y0, k0, p0 = _run(enc, 0, name, x, r, relu)
            y0 = y0.clone()
            y1, k1, p1 = _run(enc, 1, name, x, r, relu)
            torch.cuda.synchronize()
            want = SKINNY if M <= 32 else MFMA
            if (k0, p0, k1, p1) != (MFMA, MFMA, want, want):
                bad.append((name, M, "ids", k0, p0, k1, p1))
            diff = int((_bits16(y0) != _bits16(y1)).sum())
            if diff or not torch.isfinite(y1.float()).all():
                bad.append((name, M, "bits", diff))
    assert not bad, bad[:8]
    # out_layer is no MFMA linear (N = 9, a float32 result): the option leaves it alone
    x = torch.randn(5, dims[1], generator=torch.Generator().manual_seed(1)).to(TDT[dtype]).cuda()
    for sk in (0, 1):
        enc.set_option("skinny", sk)
        enc.linear("out_layer", x, out_f32=True)
        assert enc.last_linear_kernel == ROWWAVE_VEC and enc.linear_plan("out_layer", 5) == ROWWAVE_VEC
    enc.set_option("skinny", 0)
    # option generic wins, as it does over tf_gemm_mfma
    enc.set_option("generic", 1)
    enc.set_option("skinny", 1)
    assert enc.linear_plan("layers.0.in_proj", 8) == GENERIC
    enc.set_option("generic", 0)
    enc.set_option("skinny", 0)
    with pytest.raises(ValueError):
        enc.linear_plan("layers.0.in_proj", 0)
    with pytest.raises(ValueError):
        enc.linear_plan("layers.0.in_proj", 257)                     # above max_tokens, as linear refuses it
    with pytest.raises(ValueError):
        enc.linear_plan("layers.9.in_proj", 4)


# ---- 2. padding ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_nan_in_the_pad_rows_reaches_no_row(encoders, dtype):
    for dims in (WIDE, CFG1):
        enc = encoders(dims, dtype)
        for name, relu, res, x_f32 in _forms(dims):
            for M in (1, 15, 17, 31):
                if x_f32:
                    # the embedding reads the handle's own 16-bit copy, of which tf_cast_pad writes M rows: 32 rows of NaN first
                    nan32 = torch.full((32, dims[0]), float("nan"), device="cuda")
                    _run(enc, 1, name, nan32, None, relu)
                clean_x, clean_r = _inputs(dims, name, M, dtype, x_f32, res)
                x, r = _inputs(dims, name, M, dtype, x_f32, res, pad=None if x_f32 else float("nan"))
                if r is not None:
                    r = _inputs(dims, name, M, dtype, x_f32, res, pad=float("nan"))[1]
                want, k0, _ = _run(enc, 0, name, clean_x, clean_r, relu)
                want = want.clone()
                got, k1, _ = _run(enc, 1, name, x, r, relu)
                torch.cuda.synchronize()
                assert (k0, k1) == (MFMA, SKINNY)
                assert torch.isfinite(got.float()).all(), (name, M)
                assert torch.equal(_bits16(got), _bits16(want)), (name, M)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rows_from_16_mt_on_are_not_written(encoders, dtype):
    """a sentinel in y from row 16 MT to row 127 and for 64 rows behind the buffer is intact (tf_gemm_mfma overwrites rows < 128)"""
    for dims in (WIDE, CFG1):
        enc = encoders(dims, dtype)
        for name, relu, res, x_f32 in _forms(dims):
            N = enc._linear_dims(name)[0]
            for M in (1, 16, 17, 32):
                x, r = _inputs(dims, name, M, dtype, x_f32, res)
                buf = torch.full(((128 + 64) * N,), SENTINEL, dtype=torch.int16, device="cuda").view(TDT[dtype])
                out = buf[:M * N].view(M, N)
                y, k, _ = _run(enc, 1, name, x, r, relu, out=out)
                torch.cuda.synchronize()
                assert k == SKINNY and y.data_ptr() == buf.data_ptr()
                first = 16 * (1 if M <= 16 else 2)
                tail = buf.view(torch.int16)[first * N:]
                assert bool((tail == SENTINEL).all()), (name, M, int((tail != SENTINEL).sum()))
                assert torch.isfinite(y.float()).all()


# ---- 3. against fp64 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [WIDE, CFG1], ids=["wide", "cfg1"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rows_within_the_bound_of_fp64(encoders, dtype, dims):
    enc = encoders(dims, dtype)
    worst = 0.0
    for name, relu, res, x_f32 in _forms(dims):
        c = LB._case(dims, name, 31, MFMA, relu=relu, res=res, x_f32=x_f32)      # MFMA: the weight rounded once to the handle's type
        ref, bound = LB.case_reference(c, dtype)
        x, r = _inputs(dims, name, 31, dtype, x_f32, res)
        y, k, _ = _run(enc, 1, name, x, r, relu)
        torch.cuda.synchronize()
        assert k == SKINNY
        ratio, where = LB.ratio(y, ref, bound)
        print(f"{dtype} {LB.case_id(c)}: max |y - fp64| / bound = {ratio:.3f} at {where}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio, where)
    print(f"{dtype}: worst {worst:.3f}")


# ---- 4. through every caller -------------------------------------------------------------------------------------------------------------------
def _both(enc, fn):
    """fn() under skinny = 0 and skinny = 1 -> the two results"""
    res = []
    for sk in (0, 1):
        enc.set_option("skinny", sk)
        try:
            res.append(fn())
        finally:
            enc.set_option("skinny", 0)
    torch.cuda.synchronize()
    return res


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(_bits32(a), _bits32(b)) and bool(torch.isfinite(a).all())
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    return a == b


@pytest.mark.parametrize("n", [1, 5, 31])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_host_positioned_stream_steps(encoders, dtype, n):
    """6 steps, the positions, 4 further steps that read the cache the first 6 left: linear and with window = 4 (a ring of 4 that wraps),
    with and without step_split and per-head ALiBi"""
    from flope_amd.tf_encoder import alibi_distances
    enc = encoders(WIDE, dtype)
    x = torch.randn(n, 10, WIDE[0], generator=torch.Generator().manual_seed(40 + n)).cuda()
    for M in (1, 5, 31):
        enc.set_option("skinny", 1)
        assert enc.linear_plan("layers.1.linear2", M) == SKINNY
        enc.set_option("skinny", 0)
    for window in (0, 4):
        for split, alibi in ((0, False), (1, False), (0, True), (1, True)):
            def walk():
                table = alibi_distances(window if window else 10, [0.5, 0.0625]) if alibi else None
                st = enc.open_stream(n, window if window else 10, window=window, bias=table)
                first = torch.stack([st.step(x[:, t].contiguous()) for t in range(6)])
                pos = st.positions
                more = torch.stack([st.step(x[:, t].contiguous()) for t in range(6, 10)])
                end = st.positions
                st.close()
                return first, pos, more, end
            enc.set_option("step_split", split)
            try:
                a, b = _both(enc, walk)
            finally:
                enc.set_option("step_split", 0)
            assert _same(a, b), (window, split, alibi)
            assert a[1] == [6] * n and a[3] == [10] * n


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_a_step_of_40_tracks_falls_back(encoders, dtype):
    enc = encoders(WIDE, dtype)
    x = torch.randn(40, 3, WIDE[0], generator=torch.Generator().manual_seed(7)).cuda()
    enc.set_option("skinny", 1)
    assert enc.linear_plan("layers.0.in_proj", 40) == MFMA and enc.linear_plan("embedding", 40) == MFMA
    enc.set_option("skinny", 0)

    def walk():
        st = enc.open_stream(40, 4)
        y = torch.stack([st.step(x[:, t].contiguous()) for t in range(3)])
        st.close()
        return y
    a, b = _both(enc, walk)
    assert _same(a, b)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_device_positioned_stream_step_assoc(encoders, dtype):
    """frames whose rows match, open, repeat a track, name a track out of range or are skipped: rows that feed nothing included"""
    enc = encoders(WIDE, dtype)
    skip = -2 ** 31

    def o(t):
        return -1 - t
    frames = [[o(0), o(1), o(0), 7, skip], [1, 1, 0, 0, o(6)], [0, skip, 0, 1, 1, 6], [o(2), 0, 1, 9, 2, o(3), 3]] * 2 + [[0, 1], [3]]
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(len(f), WIDE[0], generator=g).cuda() for f in frames]

    def walk():
        st = enc.open_stream(6, 4, window=4, positions="device", max_rows=8)
        ys, feeds = [], []
        for x, f in zip(xs, frames):
            ys.append(st.step_assoc(x, torch.tensor(f, dtype=torch.int32, device="cuda")).clone())
            feeds.append(st.last_feed())
        pos = st.positions
        st.close()
        return ys, feeds, pos
    a, b = _both(enc, walk)
    assert _same(a, b)
    assert max(a[2]) > 4 and any((f[0] < 0).any() for f in a[1])        # the ring wrapped; some rows fed nothing


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_extend_prefill_and_forward(encoders, dtype):
    enc = encoders(WIDE, dtype)
    g = torch.Generator().manual_seed(5)
    xe = torch.randn(5, 6, WIDE[0], generator=g).cuda()                # extend: n L = 30 packed rows
    xp = torch.randn(4, 8, WIDE[0], generator=g).cuda()                # prefill: 8 + 7 + 8 + 5 = 28 packed rows
    xf = torch.randn(2, 16, WIDE[0], generator=g).cuda()               # forward: B L = 32
    xn = torch.randn(5, 4, WIDE[0], generator=g).cuda()
    enc.set_option("skinny", 1)
    assert [enc.linear_plan("layers.0.linear1", M) for M in (30, 28, 32)] == [SKINNY] * 3
    enc.set_option("skinny", 0)

    def extend():
        st = enc.open_stream(5, 10)
        y = st.extend(xe).clone()
        pos = st.positions
        more = torch.stack([st.step(xn[:, t].contiguous()) for t in range(4)])
        st.close()
        return y, pos, more

    def prefill():
        st = enc.open_stream(4, 12)
        y = st.prefill(xp, lengths=[8, 7, 8, 5]).clone()
        pos = st.positions
        more = torch.stack([st.step(xn[:4, t].contiguous()) for t in range(4)])
        st.close()
        return y, pos, more

    for fn in (extend, prefill, lambda: enc(xf).clone(), lambda: enc(xf, is_causal=True).clone()):
        a, b = _both(enc, fn)
        assert _same(a, b)
    assert _both(enc, extend)[0][1] == [6] * 5 and _both(enc, prefill)[0][1] == [8, 7, 8, 5]


# ---- 5. modes that ignore it -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kernel", [("f32", GENERIC), ("f32m", F32M)])
def test_float32_handles_store_and_ignore_it(dtype, kernel):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*WIDE, dtype=dtype, max_tokens=64, skinny=1)
    enc.load_state_dict(LB.state_dict(WIDE))
    assert enc.set_option("skinny", 0) == 1 and enc.set_option("skinny", 1) == 0      # stored: the old value comes back
    x = torch.randn(16, WIDE[1], generator=torch.Generator().manual_seed(2)).cuda()
    r = torch.randn(16, WIDE[1], generator=torch.Generator().manual_seed(3)).cuda()
    got = {}
    for sk in (0, 1):
        enc.set_option("skinny", sk)
        ys = []
        for name, relu, res in (("layers.0.in_proj", False, None), ("layers.0.out_proj", False, r), ("layers.0.linear1", True, None)):
            ys.append(enc.linear(name, x, res=res, relu=relu).clone())
            assert enc.last_linear_kernel == kernel and enc.linear_plan(name, 16) == kernel
        got[sk] = ys
    torch.cuda.synchronize()
    assert _same(got[0], got[1])
    enc.close()


def test_a_refused_value_leaves_the_handle_usable(encoders):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = encoders(WIDE, "f16")
    x, _ = _inputs(WIDE, "layers.0.in_proj", 8, "f16", False, False)
    enc.set_option("skinny", 1)
    for v in (2, -1):
        with pytest.raises(ValueError):
            enc.set_option("skinny", v)
    y1 = enc.linear("layers.0.in_proj", x).clone()
    assert enc.last_linear_kernel == SKINNY                             # the refused values moved nothing
    assert enc.set_option("skinny", 0) == 1
    y0 = enc.linear("layers.0.in_proj", x)
    assert enc.last_linear_kernel == MFMA and torch.equal(_bits16(y0), _bits16(y1))
    with pytest.raises(ValueError):
        TransformerEncoder(*WIDE, dtype="f16", max_tokens=64, skinny=2)
    made = TransformerEncoder(*WIDE, dtype="f16", max_tokens=64, skinny=1)
    made.load_state_dict(LB.state_dict(WIDE))
    assert made.linear_plan("layers.0.in_proj", 8) == SKINNY
    made.close()
