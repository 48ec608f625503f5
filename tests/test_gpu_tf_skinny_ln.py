"""Option "skinny_ln" on the device (tf_gemm_skinny_ln, flope_tf_linear_ln / _linear_ln_plan / _last_ln): a LayerNorm that
stands directly in front of a skinny linear of K = model_dim <= 512 runs inside that linear's launch.  The contract is bits: the launch
returns what tf_layernorm_vec followed by tf_gemm_skinny return, so nothing any caller returns changes; 2 num_layers - 1 launches leave
a forward.

Handles: D128 (16, 128, 9, 2, 2, 256), D384 (24, 384, 9, 6, 2, 1536) -- two layers, so the second LayerNorm in front of the next
in_proj is there --, D512 (16, 512, 9, 4, 2, 512) -- the ring full, all 64 LayerNorm lanes taken -- and D640 (16, 640, 9, 5, 1, 640),
which must fall back.

  1. enc.linear_ln alone on layers.0.linear1 (ReLU) and layers.1.in_proj, M in {1, 15, 16, 17, 31, 32}: id 6, `normed` the bits of
     enc.layernorm, `y` the bits of enc.linear on it under skinny = 1; the plan agrees; refused at M = 33, d = 640 and skinny = 0
  2. NaN in the rows >= M of x; a sentinel in both results from row 16 MT on and behind the buffers
  3. against fp64 within tests/tf_linear_bound.py's bounds (implied by 1; kept so the file reads on its own)
  4. through every caller, skinny_ln = 1 against 0 under skinny = 1: step (linear and windowed, step_split, per-head ALiBi), step_assoc,
     extend, prefill, the forward; enc.last_ln on each
  5. what keeps its launches: 40 tracks, skinny = 0, d = 640, a float32 handle; a refused value leaves the handle usable
"""
import numpy as np
import pytest
import torch

import tf_linear_bound as LB

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
GENERIC, MFMA, SKINNY, SKINNY_LN = 0, 3, 5, 6
D128 = (16, 128, 9, 2, 2, 256)
D384 = (24, 384, 9, 6, 2, 1536)
D512 = (16, 512, 9, 4, 2, 512)
D640 = (16, 640, 9, 5, 1, 640)
FOLDING = [D128, D384, D512]
IDS = ["d128", "d384", "d512"]
ROWS = (1, 15, 16, 17, 31, 32)
FORMS = (("layers.0.linear1", True), ("layers.1.in_proj", False))
SENTINEL = 0x5A5A


def _bits16(t):
    return t.contiguous().view(torch.int16)


def _bits32(t):
    return t.contiguous().view(torch.int32)


_ENC = {}


@pytest.fixture(scope="module")
def encoders():
    """(dims, dtype) -> a loaded encoder, made once per module; every test leaves options skinny and skinny_ln at 0"""
    from flope_amd.tf_encoder import TransformerEncoder

    def get(dims, dtype):
        key = (dims, dtype)
        if key not in _ENC:
            enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=256)
            enc.load_state_dict(LB.state_dict(dims))
            _ENC[key] = enc
        return _ENC[key]

    yield get
    for enc in _ENC.values():
        enc.close()
    _ENC.clear()


class _Options:
    def __init__(self, enc, **kw):
        self.enc, self.kw = enc, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.enc.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.enc.set_option(k, 0)


def _inputs(M, d, dtype, family="normal", pad=None):
    """x [M, d] as a view of 128-row storage whose rows >= M hold `pad` (None: zero); gamma, beta float32 [d] far from 1 and 0.
    Row 0 carries a large common offset on top of its family (cancellation in the variance) where there is more than one row."""
    x, w, b = LB.ln_inputs(family, M, d, dtype)
    x = x.clone()
    if M > 1:
        x[0] = (x[0].float() + 60.0).to(x.dtype)
    big = torch.zeros(128, d, dtype=x.dtype, device="cuda")
    if pad is not None:
        big.fill_(pad)
    big[:M] = x.cuda()
    return big[:M], w.cuda(), b.cuda()


def _separate(enc, name, x, w, b, relu):
    """the two launches under skinny = 1 -> (y, normed, ids)"""
    with _Options(enc, skinny=1):
        normed = enc.layernorm(x, w, b)
        y = enc.linear(name, normed, relu=relu)
        return y, normed, (enc.last_ln_kernel, enc.last_linear_kernel)


# ---- 1. the launch alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", FOLDING, ids=IDS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_linear_ln_is_the_two_launches_in_bits(encoders, dtype, dims):
    enc = encoders(dims, dtype)
    d = dims[1]
    bad = []
    for name, relu in FORMS:
        for M in ROWS:
            for family in ("normal", "offset") if M == 31 else ("normal",):
                x, w, b = _inputs(M, d, dtype, family)
                y0, n0, ids = _separate(enc, name, x, w, b, relu)
                with _Options(enc, skinny=1, skinny_ln=1):
                    y1, n1 = enc.linear_ln(name, x, w, b, relu=relu)
                    got = (enc.last_linear_kernel, enc.linear_ln_plan(name, M))
                torch.cuda.synchronize()
                if ids != (LB.LN_VEC, SKINNY) or got != (SKINNY_LN, SKINNY_LN):
                    bad.append((name, M, "ids", ids, got))
                dn, dy = int((_bits16(n0) != _bits16(n1)).sum()), int((_bits16(y0) != _bits16(y1)).sum())
                if dn or dy or not torch.isfinite(y1.float()).all() or not torch.isfinite(n1.float()).all():
                    bad.append((name, M, family, "bits", dn, dy))
    assert not bad, bad[:8]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_where_the_rule_says_no_the_call_is_refused(encoders, dtype):
    """33 rows, model_dim 640 and skinny = 0: ValueError, nothing written, and the plan is the separate form's id"""
    for dims, M, sk, want in ((D384, 33, 1, MFMA), (D640, 8, 1, SKINNY), (D384, 8, 0, MFMA), (D128, 8, 0, MFMA)):
        enc = encoders(dims, dtype)
        d = dims[1]
        x, w, b = _inputs(M, d, dtype)
        for name, relu in (("layers.0.linear1", True), ("layers.0.in_proj", False)):
            N = enc._linear_dims(name)[0]
            yb = torch.full((128 * N,), SENTINEL, dtype=torch.int16, device="cuda").view(TDT[dtype])
            nb = torch.full((128 * d,), SENTINEL, dtype=torch.int16, device="cuda").view(TDT[dtype])
            with _Options(enc, skinny=sk, skinny_ln=1):
                assert enc.linear_ln_plan(name, M) == want == enc.linear_plan(name, M), (dims, M, sk, name)
                with pytest.raises(ValueError):
                    enc.linear_ln(name, x, w, b, relu=relu, out=yb[:M * N].view(M, N), normed=nb[:M * d].view(M, d))
            torch.cuda.synchronize()
            assert bool((yb.view(torch.int16) == SENTINEL).all()) and bool((nb.view(torch.int16) == SENTINEL).all())
    enc = encoders(D384, dtype)
    x, w, b = _inputs(8, 384, dtype)
    with _Options(enc, skinny=1, skinny_ln=1):
        with pytest.raises(ValueError):                                  # x aliases normed
            enc.linear_ln("layers.0.linear1", x, w, b, relu=True, normed=x)
        with pytest.raises(ValueError):                                  # no packed linear: out_layer
            enc.linear_ln("out_layer", x, w, b)
        assert enc.linear_ln_plan("out_layer", 8) == enc.linear_plan("out_layer", 8)
        with pytest.raises(ValueError):                                  # K = ff, not model_dim
            enc.linear_ln("layers.0.linear2", torch.zeros(8, 384, dtype=TDT[dtype], device="cuda"), w, b)
        with pytest.raises(ValueError):
            enc.linear_ln_plan("layers.0.linear1", 0)
        with pytest.raises(ValueError):
            enc.linear_ln_plan("layers.7.linear1", 4)
    with _Options(enc, skinny=1, skinny_ln=1, generic=1):                # option generic wins, as it does over skinny
        assert enc.linear_ln_plan("layers.0.linear1", 8) == GENERIC


# ---- 2. padding --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", FOLDING, ids=IDS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_nan_in_the_pad_rows_reaches_no_row(encoders, dtype, dims):
    enc = encoders(dims, dtype)
    d = dims[1]
    for name, relu in FORMS:
        for M in (1, 15, 17, 31):
            clean, w, b = _inputs(M, d, dtype)
            x, _, _ = _inputs(M, d, dtype, pad=float("nan"))
            y0, n0, _ = _separate(enc, name, clean, w, b, relu)
            with _Options(enc, skinny=1, skinny_ln=1):
                y1, n1 = enc.linear_ln(name, x, w, b, relu=relu)
            torch.cuda.synchronize()
            assert torch.isfinite(y1.float()).all() and torch.isfinite(n1.float()).all(), (name, M)
            assert torch.equal(_bits16(y1), _bits16(y0)) and torch.equal(_bits16(n1), _bits16(n0)), (name, M)


@pytest.mark.parametrize("dims", FOLDING, ids=IDS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rows_from_16_mt_on_are_not_written(encoders, dtype, dims):
    """a sentinel in normed and y from row 16 MT to row 127 and for 64 rows behind each buffer is intact"""
    enc = encoders(dims, dtype)
    d = dims[1]
    for name, relu in FORMS:
        N = enc._linear_dims(name)[0]
        for M in (1, 16, 17, 32):
            x, w, b = _inputs(M, d, dtype)
            yb = torch.full(((128 + 64) * N,), SENTINEL, dtype=torch.int16, device="cuda").view(TDT[dtype])
            nb = torch.full(((128 + 64) * d,), SENTINEL, dtype=torch.int16, device="cuda").view(TDT[dtype])
            with _Options(enc, skinny=1, skinny_ln=1):
                y, n = enc.linear_ln(name, x, w, b, relu=relu, out=yb[:M * N].view(M, N), normed=nb[:M * d].view(M, d))
            torch.cuda.synchronize()
            assert y.data_ptr() == yb.data_ptr() and n.data_ptr() == nb.data_ptr()
            first = 16 * (1 if M <= 16 else 2)
            for buf, cols in ((yb, N), (nb, d)):
                tail = buf.view(torch.int16)[first * cols:]
                assert bool((tail == SENTINEL).all()), (name, M, cols, int((tail != SENTINEL).sum()))
            assert torch.isfinite(y.float()).all() and torch.isfinite(n.float()).all()


# ---- 3. against fp64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", FOLDING, ids=IDS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rows_within_the_bounds_of_fp64(encoders, dtype, dims):
    """normed against LayerNorm in fp64 of the stored x; y against the linear in fp64 of the device's own normed"""
    enc = encoders(dims, dtype)
    d = dims[1]
    sd = LB.state_dict(dims)
    for name, relu in FORMS:
        for family in ("normal", "offset", "outlier"):
            x, w, b = _inputs(31, d, dtype, family)
            with _Options(enc, skinny=1, skinny_ln=1):
                y, n = enc.linear_ln(name, x, w, b, relu=relu)
            torch.cuda.synchronize()
            ref, bound = LB.ln_reference(x.cpu(), w.cpu(), b.cpu(), dtype)
            rn, where_n = LB.ratio(n, ref, bound)
            wk, bk = LB.weight_keys(name)
            ref, bound = LB.linear_reference(n.cpu(), LB.kernel_weight(sd[wk], dtype, MFMA), sd[bk], None, relu, dtype)
            ry, where_y = LB.ratio(y, ref, bound)
            print(f"{dtype} d{d} {name} {family}: normed {rn:.3f} at {where_n}, y {ry:.3f} at {where_y} (max |got - fp64| / bound)")
            assert rn <= 1.0 and ry <= 1.0, (name, family, rn, ry)


# ---- 4. through every caller -------------------------------------------------------------------------------------------------------------
def _both(enc, fn):
    """fn() under skinny_ln = 0 and 1, both with skinny = 1 -> the two results and the two last_ln"""
    res, lns = [], []
    for v in (0, 1):
        with _Options(enc, skinny=1, skinny_ln=v):
            res.append(fn())
            lns.append(enc.last_ln)
    torch.cuda.synchronize()
    return res[0], res[1], lns


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(_bits32(a), _bits32(b)) and bool(torch.isfinite(a).all())
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    return a == b


def _counts(dims):
    nl = dims[4]
    return [(2 * nl, 0), (1, 2 * nl - 1)]


@pytest.mark.parametrize("n", [1, 5, 31])
@pytest.mark.parametrize("dims", [D128, D384], ids=["d128", "d384"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_host_positioned_stream_steps(encoders, dtype, dims, n):
    """6 steps, the positions, 4 further steps that read the cache the first 6 left: linear and with window = 4 (a ring of 4 that wraps),
    with and without step_split and per-head ALiBi"""
    from flope_amd.tf_encoder import alibi_distances
    enc = encoders(dims, dtype)
    x = torch.randn(n, 10, dims[0], generator=torch.Generator().manual_seed(40 + n)).cuda()
    slopes = [2.0 ** -(h + 1) for h in range(dims[3])]
    for window in (0, 4):
        for split, alibi in ((0, False), (1, False), (0, True), (1, True)):
            def walk():
                table = alibi_distances(window if window else 10, slopes) if alibi else None
                st = enc.open_stream(n, window if window else 10, window=window, bias=table)
                first = torch.stack([st.step(x[:, t].contiguous()) for t in range(6)])
                pos = st.positions
                more = torch.stack([st.step(x[:, t].contiguous()) for t in range(6, 10)])
                end = st.positions
                st.close()
                return first, pos, more, end
            with _Options(enc, step_split=split):
                a, b, lns = _both(enc, walk)
            assert _same(a, b), (window, split, alibi)
            assert lns == _counts(dims), (lns, window, split, alibi)
            assert a[1] == [6] * n and a[3] == [10] * n


@pytest.mark.parametrize("dims", [D128, D512], ids=["d128", "d512"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_device_positioned_stream_step_assoc(encoders, dtype, dims):
    """frames whose rows match, open, repeat a track, name a track out of range or are skipped: rows that feed nothing included"""
    enc = encoders(dims, dtype)
    skip = -2 ** 31

    def o(t):
        return -1 - t
    frames = [[o(0), o(1), o(0), 7, skip], [1, 1, 0, 0, o(6)], [0, skip, 0, 1, 1, 6], [o(2), 0, 1, 9, 2, o(3), 3]] * 2 + [[0, 1], [3]]
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(len(f), dims[0], generator=g).cuda() for f in frames]

    def walk():
        st = enc.open_stream(6, 4, window=4, positions="device", max_rows=8)
        ys, feeds = [], []
        for x, f in zip(xs, frames):
            ys.append(st.step_assoc(x, torch.tensor(f, dtype=torch.int32, device="cuda")).clone())
            feeds.append(st.last_feed())
        pos = st.positions
        more = [st.step_assoc(x, torch.tensor(f, dtype=torch.int32, device="cuda")).clone() for x, f in list(zip(xs, frames))[1:5]]
        end = st.positions
        st.close()
        return ys, feeds, pos, more, end
    a, b, lns = _both(enc, walk)
    assert _same(a, b)
    assert lns == _counts(dims), lns
    assert max(a[2]) > 4 and any((f[0] < 0).any() for f in a[1])        # the ring wrapped; some rows fed nothing


@pytest.mark.parametrize("dims", FOLDING, ids=IDS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_extend_prefill_and_forward(encoders, dtype, dims):
    enc = encoders(dims, dtype)
    g = torch.Generator().manual_seed(5)
    xe = torch.randn(5, 6, dims[0], generator=g).cuda()                # extend: n L = 30 packed rows
    xp = torch.randn(4, 8, dims[0], generator=g).cuda()                # prefill: 8 + 7 + 8 + 5 = 28 packed rows
    xf = torch.randn(2, 16, dims[0], generator=g).cuda()               # forward: B L = 32
    xn = torch.randn(5, 4, dims[0], generator=g).cuda()
    seen = {}

    def extend():
        st = enc.open_stream(5, 10)
        y = st.extend(xe).clone()
        seen["extend"] = enc.last_ln
        pos = st.positions
        more = torch.stack([st.step(xn[:, t].contiguous()) for t in range(4)])
        st.close()
        return y, pos, more

    def prefill():
        st = enc.open_stream(4, 12)
        y = st.prefill(xp, lengths=[8, 7, 8, 5]).clone()
        seen["prefill"] = enc.last_ln
        pos = st.positions
        more = torch.stack([st.step(xn[:4, t].contiguous()) for t in range(4)])
        st.close()
        return y, pos, more

    for fn in (extend, prefill, lambda: enc(xf).clone(), lambda: enc(xf, is_causal=True).clone()):
        a, b, lns = _both(enc, fn)
        assert _same(a, b)
        assert lns == _counts(dims), lns
    assert seen == {"extend": _counts(dims)[1], "prefill": _counts(dims)[1]}      # (the last pass was under skinny_ln = 1)
    a, _, _ = _both(enc, extend)
    assert a[1] == [6] * 5
    a, _, _ = _both(enc, prefill)
    assert a[1] == [8, 7, 8, 5]


# ---- 5. what keeps its launches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_40_tracks_skinny_off_and_d640_keep_their_launches(encoders, dtype):
    def steps(enc, dims, n):
        x = torch.randn(n, 3, dims[0], generator=torch.Generator().manual_seed(7)).cuda()

        def walk():
            st = enc.open_stream(n, 4)
            y = torch.stack([st.step(x[:, t].contiguous()) for t in range(3)])
            st.close()
            return y
        return walk

    enc = encoders(D128, dtype)
    a, b, lns = _both(enc, steps(enc, D128, 40))                       # more than 32 rows
    assert _same(a, b) and lns == [(4, 0), (4, 0)], lns
    with _Options(enc, skinny=0, skinny_ln=1):                          # stored and ignored without skinny
        y = steps(enc, D128, 5)()
        assert enc.last_ln == (4, 0)
    with _Options(enc, skinny=1, skinny_ln=1):
        y1 = steps(enc, D128, 5)()
        assert enc.last_ln == (1, 3)
    torch.cuda.synchronize()
    assert _same(y, y1)
    enc = encoders(D640, dtype)                                         # more than one LayerNorm vector per lane
    a, b, lns = _both(enc, steps(enc, D640, 5))
    assert _same(a, b) and lns == [(2, 0), (2, 0)], lns


def test_a_float32_handle_stores_and_ignores_it():
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*D128, dtype="f32", max_tokens=64, skinny=1, skinny_ln=1)
    enc.load_state_dict(LB.state_dict(D128))
    assert enc.set_option("skinny_ln", 0) == 1 and enc.set_option("skinny_ln", 1) == 0      # stored: the old value comes back
    x = torch.randn(2, 8, D128[0], generator=torch.Generator().manual_seed(2)).cuda()
    got = {}
    for v in (0, 1):
        enc.set_option("skinny_ln", v)
        got[v] = enc(x).clone()
        assert enc.last_ln == (4, 0)
    torch.cuda.synchronize()
    assert _same(got[0], got[1])
    assert enc.linear_ln_plan("layers.0.linear1", 8) == GENERIC
    with pytest.raises(ValueError):
        enc.linear_ln("layers.0.linear1", torch.zeros(8, 128, device="cuda"), torch.ones(128, device="cuda"), torch.zeros(128, device="cuda"))
    enc.close()


def test_a_refused_value_leaves_the_handle_usable(encoders):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = encoders(D128, "f16")
    x, w, b = _inputs(8, 128, "f16")
    with _Options(enc, skinny=1, skinny_ln=1):
        for v in (2, -1):
            with pytest.raises(ValueError):
                enc.set_option("skinny_ln", v)
        y1, n1 = enc.linear_ln("layers.0.linear1", x, w, b, relu=True)
        assert enc.last_linear_kernel == SKINNY_LN                      # the refused values moved nothing
        assert enc.set_option("skinny_ln", 0) == 1
    y0, n0, _ = _separate(enc, "layers.0.linear1", x, w, b, True)
    torch.cuda.synchronize()
    assert torch.equal(_bits16(y0), _bits16(y1)) and torch.equal(_bits16(n0), _bits16(n1))
    with pytest.raises(ValueError):
        TransformerEncoder(*D128, dtype="f16", max_tokens=64, skinny=1, skinny_ln=2)
    made = TransformerEncoder(*D128, dtype="f16", max_tokens=64, skinny=1, skinny_ln=1)
    made.load_state_dict(LB.state_dict(D128))
    assert made.linear_ln_plan("layers.0.linear1", 8) == SKINNY_LN and made.last_ln == (0, 0)
    made.close()
