"""Every linear and LayerNorm launch of the encoder on the device, one operation at a time (flope_tf_linear, flope_tf_layernorm:
exactly what a forward launches, with the id of the kernel that ran), element by element against fp64 within the derived bounds of
tests/tf_linear_bound.py:

  1. each case asserts the kernel id, finiteness, |got - ref| <= bound at every element, equal bits on a second run, a sentinel
     untouched behind the (padded) output, and NaN in the pad rows of x and res reaching no real row -- first as NaN, then as zeros,
     with equal bits; nothing is provoked: the pad rows are inside the allocation the contract asks for;
  2. tf_linear_f32m with ReLU and with a residual is also the CPU walk of its feed order, bit for bit;
  3. the entry points called in run_forward's order give the forward's bits;
  4. rows M .. Mpad of the handle's buffers, left NaN by an earlier, larger forward, reach no token of a later, smaller one;
  5. what the entry points refuse;
  6. every FLOPE_TF_LIN_* and FLOPE_TF_LN_* id was returned in each dtype that can reach it.
Every case prints its worst err / bound (-s).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import tf_linear_bound as LB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 1234.0                    # exact in f16, bf16 and float32
GUARD = 64                           # rows behind every buffer: NaN behind inputs, the sentinel behind outputs
MAX_TOKENS = {LB.A: 1100, LB.B: 64, LB.C: 33000, LB.D_VEC: 8, LB.D_ROW: 8, LB.D_16: 8, LB.D_16R: 8, LB.F1: 771, LB.F2: 771}
LIN_NAME = {LB.GENERIC: "generic", LB.ROWWAVE: "rowwave", LB.ROWWAVE_VEC: "rowwave_vec", LB.MFMA: "mfma", LB.F32M: "f32m"}
# What ran in this session, for the coverage test at the end of the file.  It depends on the order of the file: under a -k selection,
# a random order or one worker of pytest-xdist, the coverage test finds these partly filled and runs the missing cases itself (by
# calling the test functions), so its assertion holds in any order, at the price of running those cases twice in the session.
_DONE, _SEEN, _WORST = set(), set(), {}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _new(dims, dtype, max_tokens, load=True, **kw):
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens, **kw)
    if load:
        enc.load_state_dict(LB.state_dict(dims))
    return enc


@pytest.fixture(scope="module")
def handles():
    cache = {}

    def get(dims, dtype):
        if (dims, dtype) not in cache:
            cache[(dims, dtype)] = _new(dims, dtype, MAX_TOKENS[dims])
        return cache[(dims, dtype)]

    yield get
    for enc in cache.values():
        enc.close()


def _guarded(t, rows, rpad, fill):
    """t [rows, cols] at the head of a [rpad + GUARD, cols] device tensor whose other rows hold `fill`; -> (whole, view of the rows)"""
    big = torch.full((rpad + GUARD, t.shape[1]), fill, dtype=t.dtype, device="cuda")
    big[:rows] = t.cuda()
    return big, big[:rows]


def _run_linear_case(enc, c, dtype):
    rows, f16h = c["rows"], dtype in ("f16", "bf16")
    rpad = (rows + 127) // 128 * 128 if f16h else rows
    x, r = LB.linear_inputs(c["dims"], c["name"], rows, dtype, c["x_f32"], c["res"])
    ref, bound = LB.case_reference(c, dtype)
    odt = LB.TDT[LB.out_key(c, dtype)]
    xbig, xv = _guarded(x, rows, rpad, float("nan"))
    rbig, rv = _guarded(r, rows, rpad, float("nan")) if r is not None else (None, None)
    obig = torch.full((rpad + GUARD, ref.shape[1]), SENTINEL, dtype=odt, device="cuda")
    enc.set_option("generic", c["generic"])
    try:
        got = enc.linear(c["name"], xv, res=rv, relu=c["relu"], out_f32=c["out_f32"], out=obig[:rows])
        kid = enc.last_linear_kernel
        assert kid == c["kernel"], f"{LIN_NAME.get(kid, kid)} ran where {LIN_NAME[c['kernel']]} was expected"
        torch.cuda.synchronize()
        first = got.clone()
        assert got.data_ptr() == obig.data_ptr()
        assert torch.isfinite(got).all(), "a non-finite output: a pad row of x or res reached a real row, or rows past the input were read"
        # only tf_gemm_mfma may write the pad rows of its last tile; nothing may write behind them
        tail = obig[rpad:] if kid == LB.MFMA else obig[rows:]
        assert (tail == SENTINEL).all(), "a store past the output's rows"
        q, where = LB.ratio(got, ref, bound)
        print(f"{dtype} {LB.case_id(c)} [{LIN_NAME[kid]}]: max err / bound {q:.3f} at {where}")
        assert q <= 1.0
        obig[:rpad] = SENTINEL
        enc.linear(c["name"], xv, res=rv, relu=c["relu"], out_f32=c["out_f32"], out=obig[:rows])
        torch.cuda.synchronize()
        assert torch.equal(_bits(obig[:rows]), _bits(first)), "two runs differ"
        xbig[rows:] = 0.0                                            # other pad rows, the same real rows
        if rbig is not None:
            rbig[rows:] = 0.0
        obig[:rpad] = SENTINEL
        enc.linear(c["name"], xv, res=rv, relu=c["relu"], out_f32=c["out_f32"], out=obig[:rows])
        torch.cuda.synchronize()
        assert torch.equal(_bits(obig[:rows]), _bits(first)), "the pad rows of x / res changed a real row"
    finally:
        enc.set_option("generic", 0)
    _DONE.add((dtype, LB.case_id(c)))
    _SEEN.add(("lin", kid, dtype))
    key = (LIN_NAME[kid], dtype, LB.out_key(c, dtype))
    _WORST[key] = max(_WORST.get(key, 0.0), q)
    return first


def _params():
    out = []
    for dt in ("f16", "bf16", "f32", "f32m"):
        seen = set()
        for c in LB.linear_cases(dt):
            if LB.case_id(c) not in seen:
                seen.add(LB.case_id(c))
                out.append(pytest.param(dt, c, id=dt + "-" + LB.case_id(c)))
    return out


# ---- 1. linears ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,case", _params())
def test_linear_every_element_within_the_bound_of_fp64(handles, dtype, case):
    _run_linear_case(handles(case["dims"], dtype), case, dtype)


# ---- 2. tf_linear_f32m with an epilogue: also the CPU walk, bit for bit --------------------------------------------------------------
@pytest.fixture(scope="module")
def tfh():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_f32m.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_f32m.so"])
    lib = C.CDLL(path)
    lib.tf_f32m_image_floats.restype = C.c_long
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# F2 at 771 rows is the one case with a full grid of 12 row tiles on the throughput shape: the mp choice meets a partly filled tile
WALK = [(LB.F1, 37), (LB.F1, 131), (LB.F1, 771), (LB.F2, 37), (LB.F2, 131), (LB.F2, 771)]


@pytest.mark.parametrize("dims,rows", WALK, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_f32m_relu_and_residual_are_the_host_walk_bit_for_bit(handles, tfh, dims, rows):
    enc = handles(dims, "f32m")
    sd = LB.state_dict(dims)
    for name, relu, res in (("layers.0.linear1", True, False), ("layers.0.linear2", False, True)):
        wk, bk = LB.weight_keys(name)
        x, r = LB.linear_inputs(dims, name, rows, "f32m", False, res)
        got = enc.linear(name, x.cuda(), res=None if r is None else r.cuda(), relu=relu)
        assert enc.last_linear_kernel == LB.F32M
        w, b, xn = sd[wk].numpy(), sd[bk].numpy(), np.ascontiguousarray(x.numpy())
        N, K = w.shape
        img = np.zeros(tfh.tf_f32m_image_floats(N, K), dtype=np.float32)
        tfh.tf_f32m_pack(_ptr(w), N, K, _ptr(img))
        y = np.full((rows, N), np.nan, dtype=np.float32)
        rn = None if r is None else np.ascontiguousarray(r.numpy())
        assert tfh.tf_f32m_walk(_ptr(xn), _ptr(img), _ptr(b), None if rn is None else _ptr(rn), _ptr(y), rows, K, N, int(relu), 2) == 0
        g = got.cpu().numpy()
        assert np.array_equal(g, y), f"{name}: device and host walk differ in {np.count_nonzero(g != y)} of {y.size} elements, max {np.abs(g - y).max():.2e}"


def test_a_float32_view_off_the_16_byte_grid_runs_generic_within_the_bound(handles):
    enc = handles(LB.F1, "f32m")
    for name, relu, res in (("layers.0.linear1", True, False), ("layers.0.linear2", False, True)):
        c = LB._case(LB.F1, name, 37, LB.GENERIC, relu=relu, res=res)
        x, r = LB.linear_inputs(LB.F1, name, 37, "f32m", False, res)
        ref, bound = LB.case_reference(c, "f32m")
        flat = torch.zeros(x.numel() + 8, device="cuda")
        flat[1:1 + x.numel()] = x.reshape(-1).cuda()
        got = enc.linear(name, flat[1:1 + x.numel()].view(37, -1), res=None if r is None else r.cuda(), relu=relu)   # 4 bytes past a 16-byte boundary
        assert enc.last_linear_kernel == LB.GENERIC
        q, where = LB.ratio(got, ref, bound)
        print(f"f32m {name} from a misaligned view [generic]: max err / bound {q:.3f} at {where}")
        assert q <= 1.0
        _SEEN.add(("lin", LB.GENERIC, "f32m"))
        key = (LIN_NAME[LB.GENERIC], "f32m", LB.out_key(c, "f32m"))
        _WORST[key] = max(_WORST.get(key, 0.0), q)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------
def _run_ln(enc, dtype, d):
    worst = 0.0
    for rows in LB.LN_ROWS:
        for fam in LB.LN_FAMILIES:
            x, w, b = LB.ln_inputs(fam, rows, d, dtype)
            ref, bound = LB.ln_reference(x, w, b, dtype)
            xbig, xv = _guarded(x, rows, rows, float("nan"))
            obig = torch.full((rows + GUARD, d), SENTINEL, dtype=x.dtype, device="cuda")
            wg, bg = w.cuda(), b.cuda()
            got = enc.layernorm(xv, wg, bg, out=obig[:rows])
            assert enc.last_ln_kernel == LB.ln_kernel(d, dtype)
            torch.cuda.synchronize()
            first = got.clone()
            assert torch.isfinite(got).all()
            assert (obig[rows:] == SENTINEL).all(), "a store past the last row"
            q, where = LB.ratio(got, ref, bound)
            print(f"{dtype} layernorm d={d} rows={rows} {fam} [{'vec' if enc.last_ln_kernel == LB.LN_VEC else 'scalar'}]: max err / bound {q:.3f} at {where}")
            assert q <= 1.0, (fam, rows, d)
            obig[:rows] = SENTINEL
            enc.layernorm(xv, wg, bg, out=obig[:rows])
            torch.cuda.synchronize()
            assert torch.equal(_bits(obig[:rows]), _bits(first)), "two runs differ"
            worst = max(worst, q)
    _SEEN.add(("ln", enc.last_ln_kernel, dtype))
    key = ("ln_vec" if enc.last_ln_kernel == LB.LN_VEC else "ln_scalar", dtype, dtype)
    _WORST[key] = max(_WORST.get(key, 0.0), worst)
    _DONE.add((dtype, "ln%d" % d))


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("d", LB.LN_DIMS)
def test_layernorm_every_element_within_the_bound_of_fp64(dtype, d):
    enc = _new((16, d, 9, 1, 0, 8), dtype, 8, load=False)           # no layers, no weights: gamma and beta are the caller's
    try:
        _run_ln(enc, dtype, d)
    finally:
        enc.close()


# ---- 3. the entry points in run_forward's order are the forward -------------------------------------------------------------------------
def _compose(enc, x, heads):
    B, L, _ = x.shape
    M = B * L
    sd = LB.state_dict(enc.dims)
    h = enc.linear("embedding", x.reshape(M, -1))
    ids = [enc.last_linear_kernel]
    for i in range(enc.dims[4]):
        p, q = f"layers.{i}.", f"transformer_encoder.layers.{i}."
        qkv = enc.linear(p + "in_proj", h)
        att = enc.attention(qkv.view(B, L, -1)).view(M, -1)
        h2 = enc.linear(p + "out_proj", att, res=h)
        h = enc.layernorm(h2, sd[q + "norm1.weight"].cuda(), sd[q + "norm1.bias"].cuda())
        ff = enc.linear(p + "linear1", h, relu=True)
        h2 = enc.linear(p + "linear2", ff, res=h)
        h = enc.layernorm(h2, sd[q + "norm2.weight"].cuda(), sd[q + "norm2.bias"].cuda())
    return enc.linear("out_layer", h, out_f32=True).view(B, L, -1)


@pytest.mark.parametrize("dims", [LB.A, LB.B], ids=["A", "B"])
@pytest.mark.parametrize("dtype,tiled", [("f16", 0), ("f16", 1), ("bf16", 0), ("bf16", 1), ("f32", 0), ("f32m", 0)])
def test_the_entry_points_in_forward_order_give_the_forward_bits(dims, dtype, tiled):
    enc = _new(dims, dtype, 51, attn_tiled=tiled)
    try:
        for B, L in ((3, 17), (1, 1)):
            x = torch.randn(B, L, dims[0], generator=torch.Generator().manual_seed(B * 100 + L)).cuda()
            y = enc(x)
            z = _compose(enc, x, dims[3])
            torch.cuda.synchronize()
            assert torch.isfinite(y).all()
            diff = int((_bits(y) != _bits(z)).sum())
            print(f"{dtype} attn_tiled={tiled} {dims} B={B} L={L}: {diff} of {y.numel()} elements differ in bits")
            assert diff == 0
    finally:
        enc.close()


# ---- 4. stale pad rows of the handle's own buffers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32m"])
def test_nan_left_in_the_pad_rows_by_a_larger_forward_reaches_no_token(dtype):
    enc, fresh = _new(LB.A, dtype, 256), _new(LB.A, dtype, 256)
    try:
        bad = enc(torch.full((1, 256, LB.A[0]), float("nan"), device="cuda"))
        assert torch.isnan(bad).all()                                   # every buffer of the handle now holds NaN in rows 0 .. 255
        for n in (1, 130):
            x = torch.randn(1, n, LB.A[0], generator=torch.Generator().manual_seed(n)).cuda()
            y, want = enc(x), fresh(x)
            torch.cuda.synchronize()
            assert torch.isfinite(want).all()
            assert torch.equal(_bits(y), _bits(want)), f"{n} tokens behind a 256-token NaN forward differ from a fresh handle"
    finally:
        enc.close()
        fresh.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(handles):
    from flope_amd import _lib
    enc = handles(LB.A, "f16")
    lib, d = enc.lib, LB.A[1]
    x = torch.zeros(128, d, dtype=torch.float16, device="cuda")
    y = torch.full((128, 3 * d), SENTINEL, dtype=torch.float16, device="cuda")
    call = lambda name, xp, yp, rows: lib.flope_tf_linear(enc.handle, name, xp, 0, None, yp, 0, rows, 0, None)
    assert call(b"layers.0.nonsense", x.data_ptr(), y.data_ptr(), 1) == _lib.EINVAL
    assert call(b"layers.1.in_proj", x.data_ptr(), y.data_ptr(), 1) == _lib.EINVAL        # one layer only
    assert call(b"", x.data_ptr(), y.data_ptr(), 1) == _lib.EINVAL
    assert b"unknown linear" in lib.flope_tf_last_error(enc.handle)
    assert call(b"layers.0.in_proj", x.data_ptr(), y.data_ptr(), MAX_TOKENS[LB.A] + 1) == _lib.EINVAL
    assert b"max_tokens" in lib.flope_tf_last_error(enc.handle)
    assert call(b"layers.0.in_proj", x.data_ptr(), y.data_ptr(), 0) == _lib.EINVAL
    with pytest.raises(ValueError, match="unknown linear"):
        enc.linear("layers.0.nonsense", x)
    # a misaligned 16-bit buffer: refused, nothing launched
    flat = torch.zeros(128 * d + 8, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="16-byte"):
        enc.linear("layers.0.in_proj", flat[1:1 + d].view(1, d), out=y[:1])
    with pytest.raises(ValueError, match="16-byte"):
        enc.linear("layers.0.out_proj", x[:1], res=flat[1:1 + d].view(1, d))
    with pytest.raises(ValueError, match="16-byte"):
        enc.layernorm(flat[1:1 + d].view(1, d), torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"), out=x[:1])
    # a float32 input to an MFMA linear other than the embedding has no 16-bit copy to go through
    with pytest.raises(ValueError, match="embedding only"):
        enc.linear("layers.0.in_proj", torch.zeros(1, d, device="cuda"))
    # ... and a 16-bit input to the MFMA embedding (K = 24, read as rows of Kp = 64) has no zero-padded columns: float32 only
    x24 = torch.zeros(128, LB.A[0], dtype=torch.float16, device="cuda")
    assert lib.flope_tf_linear(enc.handle, b"embedding", x24.data_ptr(), 0, None, y.data_ptr(), 0, 1, 0, None) == _lib.EINVAL
    assert b"x_f32" in lib.flope_tf_last_error(enc.handle)
    with pytest.raises(ValueError, match="x_f32"):
        enc.linear("embedding", x24[:1], out=y.view(-1)[:128 * d].view(128, d)[:1])
    with pytest.raises(ValueError, match="max_tokens"):
        enc.layernorm(torch.zeros(MAX_TOKENS[LB.A] + 1, d, dtype=torch.float16, device="cuda"), torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"))
    torch.cuda.synchronize()
    assert (y == SENTINEL).all() and (x == 0).all(), "a refused call wrote something"
    bare = _new(LB.A, "f16", 8, load=False)
    try:
        with pytest.raises(RuntimeError, match="weights not loaded"):
            bare.linear("embedding", torch.zeros(1, LB.A[0], device="cuda"))
    finally:
        bare.close()


# ---- 6. coverage ---------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_id_was_returned_in_every_dtype_that_reaches_it(handles):
    """Runs last; cases that did not run in this session (a -k selection) are run here, so the assertion stands alone."""
    for p in _params():
        dt, c = p.values
        if (dt, LB.case_id(c)) not in _DONE:
            _run_linear_case(handles(c["dims"], dt), c, dt)
    if ("lin", LB.GENERIC, "f32m") not in _SEEN:
        test_a_float32_view_off_the_16_byte_grid_runs_generic_within_the_bound(handles)
    for dt in ("f16", "bf16", "f32"):
        for d in LB.LN_DIMS:
            if (dt, "ln%d" % d) not in _DONE:
                test_layernorm_every_element_within_the_bound_of_fp64(dt, d)
    want = {("lin", k, dt) for dt in ("f16", "bf16") for k in (LB.GENERIC, LB.ROWWAVE, LB.ROWWAVE_VEC, LB.MFMA)}
    want |= {("lin", LB.GENERIC, "f32"), ("lin", LB.ROWWAVE, "f32"), ("lin", LB.F32M, "f32m"), ("lin", LB.GENERIC, "f32m")}
    want |= {("ln", k, dt) for dt in ("f16", "bf16") for k in (LB.LN_VEC, LB.LN_SCALAR)} | {("ln", LB.LN_SCALAR, "f32")}
    assert _SEEN == want, _SEEN ^ want
    for (kernel, dt, out), q in sorted(_WORST.items()):
        print(f"worst err / bound on the device: {kernel:12s} {dt:5s} stored as {out:5s} {q:.3f}")
