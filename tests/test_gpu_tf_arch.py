"""The encoder's architectures on the device (norm_first, activation="gelu", final_norm).

  1. constructor and options: the keywords, refused values, FLOPE_ESTATE after load, a missing or unexpected transformer_encoder.norm.*
  2. one GELU linear alone: layers.0.linear1 with act="gelu" at rows {1, 127, 128, 129} in f32, f32m, f16, bf16 and with generic = 1: the
     kernel id relu=True gives, every element within tests/tf_act_bound.py's bound of fp64 (the worst ratio printed), NaN pad rows reach
     no row < M, GELU + residual refused with nothing written
  3. bit contracts: skinny = 1 gives tf_gemm_mfma's GELU bits at rows {1, 15, 16, 17, 31, 32}; linear_ln_act(act="gelu") gives the bits of
     layernorm followed by linear; the default architecture's forward is the forward of a handle built without the keywords
  4. whole forwards of the seven non-default architectures against the fp64 fixture (torch's own modules), (B, L) = (5, 50) and (2, 33),
     four dtypes, at the tolerances of tests/test_gpu_tf_encoder.py
  5. the contracts that must survive, for pre-norm + GELU + final norm: the causal prefix, ragged rows, an all-clear compiled mask, a
     stream's step / extend / prefill against the causal forward, skinny / skinny_ln against the options off with enc.last_ln, fused = 1
"""
import numpy as np
import pytest
import torch

import tf_act_bound as AB
import tf_arch_cases as AC
import tf_linear_bound as LB

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f32m": torch.float32}
DTYPES = ["f32", "f32m", "f16", "bf16"]
GENERIC, MFMA, SKINNY, SKINNY_LN = 0, 3, 5, 6
DA, DB = AC.SHAPES["a"], AC.SHAPES["b"]
DG = (16, 192, 5, 3, 1, 320)                                             # N = 320 is no multiple of 128: the generic linears on 16-bit handles
FULL = {"norm_first": True, "activation": "gelu", "final_norm": True}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b)) and bool(torch.isfinite(a.float()).all())


_ENC = {}


def _sd(dims, final_norm):
    if dims in AC.SHAPES.values():
        return AC.state_dict(dims, final_norm)
    sd = dict(LB.state_dict(dims))
    if final_norm:
        sd.update({k: v for k, v in AC.state_dict((dims[0], dims[1], dims[2], dims[3], 0, dims[5]), True).items() if ".norm." in k})
    return sd


def _enc(dims, dtype, arch=None, **kw):
    from flope_amd.tf_encoder import TransformerEncoder
    arch = dict(arch or {})
    key = (dims, dtype, tuple(sorted(arch.items())), tuple(sorted(kw.items())))
    if key not in _ENC:
        enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=256, **arch, **kw)
        enc.load_state_dict(_sd(dims, arch.get("final_norm", False)))
        _ENC[key] = enc
    return _ENC[key]


@pytest.fixture(scope="module")
def FX():
    return np.load(AC.FIXTURE)


# ---- 1. constructor and options ------------------------------------------------------------------------------------------------------------
def test_constructor_options_and_state_dict():
    from flope_amd.tf_encoder import TransformerEncoder
    enc = TransformerEncoder(*DA, dtype="f32", max_tokens=64, **FULL)
    assert enc.arch == FULL
    for name, bad in (("norm_first", 2), ("norm_first", -1), ("activation", 0), ("activation", 3), ("final_norm", 2)):
        with pytest.raises(ValueError):
            enc.set_option(name, bad)
    assert enc.set_option("norm_first", 1) == 1 and enc.set_option("activation", 2) == 2 and enc.set_option("final_norm", 1) == 1    # the old values
    sd = AC.state_dict(DA, True)
    with pytest.raises(KeyError):                                        # final_norm=True needs the norm
        enc.load_state_dict(AC.state_dict(DA, False))
    enc.load_state_dict(sd)
    for name, v in (("norm_first", 0), ("activation", 1), ("final_norm", 0), ("norm_first", 1)):
        with pytest.raises(RuntimeError, match="-3"):                    # FLOPE_ESTATE: fixed once the weights are loaded
            enc.set_option(name, v)
    with pytest.raises(ValueError):                                      # ... and a refused value is still the caller's argument
        enc.set_option("activation", 7)
    x = torch.randn(2, 5, DA[0], generator=torch.Generator().manual_seed(1)).cuda()
    y = enc(x)
    assert torch.isfinite(y).all() and _same(y, _enc(DA, "f32", FULL)(x))
    plain = TransformerEncoder(*DA, dtype="f32", max_tokens=64)
    assert plain.arch == {"norm_first": False, "activation": "relu", "final_norm": False}
    with pytest.raises(ValueError, match="transformer_encoder.norm.weight"):     # a trained norm is never dropped silently
        plain.load_state_dict(sd)
    plain.load_state_dict(AC.state_dict(DA, False))
    assert plain.linear_plan("layers.0.linear1", 4) == enc.linear_plan("layers.0.linear1", 4)
    enc.close()
    plain.close()


# ---- 2. one GELU linear alone --------------------------------------------------------------------------------------------------------------
def _x_with_nan_pad(x, dtype):
    """x [M, K] at the head of storage of roundup(M, 128) rows whose pad rows are NaN (16-bit handles read whole tiles)"""
    M, K = x.shape
    if dtype in ("f32", "f32m"):
        return x.cuda()
    rp = (M + 127) // 128 * 128
    big = torch.full((rp, K), float("nan"), dtype=x.dtype, device="cuda")
    big[:M] = x.cuda()
    return big[:M]


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("dims", [DA, DB, DG], ids=["a", "b", "g"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_linear_alone_within_the_bound(dtype, dims, generic):
    enc = _enc(dims, dtype)
    sd = LB.state_dict(dims)
    W, b = sd["transformer_encoder.layers.0.linear1.weight"], sd["transformer_encoder.layers.0.linear1.bias"]
    out = "f32" if dtype in ("f32", "f32m") else dtype
    enc.set_option("generic", generic)
    try:
        for M in (1, 127, 128, 129):
            x = torch.randn(M, dims[1], generator=torch.Generator().manual_seed(100 + M)).to(TDT[dtype])
            xg = _x_with_nan_pad(x, dtype)
            want_id = enc.linear_plan("layers.0.linear1", M)             # the default handle plans linear1 with ReLU
            y_relu = enc.linear("layers.0.linear1", xg, relu=True)
            assert enc.last_linear_kernel == want_id
            y = enc.linear("layers.0.linear1", xg, act="gelu")
            assert enc.last_linear_kernel == want_id, (M, enc.last_linear_kernel, want_id)
            Wk = W.to(TDT[dtype]).float() if want_id in (MFMA, SKINNY) else W
            ref, bound = AB.gelu_linear_reference(x.float(), Wk, b, out)
            ratio, where = LB.ratio(y, ref, bound)
            print(f"gelu linear1 {dtype} {dims[1]}->{W.shape[0]} M = {M} generic = {generic} kernel {want_id}: worst ratio {ratio:.4f} at {where}")
            assert ratio <= 1.0, (M, ratio, where)
            assert not _same(y, y_relu)
            # GELU with a residual: refused, nothing written
            r = torch.zeros(M, W.shape[0], dtype=TDT[dtype], device="cuda")
            with pytest.raises(ValueError):
                enc.linear("layers.0.linear1", xg, res=r, act="gelu")
            with pytest.raises(ValueError):
                enc.linear("layers.0.linear1", xg, relu=True, act="gelu")
            keep = y.clone()
            rc = enc.lib.flope_tf_linear_act(enc.handle, b"layers.0.linear1", xg.data_ptr(), 0, r.data_ptr(), y.data_ptr(), 0, M, 2, None)
            torch.cuda.synchronize()
            assert rc == -1 and torch.equal(_bits(y), _bits(keep))
    finally:
        enc.set_option("generic", 0)


def test_gelu_f32m_linear_under_reserved_lds():
    """option f32mlds reserves untouched LDS in a tf_linear_f32m launch (more than 64 KiB needs the kernel's attribute set at create):
    the GELU instantiations at 96 and 160 KiB, alone and in a forward, give the bits of f32mlds = 0 -- as the ReLU ones do"""
    enc, full = _enc(DB, "f32m"), _enc(DB, "f32m", FULL)
    xf = AC.inputs(DB, 2, 33).cuda()
    want_f = full(xf).clone()
    want = {}
    for M in (1, 33, 129, 250):                                          # MP = 1, 2, 4 of tf_f32m_mp
        x = torch.randn(M, DB[1], generator=torch.Generator().manual_seed(300 + M)).cuda()
        want[M] = (x, enc.linear("layers.0.linear1", x, act="gelu").clone(), enc.linear("layers.0.linear1", x, relu=True).clone())
        assert enc.last_linear_kernel == 4
    try:
        for kib in (96, 160):
            enc.set_option("f32mlds", kib)
            full.set_option("f32mlds", kib)
            for M, (x, yg, yr) in want.items():
                assert _same(enc.linear("layers.0.linear1", x, act="gelu"), yg), (kib, M)
                assert enc.last_linear_kernel == 4
                assert _same(enc.linear("layers.0.linear1", x, relu=True), yr), (kib, M)
            assert _same(full(xf), want_f), kib
    finally:
        enc.set_option("f32mlds", 0)
        full.set_option("f32mlds", 0)


# ---- 3. bit contracts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [DA, DB], ids=["a", "b"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_skinny_and_linear_ln_gelu_bits(dtype, dims):
    enc = _enc(dims, dtype)
    sd = LB.state_dict(dims)
    g, be = sd["transformer_encoder.layers.0.norm1.weight"].cuda(), sd["transformer_encoder.layers.0.norm1.bias"].cuda()
    for M in (1, 15, 16, 17, 31, 32):
        x = _x_with_nan_pad(torch.randn(M, dims[1], generator=torch.Generator().manual_seed(7 + M)).to(TDT[dtype]), dtype)
        y0 = enc.linear("layers.0.linear1", x, act="gelu")
        assert enc.last_linear_kernel == MFMA
        enc.set_option("skinny", 1)
        try:
            y1 = enc.linear("layers.0.linear1", x, act="gelu")
            assert enc.last_linear_kernel == SKINNY and _same(y0, y1), M
            enc.set_option("skinny_ln", 1)
            yl, nl = enc.linear_ln_act("layers.0.linear1", x, g, be, "gelu")
            assert enc.last_linear_kernel == SKINNY_LN
            n0 = enc.layernorm(x.contiguous(), g, be)
            y2 = enc.linear("layers.0.linear1", n0, act="gelu")
            assert _same(nl, n0) and _same(yl, y2), M
            yr, _ = enc.linear_ln("layers.0.linear1", x, g, be, relu=True)                 # the older call keeps meaning ReLU
            assert _same(yr, enc.linear("layers.0.linear1", n0, relu=True))
        finally:
            enc.set_option("skinny_ln", 0)
            enc.set_option("skinny", 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_default_architecture_is_the_handle_of_before(dtype):
    x = AC.inputs(DA, 2, 33).cuda()
    a, b = _enc(DA, dtype), _enc(DA, dtype, AC.DEFAULT)
    assert a is not b and _same(a(x), b(x)) and _same(a(x, is_causal=True), b(x, is_causal=True))
    assert _same(a(x, lengths=[33, 7]), b(x, lengths=[33, 7]))


# ---- 4. whole forwards against the fixture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", AC.NON_DEFAULT, ids=AC.arch_id)
@pytest.mark.parametrize("shape", list(AC.SHAPES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_against_the_fp64_fixture(FX, dtype, shape, arch):
    dims = AC.SHAPES[shape]
    enc = _enc(dims, dtype, arch)
    assert enc.arch == arch
    for B, L in AC.BL:
        x = torch.from_numpy(FX[f"x_{shape}_{B}x{L}"]).cuda()
        y = enc(x).double().cpu().numpy()
        err = float(np.abs(y - FX[AC.key(shape, arch, B, L)]).max())
        print(f"{AC.arch_id(arch)} {dtype} {shape} {B}x{L}: max |err| {err:.3e} (tolerance {AC.TOL[dtype]:g})")
        assert np.isfinite(y).all() and err <= AC.TOL[dtype], (B, L, err)


# ---- 5. the contracts that must survive ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_causal_prefix_ragged_rows_and_clear_mask(dtype):
    enc = _enc(DA, dtype, FULL)
    x = AC.inputs(DA, 2, 33).cuda()
    full = enc(x, is_causal=True).clone()
    assert _same(enc(x[:, :20].contiguous(), is_causal=True), full[:, :20])
    lens = [33, 9]
    y = enc(x, lengths=lens).clone()
    ob = AC.state_dict(DA, True)["out_layer.bias"].cuda()
    assert torch.equal(_bits(y[1, 9:]), _bits(ob.expand(24, -1))) and not torch.equal(_bits(y[1, :9]), _bits(ob.expand(9, -1)))
    m = enc.make_mask(torch.zeros(33, 33, dtype=torch.bool))
    # the masked kernel walks the generic attention kernel's order: the bits are the plain forward's where that kernel runs the plain
    # forward -- option generic on a 16-bit handle; a float32 handle ignores it, so the f32m handle states f32mfma = 0 for the comparison
    enc.set_option("generic", 1)
    if dtype == "f32m":
        enc.set_option("f32mfma", 0)
    try:
        enc.attention(torch.zeros(2, 33, 3 * DA[1], dtype=TDT[dtype], device="cuda"))
        assert enc.last_attn_kernel == GENERIC
        assert _same(enc(x, mask=m), enc(x))
    finally:
        enc.set_option("generic", 0)
        if dtype == "f32m":
            enc.set_option("f32mfma", 1)
    m.close()


@pytest.mark.parametrize("n", [1, 5, 31])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_rows_are_the_causal_forward(dtype, n):
    """step, extend and prefill against enc(x, is_causal=True), linear and window = 4: in bits where the forward's attention kernel is
    the generic one (read from last_attn_kernel), within the dtype's tolerance elsewhere -- tests/test_gpu_tf_stream.py's conditions"""
    enc = _enc(DA, dtype, FULL)
    T = 8
    x = torch.randn(n, T, DA[0], generator=torch.Generator().manual_seed(60 + n)).cuda()
    for window in (0, 4):
        want = enc(x, is_causal=True, window=window).clone()
        enc.attention(torch.zeros(n, T, 3 * DA[1], dtype=TDT[dtype], device="cuda"), is_causal=True, window=window)
        bits = enc.last_attn_kernel == GENERIC

        def close(got, ref):
            return _same(got, ref) if bits else float((got - ref).abs().max()) <= AC.TOL[dtype]
        st = enc.open_stream(n, T, window=window)
        walked = torch.stack([st.step(x[:, t].contiguous()).clone() for t in range(T)], dim=1)
        assert close(walked, want), (window, "step")
        st.close()
        st = enc.open_stream(n, T, window=window)
        a = st.extend(x[:, :3].contiguous()).clone()
        b = st.extend(x[:, 3:T].contiguous()).clone()
        assert close(torch.cat([a, b], dim=1), want), (window, "extend")
        st.close()
        st = enc.open_stream(n, T, window=window)
        pre = st.prefill(x[:, :T - 1].contiguous()).clone()
        last = st.step(x[:, T - 1].contiguous()).clone()
        assert close(pre, want[:, :T - 1]) and close(last, want[:, T - 1]), (window, "prefill")
        st.close()


@pytest.mark.parametrize("n", [1, 5, 31])
@pytest.mark.parametrize("dims", [DA, DB], ids=["a", "b"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_skinny_options_keep_the_bits_and_fold_every_layer_norm(dtype, dims, n):
    enc = _enc(dims, dtype, FULL)
    nl = dims[4]
    x = torch.randn(n, 6, dims[0], generator=torch.Generator().manual_seed(70 + n)).cuda()

    def walk(window):
        st = enc.open_stream(n, 6, window=window)
        ys = torch.stack([st.step(x[:, t].contiguous()).clone() for t in range(6)])
        ln = enc.last_ln
        st.close()
        st = enc.open_stream(n, 6, window=window)
        ye = st.extend(x[:, :1].contiguous()).clone()
        st.close()
        return ys, ye, ln
    for window in (0, 4):
        off = walk(window)
        assert off[2] == (2 * nl + 1, 0)
        enc.set_option("skinny", 1)
        try:
            on = walk(window)
            assert on[2] == (2 * nl + 1, 0)
            enc.set_option("skinny_ln", 1)
            folded = walk(window)
        finally:
            enc.set_option("skinny_ln", 0)
            enc.set_option("skinny", 0)
        assert folded[2] == (1, 2 * nl)                                  # pre-norm: every per-layer LayerNorm folded, the final norm launched
        for r in (on, folded):
            assert _same(r[0], off[0]) and _same(r[1], off[1]), window
    nofn = _enc(dims, dtype, {"norm_first": True, "activation": "gelu"})
    nofn.set_option("skinny", 1)
    nofn.set_option("skinny_ln", 1)
    try:
        st = nofn.open_stream(n, 4, window=4)
        y = st.step(x[:, 0].contiguous()).clone()
        assert nofn.last_ln == (0, 2 * nl) and torch.isfinite(y).all()   # pre-norm without a final norm: no stand-alone LayerNorm at all
        st.close()
    finally:
        nofn.set_option("skinny_ln", 0)
        nofn.set_option("skinny", 0)


def test_fused_option_is_ignored_under_another_architecture():
    TOY = (16, 32, 9, 4, 2, 64)
    x = torch.randn(3, 12, TOY[0], generator=torch.Generator().manual_seed(2)).cuda()
    d = _enc(TOY, "f32", None, fused=1)
    assert d.forward_plan(3, 12) == "fused"
    d(x)
    assert d.last_forward_fused                                           # the default architecture keeps its single launch
    for arch in (FULL, {"activation": "gelu"}, {"norm_first": True}, {"final_norm": True}):
        a, b = _enc(TOY, "f32", arch, fused=1), _enc(TOY, "f32", arch)
        assert a.forward_plan(3, 12) == "launches"
        ya = a(x).clone()
        assert a.last_forward_fused is False and _same(ya, b(x))
        assert _same(a(x, is_causal=True), b(x, is_causal=True)) and a.last_forward_fused is False
