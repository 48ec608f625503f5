"""Causal attention of the encoder on the device (option "causal", `is_causal=` / `mask=`).

A causal row depends on the rows in front of it only, and every kernel computes a query from its own keys in an order that does not
depend on how long the sequence is -- so besides the tolerances against fp64 the causal path is held to BIT equalities:

  1. the four attention kernels stand-alone, the case table of tests/test_gpu_tf_varlen.py, at lengths with a single key, a diagonal
     inside a ragged step, a second query block with skipped blocks, and a reused ring stage: the kernel id of the non-causal pick,
     the fp64 causal reference (element-wise bound for 16 bits; 2e-4 for float32 and beside it the element-wise bound of
     tests/tf_attn_f32m_bound.py for tf_attn_f32m, the row bound of tests/tf_attn_mask_bound.py for the generic kernel), row 0 = v[0], the last row = the non-causal last
     row, prefix = prefix, a sentinel behind the output, two runs equal, and ragged x causal = each sequence alone;
  2. the whole encoder in every mode on two shapes: the fp64 causal restatement, the reference module's own causal output, mask= in
     both forms, prefix = prefix, lengths (valid rows, the reference's padded-and-masked rows, out_layer.bias behind them), the
     single launch of option fused, and an undisturbed handle;
  3. the masks that are refused.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import tf_attn_bound as AB
import tf_attn_causal_bound as CB
import tf_attn_f32m_bound as FB
import tf_attn_mask_bound as MB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_ID = {"bf16": 0, "f16": 1, "f32": 2, "f32m": 2}
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f32m": torch.float32}
GENERIC, MFMA64, TILED, F32M = 0, 1, 2, 3
SENTINEL = 1234.0                    # exact in f16, bf16 and float32
B, H = 2, 2
SEQ_LENS = [1, 33, 129, 161]
PREFIXES = [1, 32, 33, 64, 65, 128]
LENGTHS = [129, 1, 33, 64, 65, 32, 130]

# dtype, head_dim, options, the kernel id expected (tests/test_gpu_tf_varlen.py: ATTN_CASES)
ATTN_CASES = {
    "tiled": [("f16", 32, dict(attn_tiled=2), TILED), ("bf16", 32, dict(attn_tiled=2), TILED),
              ("f16", 128, dict(attn_tiled=2), TILED), ("bf16", 128, dict(attn_tiled=2), TILED)],
    "mfma": [("f16", 64, {}, MFMA64), ("bf16", 64, {}, MFMA64)],
    "generic": [("f16", 64, dict(generic=1), GENERIC), ("bf16", 32, dict(generic=1), GENERIC), ("f32", 8, {}, GENERIC)],
    "f32m": [("f32m", 8, {}, F32M), ("f32m", 64, {}, F32M)],
}


def _harness(name):
    path = os.path.join(ROOT, "tests", "host_harness", name)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/" + name])
    return C.CDLL(path)


PLAN = _harness("libflope_host_tf_varlen.so")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _qkv(dtype, hd, batch, L, seed):
    if dtype in ("f16", "bf16"):
        return AB.make_qkv(batch, L, H, hd, dtype, seed=seed)
    return torch.randn(batch, L, 3 * H * hd, generator=torch.Generator().manual_seed(seed * 977 + hd * 31 + L))


def _within_reference(got, qkv, dtype, what):
    """check 2: finite and within the fp64 causal reference"""
    assert torch.isfinite(got).all(), f"{what}: a non-finite output"
    if dtype in ("f16", "bf16"):
        ref, bound = CB.reference_of(qkv, H, dtype)
        r, where = AB.ratio(got, ref, bound)
        print(f"{what}: err / bound {r:.3f} at {where}")
        assert r <= 1.0, (what, where)
    else:
        err = float((got.double().cpu() - CB.attention_fp64(qkv, H)).abs().max())
        r2 = 0.0
        if dtype == "f32m":                                   # tf_attn_f32m: tests/tf_attn_f32m_bound.py, both assertions
            r, where, r2 = FB.verdict(got, FB.reference_of(qkv, H, causal=True))
        else:                                                 # the row kernel over the contiguous keys 0 .. i
            ref, bound = MB.reference_of(qkv, MB.make_allowed("causal", qkv.shape[1]), H, "f32")
            r, where = MB.ratio(got, ref, bound)
        print(f"{what}: |out - fp64|max {err:.2e}; err / bound {r:.3f} at {where}" + (f"; relL2 / yardstick {r2:.3f}" if dtype == "f32m" else ""))
        assert err < 2e-4, what
        assert r <= 1.0 and r2 <= 1.0, (what, where)          # every element within its derived bound


def _check_attention(dtype, hd, opts, want):
    from flope_amd.tf_encoder import TransformerEncoder
    d = H * hd
    enc = TransformerEncoder(16, d, 9, H, 0, 64, dtype=dtype, max_tokens=max(B * max(SEQ_LENS), sum(LENGTHS)), attn_tiled=opts.get("attn_tiled", 0))
    if opts.get("generic"):
        enc.set_option("generic", 1)
    og, of, ot = opts.get("generic", 0), int(dtype == "f32m"), opts.get("attn_tiled", 0)
    pick = lambda n: PLAN.tf_varlen_pick(DT_ID[dtype], hd, n, og, of, ot, 1)
    for L in SEQ_LENS:
        what = f"{dtype} hd={hd} L={L}"
        assert pick(L) == want
        host = _qkv(dtype, hd, B, L, seed=5)
        qkv = host.cuda()
        obig = torch.full((B * L + 64, d), SENTINEL, dtype=TDT[dtype], device="cuda")
        got = enc.attention(qkv, out=obig[:B * L].view(B, L, d), is_causal=True)
        assert enc.last_attn_kernel == want                                         # 1: the non-causal pick
        torch.cuda.synchronize()
        first = obig.clone()
        assert (obig[B * L:] == SENTINEL).all(), f"{what}: a store past the last token"          # 6
        _within_reference(got, host, dtype, what)                                   # 2
        assert torch.equal(_bits(got[:, 0]), _bits(qkv[:, 0, 2 * d:])), f"{what}: row 0 is not v[0]"                 # 3
        plain = enc.attention(qkv)
        assert enc.last_attn_kernel == want
        assert torch.equal(_bits(got[:, L - 1]), _bits(plain[:, L - 1])), f"{what}: the last row is not the non-causal last row"      # 4
        if L > 1:
            assert not torch.equal(_bits(got[:, 0]), _bits(plain[:, 0])), f"{what}: the option changed nothing"
        for n in PREFIXES:                                                          # 5
            if n >= L:
                continue
            assert pick(n) == want
            pre = enc.attention(qkv[:, :n].contiguous(), is_causal=True)
            assert enc.last_attn_kernel == want
            diff = int((_bits(pre) != _bits(got[:, :n])).sum())
            assert diff == 0, f"{what}: {diff} elements of the causal attention of the first {n} rows differ from the first {n} rows of the whole"
        obig[:B * L] = SENTINEL
        enc.attention(qkv, out=obig[:B * L].view(B, L, d), is_causal=True)
        torch.cuda.synchronize()
        assert torch.equal(_bits(obig), _bits(first)), f"{what}: two runs differ"   # 6
    # 7: ragged x causal
    T = sum(LENGTHS)
    assert all(pick(n) == want for n in LENGTHS)
    seqs = [_qkv(dtype, hd, 1, n, seed=11 + i)[0] for i, n in enumerate(LENGTHS)]
    big = torch.full((T + 64, 3 * d), float("nan"), dtype=TDT[dtype], device="cuda")
    big[:T] = torch.cat(seqs).cuda()
    obig = torch.full((T + 64, d), SENTINEL, dtype=TDT[dtype], device="cuda")
    packed = enc.attention(big[:T], lengths=LENGTHS, out=obig[:T], is_causal=True)
    assert enc.last_attn_kernel == want
    torch.cuda.synchronize()
    assert torch.isfinite(packed).all() and (obig[T:] == SENTINEL).all()
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    for i, n in enumerate(LENGTHS):
        alone = enc.attention(seqs[i].cuda().view(1, n, 3 * d), is_causal=True)
        diff = int((_bits(alone[0]) != _bits(packed[off[i]:off[i + 1]])).sum())
        assert diff == 0, f"{dtype} hd={hd}: sequence {i} (length {n}) of the ragged causal batch differs in {diff} elements from itself alone"
    _within_reference(packed[off[6]:off[7]][None], seqs[6][None], dtype, f"{dtype} hd={hd} ragged, length {LENGTHS[6]}")
    plain = enc.attention(big[:T], lengths=LENGTHS)                                 # a plain call afterwards is non-causal again
    assert not torch.equal(_bits(plain), _bits(packed))
    enc.close()


@pytest.mark.parametrize("case", ATTN_CASES["tiled"], ids=lambda c: f"{c[0]}-hd{c[1]}")
def test_attention_tiled(case):
    _check_attention(*case)


@pytest.mark.parametrize("case", ATTN_CASES["mfma"], ids=lambda c: f"{c[0]}-hd{c[1]}")
def test_attention_mfma64(case):
    _check_attention(*case)


@pytest.mark.parametrize("case", ATTN_CASES["generic"], ids=lambda c: f"{c[0]}-hd{c[1]}")
def test_attention_generic(case):
    _check_attention(*case)


@pytest.mark.parametrize("case", ATTN_CASES["f32m"], ids=lambda c: f"{c[0]}-hd{c[1]}")
def test_attention_f32m(case):
    _check_attention(*case)


# ---- the whole encoder ------------------------------------------------------------------------------------------------------------
TOY = (16, 32, 9, 4, 2, 64)
WIDE = (16, 128, 9, 2, 2, 256)
MODES = [("f32", 0, 2e-4), ("f32m", 0, 2e-4), ("f16", 0, 1.5e-2), ("f16", 1, 1.5e-2), ("bf16", 0, 1.2e-1), ("bf16", 1, 1.2e-1)]


@pytest.fixture(scope="module")
def shapes():
    """name -> (dims, state dict, x [B, L, in], lengths, fp64 causal restatement of the batch, ... of each sequence alone, the
    reference's causal output or None, its padded-and-masked output or None)"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_causal_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    out = {"toy": (TOY, sd, f["x"], [int(v) for v in f["lengths"]], f["y_causal"], f["y_causal_padded"])}
    wsd = T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)
    out["wide"] = (WIDE, wsd, np.random.default_rng(1).standard_normal((3, 50, 16)).astype(np.float32), [50, 1, 33], None, None)
    res = {}
    for name, (dims, s, x, lens, y, yp) in out.items():
        full = CB.causal_forward(s, x, dims[3])
        alone = [CB.causal_forward(s, x[b:b + 1, :n], dims[3])[0] for b, n in enumerate(lens)]
        res[name] = (dims, s, x, lens, full, alone, y, yp)
    return res


@pytest.mark.parametrize("shape", ["wide", "toy"])
@pytest.mark.parametrize("dtype,tiled,tol", MODES, ids=lambda v: str(v))
def test_whole_encoder(shapes, shape, dtype, tiled, tol):
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, x, lens, full, alone64, ref_y, ref_yp = shapes[shape]
    Bx, L = x.shape[0], x.shape[1]
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=Bx * L, attn_tiled=tiled)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    clean = torch.from_numpy(x).cuda()
    before = enc(clean).clone()                                       # the plain forward, in front of any causal call
    y = enc(clean, is_causal=True).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    e = float(np.abs(y.cpu().numpy() - full).max())
    print(f"{dtype} attn_tiled={tiled} {shape}: |y - fp64 causal restatement|max {e:.3e}, tolerance {tol}")
    assert e < tol
    assert not torch.equal(_bits(y), _bits(before))
    if ref_y is not None and dtype == "f32":
        er = float(np.abs(y.cpu().numpy() - ref_y).max())
        print(f"f32 toy vs the reference module under generate_square_subsequent_mask: {er:.2e}")
        assert er < 1e-5
    # mask= in torch's two forms, on the host and on the device, with and without the hint
    sub = torch.nn.Transformer.generate_square_subsequent_mask(L)
    above = torch.ones(L, L, dtype=torch.bool).triu(1)
    for m in (sub, above, sub.cuda(), above.cuda()):
        assert torch.equal(_bits(enc(clean, mask=m)), _bits(y))
    assert torch.equal(_bits(enc(clean, mask=sub, is_causal=True)), _bits(y))
    assert torch.equal(_bits(enc(clean, mask=torch.zeros(L, L))), _bits(before))      # an all-clear mask is no mask
    # the forward of a prefix is the prefix of the forward
    for n in sorted({1, 7, L // 2 + 1, L - 1}):
        diff = int((_bits(enc(clean[:, :n], is_causal=True)) != _bits(y[:, :n])).sum())
        assert diff == 0, f"{diff} elements of the causal forward of the first {n} rows differ from the first {n} rows of the whole"
    # causal inside each sequence of a ragged batch; padding never read
    xn = clean.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    yr = enc(xn, lengths=lens, is_causal=True).clone()
    torch.cuda.synchronize()
    bias = torch.from_numpy(np.asarray(sd["out_layer.bias"], dtype=np.float32)).cuda()
    worst = 0.0
    for b, n in enumerate(lens):
        assert torch.isfinite(yr[b, :n]).all()
        worst = max(worst, float(np.abs(yr[b, :n].cpu().numpy() - alone64[b]).max()))
        one = enc(clean[b:b + 1, :n], is_causal=True)
        diff = int((_bits(one[0]) != _bits(yr[b, :n])).sum())
        assert diff == 0, f"sequence {b} (length {n}): {diff} elements differ in bits from the sequence forwarded alone under causal"
        if n < L:
            assert torch.equal(_bits(yr[b, n:]), _bits(bias.expand(L - n, -1))), f"padded rows of sequence {b} are not out_layer.bias"
    print(f"{dtype} attn_tiled={tiled} {shape} ragged: |y - fp64 causal restatement per sequence|max {worst:.3e}")
    assert worst < tol
    if ref_yp is not None and dtype == "f32":
        ep = max(float(np.abs(yr[b, :n].cpu().numpy() - ref_yp[b, :n]).max()) for b, n in enumerate(lens))
        print(f"f32 toy vs the reference's padded-and-masked run, valid rows: {ep:.2e}")
        assert ep < 1e-5
    pad = torch.arange(L)[None, :] >= torch.tensor(lens)[:, None]
    assert torch.equal(_bits(enc(xn, src_key_padding_mask=pad, mask=sub)), _bits(yr))
    # the single launch of option fused (float32 handles)
    if dtype == "f32":
        assert enc.forward_plan(Bx, L, is_causal=True) == "launches" and not enc.last_forward_fused
        enc.set_option("fused", 1)
        if enc.forward_plan(Bx, L) == "fused":                         # (the wide shape does not fit a workgroup's LDS: nothing to compare)
            assert enc.forward_plan(Bx, L, is_causal=True) == "fused" and enc.forward_plan(Bx, L, lengths=lens, is_causal=True) == "fused"
            yf = enc(clean, is_causal=True)
            assert enc.last_forward_fused
            assert int((_bits(yf) != _bits(y)).sum()) == 0
            yfr = enc(xn, lengths=lens, is_causal=True)
            assert enc.last_forward_fused
            assert int((_bits(yfr) != _bits(yr)).sum()) == 0
            assert torch.equal(_bits(enc(clean)), _bits(before)) and enc.last_forward_fused
        else:
            assert shape == "wide" and enc.forward_plan(Bx, L, is_causal=True) == "launches"
        enc.set_option("fused", 0)
    assert torch.equal(_bits(enc(clean)), _bits(before)), "a plain forward after the causal ones does not return the bits it returned before"
    assert 0 < enc.flops(Bx, L, is_causal=True) < enc.flops(Bx, L)
    enc.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_masks_leave_the_handle_working(shapes):
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, x, lens, _, _, _, _ = shapes["toy"]
    Bx, L = x.shape[0], x.shape[1]
    enc = TransformerEncoder(*dims, dtype="f32", max_tokens=Bx * L)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    xg = torch.from_numpy(x).cuda()
    y = enc(xg, is_causal=True).clone()
    plain = enc(xg).clone()
    sub = torch.nn.Transformer.generate_square_subsequent_mask(L)
    hole = sub.clone()
    hole[3, 9] = 0.0
    with pytest.raises(ValueError, match=r"mask\[3, 9\]"):
        enc(xg, mask=hole)
    with pytest.raises(ValueError, match=r"mask\[0, 1\]"):
        enc(xg, mask=sub.t().contiguous().cuda())
    with pytest.raises(ValueError, match="mask must be"):
        enc(xg, mask=torch.nn.Transformer.generate_square_subsequent_mask(L + 1))
    with pytest.raises(ValueError, match="mask must be"):
        enc(xg, mask=sub[None].expand(Bx * dims[3], -1, -1))          # per-head masks have no kernel
    with pytest.raises(ValueError, match="is_causal=True with a mask"):
        enc(xg, mask=torch.zeros(L, L), is_causal=True)
    with pytest.raises(TypeError):
        enc(xg, None, None, sub)                                       # mask and is_causal are keyword-only
    assert torch.equal(_bits(enc(xg)), _bits(plain)) and torch.equal(_bits(enc(xg, is_causal=True)), _bits(y))
    assert torch.equal(_bits(enc(xg, mask=sub)), _bits(y))
    enc.close()
