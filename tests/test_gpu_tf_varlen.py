"""Ragged batches of the encoder on the device (flope_tf_forward_varlen / flope_tf_attention_varlen).

A masked forward of a right-padded batch is, per sequence, the forward of that sequence alone at its own length, and every kernel
computes a token from its own sequence only -- so the packed path is held to BIT equality with the fixed-length path run on each
sequence alone, besides the tolerances against fp64 that the fixed-length tests use:

  1. the four variable-length attention kernels stand-alone, one test per kernel id, on lengths with a single key, a ragged 32-key
     step, a full block, a block boundary, the reuse of a ring stage, a second query block, and sequences that leave that block
     early next to ones that need it; NaN rows behind the packed input, a sentinel behind the packed output;
  2. the whole encoder in every mode on two shapes: tolerances of the fp64 oracle per sequence, out_layer.bias in the padded rows
     (whose inputs are NaN), bit equality with each sequence alone, with the fixed path for equal lengths, of mask and lengths,
     and an undisturbed handle;
  3. capacity (B L > max_tokens >= T) and the refused batches.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import tf_attn_bound as AB
import tf_attn_f32m_bound as FB
import tf_attn_mask_bound as MB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_ID = {"bf16": 0, "f16": 1, "f32": 2, "f32m": 2}
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f32m": torch.float32}
GENERIC, MFMA64, TILED, F32M = 0, 1, 2, 3
SENTINEL = 1234.0                    # exact in f16, bf16 and float32
LENGTHS = [129, 1, 33, 64, 65, 32, 130]
H = 2


def _harness(name):
    path = os.path.join(ROOT, "tests", "host_harness", name)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/" + name])
    return C.CDLL(path)


PLAN = _harness("libflope_host_tf_varlen.so")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _sequences(dtype, hd):
    """one qkv [len, 3 H hd] per length, in the handle's dtype"""
    if dtype in ("f16", "bf16"):
        return [AB.make_qkv(1, n, H, hd, dtype, seed=11 + i)[0] for i, n in enumerate(LENGTHS)]
    g = torch.Generator().manual_seed(17 + hd)
    return [torch.randn(n, 3 * H * hd, generator=g) for n in LENGTHS]


def _fp64(seq, hd):
    q, k, v = (t.double() for t in AB.split_heads(seq[None], H))
    return AB.merge_heads(torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, dim=-1) @ v)[0]


# dtype, head_dim, options, the kernel id expected
ATTN_CASES = {
    "tiled": [("f16", 32, dict(attn_tiled=2), TILED), ("bf16", 32, dict(attn_tiled=2), TILED),
              ("f16", 128, dict(attn_tiled=2), TILED), ("bf16", 128, dict(attn_tiled=2), TILED)],
    "mfma": [("f16", 64, {}, MFMA64), ("bf16", 64, {}, MFMA64)],
    "generic": [("f16", 64, dict(generic=1), GENERIC), ("bf16", 32, dict(generic=1), GENERIC), ("f32", 8, {}, GENERIC)],
    "f32m": [("f32m", 8, {}, F32M), ("f32m", 64, {}, F32M)],
}


def _check_attention(dtype, hd, opts, want):
    from flope_amd.tf_encoder import TransformerEncoder
    d, T = H * hd, sum(LENGTHS)
    enc = TransformerEncoder(16, d, 9, H, 0, 64, dtype=dtype, max_tokens=T, attn_tiled=opts.get("attn_tiled", 0))
    if opts.get("generic"):
        enc.set_option("generic", 1)
    og, of, ot = opts.get("generic", 0), int(dtype == "f32m"), opts.get("attn_tiled", 0)
    pick = lambda n: PLAN.tf_varlen_pick(DT_ID[dtype], hd, n, og, of, ot, 1)
    assert pick(max(LENGTHS)) == want
    assert all(pick(n) == want for n in LENGTHS)              # what makes the comparison with each sequence alone one of bits
    seqs = _sequences(dtype, hd)

    def run(order):
        lens = [LENGTHS[i] for i in order]
        big = torch.full((T + 64, 3 * d), float("nan"), dtype=TDT[dtype], device="cuda")
        big[:T] = torch.cat([seqs[i] for i in order]).cuda()
        obig = torch.full((T + 64, d), SENTINEL, dtype=TDT[dtype], device="cuda")
        got = enc.attention(big[:T], lengths=lens, out=obig[:T])
        assert enc.last_attn_kernel == want                  # (a)
        torch.cuda.synchronize()
        first = obig.clone()
        assert torch.isfinite(got).all(), "a non-finite output: a row outside its sequence was read, or a padded key was not masked"
        assert (obig[T:] == SENTINEL).all(), "a store past the last token"
        obig[:T] = SENTINEL
        enc.attention(big[:T], lengths=lens, out=obig[:T])
        torch.cuda.synchronize()
        assert torch.equal(_bits(obig), _bits(first)), "two runs differ"          # (e)
        assert torch.isnan(big[T:]).all()
        off = np.concatenate([[0], np.cumsum(lens)])
        return {i: first[off[j]:off[j + 1]].clone() for j, i in enumerate(order)}

    fwd = run(list(range(len(LENGTHS))))
    for i, n in enumerate(LENGTHS):
        alone = enc.attention(seqs[i].cuda().view(1, n, 3 * d))
        assert enc.last_attn_kernel == want
        diff = int((_bits(alone[0]) != _bits(fwd[i])).sum())
        ref = _fp64(seqs[i], hd)
        err = float((fwd[i].double().cpu() - ref).abs().max())
        line = f"{dtype} hd={hd} len={n}: {diff} of {alone.numel()} elements differ in bits from the sequence alone; |out - fp64|max {err:.2e}"
        r2 = 0.0
        if dtype in ("f16", "bf16"):
            r64, bound = AB.reference_of(seqs[i][None], H, dtype)
            r, where = AB.ratio(fwd[i][None], r64, bound)
        elif dtype == "f32m":                                 # tf_attn_f32m: tests/tf_attn_f32m_bound.py, both assertions
            r, where, r2 = FB.verdict(fwd[i][None], FB.reference_of(seqs[i][None], H))
        else:                                                 # the row kernel over the contiguous keys 0 .. n - 1
            r64, bound = MB.reference_of(seqs[i][None], MB.make_allowed("clear", n), H, "f32")
            r, where = MB.ratio(fwd[i][None], r64, bound)
        print(line + f"; err / bound {r:.3f}" + (f"; relL2 / yardstick {r2:.3f}" if dtype == "f32m" else ""))
        assert diff == 0                                      # (b)
        if dtype in ("f16", "bf16"):
            assert r <= 1.0, (n, where)                       # (c) (the generic kernel keeps float32 probabilities: inside the same bound)
        else:
            assert err < 2e-4                                 # (d)
            assert r <= 1.0 and r2 <= 1.0, (n, where)         # ... and every element within its derived bound
    rev = run(list(range(len(LENGTHS)))[::-1])
    for i in range(len(LENGTHS)):
        assert torch.equal(_bits(rev[i]), _bits(fwd[i])), f"sequence {i} depends on its place in the batch"      # (f)
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
    """name -> (dims, state dict, x [B, L, in], lengths, fp64 oracle of each sequence alone, the reference's masked output or None)"""
    from oracle import tf_encoder_ref as T
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_varlen_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    out = {"toy": (TOY, sd, f["x"], [int(v) for v in f["lengths"]], f["y"])}
    wsd = T.synthetic_state_dict(WIDE[0], WIDE[1], WIDE[2], WIDE[4], WIDE[5], seed=5)
    out["wide"] = (WIDE, wsd, np.random.default_rng(1).standard_normal((5, 50, 16)).astype(np.float32), [50, 1, 17, 33, 49], None)
    res = {}
    for name, (dims, s, x, lens, y) in out.items():
        oracle = [T.forward(s, x[b:b + 1, :n], num_heads=dims[3])[0] for b, n in enumerate(lens)]
        res[name] = (dims, s, x, lens, oracle, y)
    return res


@pytest.mark.parametrize("shape", ["wide", "toy"])
@pytest.mark.parametrize("dtype,tiled,tol", MODES, ids=lambda v: str(v))
def test_whole_encoder(shapes, shape, dtype, tiled, tol):
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, x, lens, oracle, ref_y = shapes[shape]
    B, L = x.shape[0], x.shape[1]
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=B * L, attn_tiled=tiled)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    clean = torch.from_numpy(x).cuda()
    before = enc(clean).clone()                                       # the fixed-length path, padding attended to
    xn = clean.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    y = enc(xn, lengths=lens)
    torch.cuda.synchronize()
    bias = torch.from_numpy(np.asarray(sd["out_layer.bias"], dtype=np.float32)).cuda()
    worst = 0.0
    for b, n in enumerate(lens):
        worst = max(worst, float(np.abs(y[b, :n].cpu().numpy() - oracle[b]).max()))
        assert torch.isfinite(y[b, :n]).all()
        if n < L:
            assert torch.equal(_bits(y[b, n:]), _bits(bias.expand(L - n, -1))), f"padded rows of sequence {b} are not out_layer.bias"
    print(f"{dtype} attn_tiled={tiled} {shape}: |y - fp64 per sequence|max {worst:.3e}, tolerance {tol}")
    assert worst < tol
    if ref_y is not None and dtype == "f32":
        got = y.cpu().numpy()
        e = max(float(np.abs(got[b, :n] - ref_y[b, :n]).max()) for b, n in enumerate(lens))
        print(f"f32 toy vs the reference's masked run: {e:.2e}")
        assert e < 1e-5
        assert np.array_equal(got.view(np.int32)[np.arange(L)[None, :] >= np.array(lens)[:, None]],
                              ref_y.view(np.int32)[np.arange(L)[None, :] >= np.array(lens)[:, None]])
    for b, n in enumerate(lens):
        alone = enc(clean[b:b + 1, :n])
        diff = int((_bits(alone[0]) != _bits(y[b, :n])).sum())
        assert diff == 0, f"sequence {b} (length {n}): {diff} elements differ in bits from the sequence forwarded alone"
    assert torch.equal(_bits(enc(clean, lengths=[L] * B)), _bits(before)), "equal lengths do not give the fixed path's bits"
    mask = torch.arange(L)[None, :] >= torch.tensor(lens)[:, None]
    assert torch.equal(_bits(enc(xn, src_key_padding_mask=mask)), _bits(y))
    assert torch.equal(_bits(enc(xn, src_key_padding_mask=mask.cuda())), _bits(y))
    assert torch.equal(_bits(enc(xn, lengths=torch.tensor(lens))), _bits(y))
    assert torch.equal(_bits(enc(clean)), _bits(before)), "the handle's state was disturbed"
    assert enc.flops(B, L, lengths=[L] * B) == enc.flops(B, L) and 0 < enc.flops(B, L, lengths=lens) < enc.flops(B, L)
    enc.close()


# ---- capacity and errors ----------------------------------------------------------------------------------------------------------
def test_capacity_and_refused_batches(shapes):
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, x, _, _, _ = shapes["toy"]
    enc = TransformerEncoder(*dims, dtype="f32", max_tokens=20)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    xg = torch.from_numpy(x[:4]).cuda()                               # B L = 60 > max_tokens = 20 = T
    lens = [5, 1, 7, 7]
    with pytest.raises(RuntimeError, match="max_tokens"):
        enc(xg)                                                       # the fixed path needs B L <= max_tokens
    y = enc(xg, lengths=lens)
    for b, n in enumerate(lens):
        assert torch.equal(_bits(enc(xg[b:b + 1, :n])[0]), _bits(y[b, :n]))
    last = lambda: enc.lib.flope_tf_last_error(enc.handle).decode()
    with pytest.raises(ValueError, match="max_tokens"):
        enc(xg, lengths=[6, 1, 7, 7])
    assert "max_tokens" in last()
    with pytest.raises(ValueError, match=r"lengths\[1\] = 0"):
        enc(xg, lengths=[5, 0, 7, 7])
    assert "lengths[1]" in last()
    with pytest.raises(ValueError, match=r"lengths\[2\] = 16"):
        enc(xg, lengths=[1, 1, 16, 1])
    with pytest.raises(ValueError):
        enc(xg, lengths=[5, 1, 7])                                    # one value short
    hole = torch.zeros(4, 15, dtype=torch.bool)
    hole[:, 5:] = True
    hole[3, 2] = True
    with pytest.raises(ValueError, match="row 3"):
        enc(xg, src_key_padding_mask=hole)
    with pytest.raises(ValueError, match="not both"):
        enc(xg, lengths=lens, src_key_padding_mask=hole)
    qkv = torch.zeros(20, 96, device="cuda")
    with pytest.raises(ValueError, match="max_tokens"):
        enc.attention(torch.zeros(21, 96, device="cuda"), lengths=[10, 11])
    with pytest.raises(ValueError):
        enc.attention(qkv, lengths=[10, 11])                          # T is not the row count
    with pytest.raises(ValueError, match=r"lengths\[0\] = 0"):
        enc.attention(qkv, lengths=[0, 20])
    assert torch.equal(_bits(enc(xg, lengths=lens)), _bits(y)), "the handle does not work as before after the refusals"
    enc.close()
