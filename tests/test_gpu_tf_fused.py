"""The encoder's single-launch forward on the device (option fused: tf_fused_f32, one sequence per workgroup).

The fused forward is held to BIT equality with the launch sequence of the same handle (fused = 0): every generic float32 kernel
computes an element in an order that does not depend on the thread that computes it, and the fused kernel calls the definitions of those orders that the kernels call.

  1. the reference's toy fixture at the bound of test_toy_fp32_matches_the_reference_output;
  2. bits against the launch sequence and 1e-5 against the fp64 oracle at every eligible shape of tests/test_tf_fused_host.py
     (a single token, a second lane trip over keys, over LayerNorm columns and over the rowwave k, head_dim 7, every linear on
     either summation order, no layer, more workgroups than are resident), the toy also on a side stream;
  3. ragged batches: bits against the ragged launch sequence, out_layer.bias behind a sequence, each sequence alone, equal lengths;
  4. the shapes and modes that must keep the launch sequence, and the refused arguments;
  5. an undisturbed handle.
"""
import os

import numpy as np
import pytest
import torch

import test_tf_fused_host as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # float32 against the reference fixture (tests/test_gpu_tf_encoder.py); the oracle's own float32 evaluation is within 2.3e-7


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return int((_bits(a) != _bits(b)).sum())


_DATA = {}


def data(name):
    """(dims, state dict, x, fp64 oracle of the fixed-length forward), computed once per case"""
    if name not in _DATA:
        from oracle import tf_encoder_ref as T
        dims, sd, x = F.case_data(name)
        _DATA[name] = (dims, sd, x, T.forward(sd, x, num_heads=dims[3]))
    return _DATA[name]


def encoder(name, dtype="f32", fused=0, max_tokens=None):
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, x, _ = data(name)
    enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=max_tokens or x.shape[0] * x.shape[1], fused=fused)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return enc


# ---- 1. the reference pin ---------------------------------------------------------------------------------------------------------
def test_toy_fused_matches_the_reference_output(ref_fixtures):
    enc = encoder("toy", fused=1)
    x = torch.from_numpy(ref_fixtures["tf_x"]).cuda()
    assert enc.forward_plan(x.shape[0], x.shape[1]) == "fused"
    y = enc(x).cpu().numpy()
    assert enc.last_forward_fused
    err = float(np.abs(y - ref_fixtures["tf_y"]).max())
    print(f"toy fused: max |y - tf_y| = {err:.2e}")
    assert err < TOL
    enc.close()


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.ELIGIBLE)
def test_fused_bits_equal_the_launch_sequence(name):
    dims, sd, x, ref = data(name)
    B, L = x.shape[0], x.shape[1]
    enc = encoder(name)
    xg = torch.from_numpy(x).cuda()
    keep = xg.clone()
    assert enc.forward_plan(B, L) == "launches"
    assert enc.set_option("fused", 1) == 0
    assert enc.forward_plan(B, L) == "fused"
    y1 = enc(xg).clone()
    assert enc.last_forward_fused is True
    assert enc.set_option("fused", 0) == 1
    y0 = enc(xg).clone()
    assert enc.last_forward_fused is False
    torch.cuda.synchronize()
    diff = _same(y1, y0)
    err = float(np.abs(y1.cpu().numpy() - ref).max())
    print(f"{name}: {diff} of {y1.numel()} elements differ in bits from the launch sequence; |y - fp64|max {err:.2e}")
    assert diff == 0
    assert err < TOL
    assert torch.equal(_bits(xg), _bits(keep)), "x was written"
    if name == "toy":
        side = torch.cuda.Stream()
        enc.set_option("fused", 1)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ys = enc(xg).clone()
            assert enc.last_forward_fused
        side.synchronize()
        assert _same(ys, y0) == 0, "the side stream's result differs"
    enc.close()


# ---- 3. ragged batches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lens", [("toy", F.TOY_LENGTHS), ("long", [70, 1])], ids=["toy", "long"])
def test_fused_ragged(name, lens):
    from oracle import tf_encoder_ref as T
    dims, sd, x, _ = data(name)
    B, L = x.shape[0], x.shape[1]
    enc = encoder(name, fused=1)
    clean = torch.from_numpy(x).cuda()
    xn = clean.clone()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    assert enc.forward_plan(B, L, lengths=lens) == "fused"
    y1 = enc(xn, lengths=lens).clone()
    assert enc.last_forward_fused
    enc.set_option("fused", 0)
    assert enc.forward_plan(B, L, lengths=lens) == "launches"
    y0 = enc(xn, lengths=lens).clone()
    assert not enc.last_forward_fused
    enc.set_option("fused", 1)
    torch.cuda.synchronize()
    diff = _same(y1, y0)
    print(f"{name} ragged {lens}: {diff} of {y1.numel()} elements differ in bits from the ragged launch sequence")
    assert diff == 0
    bias = torch.from_numpy(np.asarray(sd["out_layer.bias"], dtype=np.float32)).cuda()
    worst = 0.0
    for b, n in enumerate(lens):
        assert torch.isfinite(y1[b, :n]).all()
        if n < L:
            assert torch.equal(_bits(y1[b, n:]), _bits(bias.expand(L - n, -1))), f"padded rows of sequence {b} are not out_layer.bias"
        alone = enc(clean[b:b + 1, :n])
        assert enc.last_forward_fused
        assert _same(alone[0], y1[b, :n]) == 0, f"sequence {b} (length {n}) differs in bits from itself forwarded alone"
        ref = T.forward(sd, x[b:b + 1, :n], num_heads=dims[3])[0]
        worst = max(worst, float(np.abs(y1[b, :n].cpu().numpy() - ref).max()))
    print(f"{name} ragged: |y - fp64 per sequence|max {worst:.2e}")
    assert worst < TOL
    assert _same(enc(clean, lengths=[L] * B), enc(clean)) == 0, "equal lengths do not give the fixed-length fused bits"
    assert all(torch.isnan(xn[b, n:]).all() for b, n in enumerate(lens)), "a padded row of x was written"
    enc.close()


def test_fused_ragged_matches_the_reference_masked_run():
    """tests/golden/tf_varlen_fixture.npz: the reference module's own output under src_key_padding_mask, as test_whole_encoder holds the
    ragged launch sequence to it"""
    from flope_amd.tf_encoder import TransformerEncoder
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_varlen_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    x, lens, ref_y = f["x"], [int(v) for v in f["lengths"]], f["y"]
    B, L = x.shape[0], x.shape[1]
    enc = TransformerEncoder(*F.CASES["toy"][0], dtype="f32", max_tokens=B * L, fused=1)
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    xn = torch.from_numpy(x).cuda()
    for b, n in enumerate(lens):
        xn[b, n:] = float("nan")
    got = enc(xn, lengths=lens).cpu().numpy()
    assert enc.last_forward_fused
    e = max(float(np.abs(got[b, :n] - ref_y[b, :n]).max()) for b, n in enumerate(lens))
    print(f"fused ragged toy vs the reference's masked run: {e:.2e}")
    assert e < TOL
    pad = np.arange(L)[None, :] >= np.array(lens)[:, None]
    assert np.array_equal(got.view(np.int32)[pad], ref_y.view(np.int32)[pad])
    enc.close()


# ---- 4. fallback and precedence ---------------------------------------------------------------------------------------------------
def test_a_sequence_that_does_not_fit_keeps_the_launch_sequence():
    dims, sd, x, _ = data("big")
    B, L = x.shape[0], x.shape[1]
    enc = encoder("big", fused=1)
    xg = torch.from_numpy(x).cuda()
    assert enc.forward_plan(B, L) == "launches"
    y1 = enc(xg).clone()
    assert not enc.last_forward_fused
    enc.set_option("fused", 0)
    assert _same(y1, enc(xg)) == 0
    # ... and a ragged batch is judged at its longest sequence
    enc.set_option("fused", 1)
    assert enc.forward_plan(B, L, lengths=[L, 1]) == "launches"
    assert enc.forward_plan(B, L, lengths=[8, 1]) == "fused"
    enc.close()


@pytest.mark.parametrize("dtype", ["f16", "f32m"])
def test_other_modes_store_and_ignore_the_option(dtype):
    dims, sd, x, _ = data("toy")
    B, L = x.shape[0], x.shape[1]
    xg = torch.from_numpy(x).cuda()
    enc = encoder("toy", dtype=dtype)
    before = enc(xg).clone()
    assert enc.set_option("fused", 1) == 0
    assert enc.set_option("fused", 1) == 1                     # stored
    assert enc.forward_plan(B, L) == "launches"
    y = enc(xg)
    assert not enc.last_forward_fused
    assert _same(y, before) == 0
    enc.close()
    enc = encoder("toy", dtype=dtype, fused=1)                # the constructor's form of the same
    assert enc.forward_plan(B, L) == "launches"
    assert _same(enc(xg), before) == 0
    if dtype == "f32m":                                        # f32mfma takes precedence only while it is set
        enc.set_option("f32mfma", 0)
        assert enc.forward_plan(B, L) == "fused"
    enc.close()


def test_refused_arguments():
    from flope_amd.tf_encoder import TransformerEncoder
    dims, sd, x, _ = data("toy")
    B, L = x.shape[0], x.shape[1]
    enc = encoder("toy", fused=1)
    assert enc.set_option("fused", 2) < 0 and enc.set_option("fused", -1) < 0
    assert enc.set_option("fused", 1) == 1                     # a refused value changes nothing
    with pytest.raises(ValueError):
        TransformerEncoder(*dims, dtype="f32", max_tokens=8, fused=2)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 0"):
        enc.forward_plan(B, L, lengths=[10, 0, 3, 7, 10, 2, 9, 5])
    with pytest.raises(ValueError, match=r"lengths\[2\] = 11"):
        enc.forward_plan(B, L, lengths=[10, 1, 11, 7, 10, 2, 9, 5])
    with pytest.raises(ValueError):
        enc.forward_plan(B, L, lengths=[10, 1])                # too few values
    with pytest.raises(ValueError, match="max_tokens"):
        enc.forward_plan(B + 1, L)
    xg = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError, match=r"lengths\[1\] = 0"):
        enc(xg, lengths=[10, 0, 3, 7, 10, 2, 9, 5])            # the forward keeps its own refusal
    assert enc.forward_plan(0, L) == "launches"               # an empty batch runs nothing
    assert enc.forward_plan(B, L) == "fused"
    enc.close()


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------
def test_fused_forwards_leave_the_handle_as_it_was():
    dims, sd, x, _ = data("toy")
    enc = encoder("toy")
    xg = torch.from_numpy(x).cuda()
    before = enc(xg).clone()
    before_r = enc(xg, lengths=F.TOY_LENGTHS).clone()
    enc.set_option("fused", 1)
    enc(xg[:3, :4].contiguous())
    enc(xg)
    enc(xg, lengths=F.TOY_LENGTHS)
    assert enc.last_forward_fused
    enc.set_option("fused", 0)
    assert _same(enc(xg), before) == 0
    assert _same(enc(xg, lengths=F.TOY_LENGTHS), before_r) == 0
    assert not enc.last_forward_fused
    enc.close()
