"""Ragged batches of the encoder (flope_tf_forward_varlen) without a device:

  1. the fixture recorded from the reference module with src_key_padding_mask (tests/golden/tf_varlen_fixture.npz): its valid rows
     are the fp64 oracle applied to each sequence alone, its padded rows are out_layer.bias exactly -- the two facts the packed
     execution rests on;
  2. the host planner (flope_amd/csrc/tf_attn_plan.h through tests/host_harness/harness_tf_varlen.cpp): offsets, token count and
     maximum, every error case, the grid / block / LDS figures of the four variable-length launches against the formulas written
     out here, and the kernel id = tf_attn_pick at the longest sequence;
  3. the three new C symbols are declared and exported;
  4. a numpy emulation of the packed addressing the kernels use (row base off[b], the sequence's own length for every bound, mask
     and clamp, early exit of query blocks past it, a grid sized by the longest sequence) reproduces per-sequence attention to
     1e-12 over a buffer with NaN rows between and behind the sequences -- and two broken copies of it do not.
"""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import test_tf_attn_plan_host as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, MFMA64, TILED, F32M = 0, 1, 2, 3
OK, E_BATCH, E_LENGTH, E_TOKENS, E_OVERFLOW = 0, -1, -2, -3, -4
INT_MAX = 2 ** 31 - 1


# ---- 1. the reference's masked run ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    f = np.load(os.path.join(ROOT, "tests", "golden", "tf_varlen_fixture.npz"))
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    return f["x"], [int(v) for v in f["lengths"]], f["y"], sd


def test_fixture_is_small_and_data_only():
    path = os.path.join(ROOT, "tests", "golden", "tf_varlen_fixture.npz")
    assert os.path.getsize(path) < 100 * 1024
    f = np.load(path, allow_pickle=False)
    assert f["x"].shape == (6, 15, 16) and f["y"].shape == (6, 15, 9) and list(f["lengths"]) == [15, 1, 7, 12, 3, 15]


def test_fixture_valid_rows_are_each_sequence_alone(fixture):
    from oracle import tf_encoder_ref as T
    x, lengths, y, sd = fixture
    assert sorted(sd) == sorted(T.expected_keys(2))
    worst = 0.0
    for b, n in enumerate(lengths):
        alone = T.forward(sd, x[b:b + 1, :n], num_heads=4)
        worst = max(worst, float(np.abs(alone[0] - y[b, :n]).max()))
    print(f"fp64 oracle per sequence vs the reference's masked run: {worst:.2e}")
    assert worst < 1e-5


def test_fixture_padded_rows_are_the_output_bias(fixture):
    x, lengths, y, sd = fixture
    bias = sd["out_layer.bias"]
    n = 0
    for b, ln in enumerate(lengths):
        for i in range(ln, y.shape[1]):
            assert np.array_equal(y[b, i].view(np.int32), bias.view(np.int32)), (b, i)
            n += 1
    assert n == 6 * 15 - sum(lengths)


# ---- 2. the planner --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_varlen.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_varlen.so"])
    return C.CDLL(path)


def run_plan(plan, lengths, L, max_tokens, B=None):
    B = len(lengths) if B is None else B
    arr = (C.c_int * max(len(lengths), 1))(*lengths)
    off = (C.c_int * (max(B, 0) + 1))(*([-7] * (max(B, 0) + 1)))
    out3 = (C.c_int * 3)()
    rc = plan.tf_varlen_plan(arr, B, L, max_tokens, off, out3)
    return rc, list(off), list(out3)


def test_error_codes_are_the_documented_ones(plan):
    assert [plan.tf_varlen_err(i) for i in range(5)] == [OK, E_BATCH, E_LENGTH, E_TOKENS, E_OVERFLOW]


def test_offsets_token_count_and_maximum(plan):
    rc, off, (T, mx, bad) = run_plan(plan, [15, 1, 7, 12, 3, 15], 15, 53)
    assert rc == OK and off == [0, 15, 16, 23, 35, 38, 53] and (T, mx, bad) == (53, 15, -1)
    rc, off, (T, mx, _) = run_plan(plan, [1], 1, 1)
    assert rc == OK and off == [0, 1] and (T, mx) == (1, 1)
    rc, off, (T, mx, _) = run_plan(plan, [129, 1, 33, 64, 65, 32, 130], 130, 454)
    assert rc == OK and off == [0, 129, 130, 163, 227, 292, 324, 454] and (T, mx) == (454, 130)
    # B L may exceed max_tokens: only the packed count is bounded
    rc, off, (T, mx, _) = run_plan(plan, [2, 1, 1, 3], 100, 7)
    assert rc == OK and off == [0, 2, 3, 4, 7] and (T, mx) == (7, 3)
    # all lengths equal: the offsets of the fixed layout
    rc, off, (T, mx, _) = run_plan(plan, [10] * 4, 10, 40)
    assert rc == OK and off == [0, 10, 20, 30, 40] and (T, mx) == (40, 10)


def test_every_error_case(plan):
    assert run_plan(plan, [], 5, 100, B=0)[0] == E_BATCH
    assert run_plan(plan, [3], 5, 100, B=-1)[0] == E_BATCH
    rc, off, (T, mx, bad) = run_plan(plan, [3, 0, 2], 5, 100)
    assert rc == E_LENGTH and bad == 1 and off == [-7] * 4 and T == -1             # nothing written
    rc, _, (_, _, bad) = run_plan(plan, [3, 2, -1], 5, 100)
    assert rc == E_LENGTH and bad == 2
    rc, _, (_, _, bad) = run_plan(plan, [6, 2, 1], 5, 100)
    assert rc == E_LENGTH and bad == 0
    rc, off, _ = run_plan(plan, [3, 2, 3], 5, 7)
    assert rc == E_TOKENS and off == [-7] * 4
    assert run_plan(plan, [3, 2, 2], 5, 7)[0] == OK                                # T == max_tokens runs
    rc, off, _ = run_plan(plan, [INT_MAX] * 3, INT_MAX, INT_MAX)
    assert rc == E_OVERFLOW and off == [-7] * 4
    assert run_plan(plan, [INT_MAX, 1], INT_MAX, INT_MAX)[0] == E_OVERFLOW
    assert run_plan(plan, [INT_MAX - 1, 1], INT_MAX, INT_MAX)[0] == OK


def test_grid_and_lds_of_the_four_launches(plan):
    def launch(which, hd, B, H, mx):
        o = (C.c_long * 4)()
        plan.tf_varlen_launch(which, hd, B, H, mx, o)
        return list(o)

    for B, H, mx in itertools.product((1, 7, 256), (1, 2, 6), (1, 15, 16, 17, 32, 33, 128, 129, 130, 257, 512)):
        pad32 = (mx + 31) // 32 * 32
        for hd in (32, 64, 96, 128):
            assert launch(TILED, hd, B, H, mx) == [B * H, (mx + 127) // 128, 256, 2 * 2 * 64 * hd * 2]
        assert launch(MFMA64, 64, B, H, mx) == [B * H, 1, pad32 // 32 * 64, pad32 * 256]
        for hd in (8, 32, 64, 128):
            nt = 1 if hd <= 16 else 2 if hd <= 32 else 4 if hd <= 64 else 8
            assert launch(F32M, hd, B, H, mx) == [B * H, (mx + 15) // 16, 256, (16 * (((mx + 15) & ~15) + 4) + 3 * nt * 256) * 4]
        assert launch(GENERIC, 40, B, H, mx) == [B * H, min((mx + 3) // 4, 64), 256, 4 * mx * 4]
    # the same figures as the fixed-length launches of a batch whose every sequence has the longest length
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_attn.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_attn.so"])
    attn = C.CDLL(path)
    attn.tf_attn_lds_bytes.restype = C.c_long
    for which, hd, mx in [(TILED, 96, 200), (MFMA64, 64, 33), (F32M, 32, 50), (GENERIC, 40, 577)]:
        assert launch(which, hd, 3, 2, mx)[3] == attn.tf_attn_lds_bytes(which, hd, mx)


def test_kernel_id_is_tf_attn_pick_at_the_longest_sequence(plan):
    """The harness's tf_varlen_pick hands the longest length to tf_attn_pick and nothing else, so this pins the rule's table (as
    tests/test_tf_attn_plan_host.py does) at the lengths a ragged batch presents; it cannot notice launch_attention choosing by
    something other than the maximum.  That is check (a) of tests/test_gpu_tf_varlen.py: the id the device call returns for a batch
    of mixed lengths against this function at max(lengths)."""
    seen = set()
    for dtype, dh, mx, g, f, t, al in itertools.product((P.DT_BF16, P.DT_F16, P.DT_F32), P.HEAD_DIMS, P.SEQ_LENS, (0, 1), (0, 1), (0, 1, 2), (0, 1)):
        got = plan.tf_varlen_pick(dtype, dh, mx, g, f, t, al)
        assert got == P.expected(dtype, dh, mx, g, f, t, al), (dtype, dh, mx, g, f, t, al, got)
        seen.add(got)
    assert seen == {GENERIC, MFMA64, TILED, F32M}


# ---- 3. symbols ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["flope_tf_forward_varlen", "flope_tf_attention_varlen", "flope_tf_forward_flops_varlen"]


def test_new_symbols_are_declared_and_exported():
    from flope_amd import _lib
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    declared = set(re.findall(r"\b(flope_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.flope_tf_forward_flops_varlen.restype is C.c_double


def test_mask_and_lengths_conversion_on_the_host():
    import torch
    from flope_amd import tf_encoder as E
    m = torch.tensor([[False, False, True], [False, True, True], [False, False, False]])
    assert E._mask_to_lengths(m, 3, 3) == [2, 1, 3]
    with pytest.raises(ValueError, match="row 1"):
        E._mask_to_lengths(torch.tensor([[False, True], [True, False]]), 2, 2)          # a hole in front
    with pytest.raises(ValueError, match="row 0"):
        E._mask_to_lengths(torch.tensor([[True, True], [False, False]]), 2, 2)          # an empty sequence
    with pytest.raises(ValueError, match="row 2"):
        E._mask_to_lengths(torch.tensor([[False] * 3, [False] * 3, [False, True, False]]), 3, 3)
    with pytest.raises(ValueError):
        E._mask_to_lengths(torch.zeros(2, 3), 2, 3)                                      # not bool
    with pytest.raises(ValueError):
        E._mask_to_lengths(torch.zeros(2, 2, dtype=torch.bool), 2, 3)                    # wrong shape
    assert list(E._host_lengths(torch.tensor([3, 1]), 2)) == [3, 1] and list(E._host_lengths((4, 5, 6), 3)) == [4, 5, 6]
    with pytest.raises(ValueError):
        E._host_lengths([1, 2], 3)
    with pytest.raises(ValueError):
        E._host_lengths(torch.tensor([1.0, 2.0]), 2)


# ---- 4. the packed addressing, emulated -------------------------------------------------------------------------------------------
SENTINEL = 1234.0


def emulate(buf, start, lens, H, clamp="own", base="own"):
    """The variable-length kernels' addressing in float64 (tf_attn_f32m's shape: 16-query workgroups, key tiles of 16 with the rows
    past the sequence clamped for the loads, masked scores, P = 0 there and the values still multiplied in).  buf [rows][3 d];
    sequence b = rows start[b] .. start[b] + lens[b] - 1.  The grid is that of the longest sequence.
    clamp = "max": the defect of clamping to the longest length - 1; base = "fixed": the defect of row base b * longest."""
    d = buf.shape[1] // 3
    dh = d // H
    mx = max(lens)
    out = np.full((buf.shape[0], d), SENTINEL)
    for b, L in enumerate(lens):
        row0 = start[b] if base == "own" else b * mx
        last = (L if clamp == "own" else mx) - 1
        for h, qb in itertools.product(range(H), range((mx + 15) // 16)):
            q0 = qb * 16
            if q0 >= L:                                   # the workgroup leaves before its first barrier
                continue
            Lp = (L + 15) & ~15
            qrows = row0 + np.minimum(q0 + np.arange(16), last)
            krows = row0 + np.minimum(np.arange(Lp), last)
            q = buf[qrows, h * dh:(h + 1) * dh]
            k = buf[krows, d + h * dh:d + (h + 1) * dh]
            v = buf[krows, 2 * d + h * dh:2 * d + (h + 1) * dh]
            s = np.where(np.arange(Lp)[None, :] < L, q @ k.T / math.sqrt(dh), -3.0e38)
            e = np.exp(s[:, :L] - s[:, :L].max(axis=1, keepdims=True))
            p = np.zeros((16, Lp))
            p[:, :L] = e / e.sum(axis=1, keepdims=True)
            o = np.einsum("qj,jc->qc", p, v)              # 0 x NaN = NaN: a clamp that leaves the sequence shows
            for i in range(16):
                if q0 + i < L:
                    out[row0 + q0 + i, h * dh:(h + 1) * dh] = o[i]
    return out


def reference_alone(seq, H):
    d = seq.shape[1] // 3
    dh = d // H
    out = np.empty((seq.shape[0], d))
    for h in range(H):
        q, k, v = (seq[:, i * d + h * dh:i * d + (h + 1) * dh] for i in range(3))
        s = q @ k.T / math.sqrt(dh)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h * dh:(h + 1) * dh] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out


@pytest.fixture(scope="module")
def packed():
    """sequences of the GPU test's lengths scaled down (single key, ragged tile, full tile, tile boundary, a second query block next
    to sequences that leave it early), each followed by one NaN row, NaN rows behind the last"""
    rng = np.random.default_rng(3)
    H, dh = 2, 8
    lens = [33, 1, 9, 16, 17, 8, 34]
    seqs = [rng.standard_normal((n, 3 * H * dh)) for n in lens]
    rows, start = [], []
    for s in seqs:
        start.append(sum(r.shape[0] for r in rows))
        rows += [s, np.full((1, 3 * H * dh), np.nan)]
    rows.append(np.full((len(lens) * max(lens), 3 * H * dh), np.nan))       # (room for the broken copy that strides by the longest length)
    return np.concatenate(rows), start, lens, seqs, H


def _worst(out, start, lens, seqs, H):
    w = 0.0
    for s0, n, seq in zip(start, lens, seqs):
        err = np.abs(out[s0:s0 + n] - reference_alone(seq, H))
        w = max(w, float(np.where(np.isfinite(err), err, np.inf).max()))
    return w


def test_emulated_packed_addressing_is_per_sequence_attention(packed):
    buf, start, lens, seqs, H = packed
    out = emulate(buf, start, lens, H)
    w = _worst(out, start, lens, seqs, H)
    print(f"packed emulation vs each sequence alone: {w:.2e}")
    assert w < 1e-12
    valid = np.zeros(buf.shape[0], dtype=bool)
    for s0, n in zip(start, lens):
        valid[s0:s0 + n] = True
    assert (out[~valid] == SENTINEL).all(), "a store outside the sequences"
    assert np.isfinite(out[valid]).all()


def test_clamping_to_the_longest_length_fails(packed):
    buf, start, lens, seqs, H = packed
    assert not _worst(emulate(buf, start, lens, H, clamp="max"), start, lens, seqs, H) < 1e-12


def test_fixed_stride_offsets_fail(packed):
    buf, start, lens, seqs, H = packed
    assert not _worst(emulate(buf, start, lens, H, base="fixed"), start, lens, seqs, H) < 1e-12
