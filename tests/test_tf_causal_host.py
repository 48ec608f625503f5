"""Causal attention of the encoder (option "causal") without a device:

  1. the fixture recorded from the reference module under generate_square_subsequent_mask (tests/golden/tf_causal_fixture.npz) pins
     the test-side fp64 causal restatement of the oracle (tests/tf_attn_causal_bound.py), alone and with a padding mask on top;
  2. the planner's constexpr functions the kernels call (flope_amd/csrc/tf_attn_plan.h through
     tests/host_harness/harness_tf_causal.cpp) against brute force for every length up to 300, and once more in a stand-alone
     program under AddressSanitizer + UBSan;
  3. the emulation of the 32-key-step walk with the wave skip passes the element-wise bound on every shape of the tiled kernel's
     tests, and four broken copies of it fail on every shape with more than one key;
  4. the Python mask helper;
  5. the option and the FLOP counts (these two need a handle, hence a device: marked gpu).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import tf_attn_bound as AB
import tf_attn_causal_bound as CB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMAX = 300


# ---- 1. the reference's causal runs -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    path = os.path.join(ROOT, "tests", "golden", "tf_causal_fixture.npz")
    assert os.path.getsize(path) < 100 * 1024
    f = np.load(path, allow_pickle=False)
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    return f["x"], [int(v) for v in f["lengths"]], f["y_causal"], f["y_causal_padded"], sd


def test_fixture_pins_the_causal_restatement(fixture):
    x, lengths, y, yp, sd = fixture
    assert x.shape == (6, 15, 16) and y.shape == (6, 15, 9) and yp.shape == (6, 15, 9) and lengths == [15, 1, 7, 12, 3, 15]
    e = float(np.abs(CB.causal_forward(sd, x, 4) - y).max())
    print(f"fp64 causal restatement vs the reference under generate_square_subsequent_mask: {e:.2e}")
    assert e < 1e-5
    from oracle import tf_encoder_ref as T
    plain = float(np.abs(T.forward(sd, x, num_heads=4) - y).max())
    print(f"(the unmasked oracle is {plain:.2f} away: the fixture is a causal one)")
    assert plain > 0.1


def test_fixture_with_padding_is_each_sequence_alone_under_causal(fixture):
    x, lengths, _, yp, sd = fixture
    worst = max(float(np.abs(CB.causal_forward(sd, x[b:b + 1, :n], 4)[0] - yp[b, :n]).max()) for b, n in enumerate(lengths))
    print(f"fp64 causal restatement per sequence vs the reference's masked and padded run, valid rows: {worst:.2e}")
    assert worst < 1e-5


def test_causal_prefix_property_of_the_restatement(fixture):
    """what makes one causal forward of a track the live answer at every frame"""
    x, _, _, _, sd = fixture
    full = CB.causal_forward(sd, x, 4)
    for n in (1, 7, 14):
        assert float(np.abs(CB.causal_forward(sd, x[:, :n], 4) - full[:, :n]).max()) < 1e-12


# ---- 2. the planner --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_causal.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_causal.so"])
    return C.CDLL(path)


def _tiled_walk(plan, qb, w, L):
    cap = (L + 31) // 32
    steps = (C.c_int * cap)()
    trips = C.c_int(-1)
    n = plan.tfc_tiled_walk(qb, w, L, steps, cap, C.byref(trips))
    assert 0 <= n <= cap
    return list(steps[:n]), trips.value


def test_closed_forms(plan):
    for L in range(1, LMAX + 1):
        for i in range(L):
            assert plan.tfc_keys(i, 1, L) == i + 1                                   # tf_attn_row's key loops
        for q0 in range(0, L, 32):
            assert plan.tfc_keys(q0, 32, (L + 31) // 32 * 32) == min((L + 31) // 32 * 32, q0 + 32)      # tf_attn_mfma's step loop
        for qb in range((L + 127) // 128):
            assert plan.tfc_tiled_blocks(qb, L) == (min(L, qb * 128 + 128) + 63) // 64
        for q0 in range(0, L, 16):
            assert plan.tfc_f32m_tiles(q0, L) == (min(L, q0 + 16) + 15) // 16
    assert [plan.tfc_step_taken(32, kb) for kb in (0, 32, 63, 64)] == [1, 1, 1, 0]
    # the issue's figure: L = 1024 walks sum 2 (y + 1) = 72 of 8 x 16 = 128 block iterations
    assert sum(plan.tfc_tiled_blocks(qb, 1024) for qb in range(8)) == 72


def test_tiled_walk_covers_every_visible_key_and_no_step_above(plan):
    for L in range(1, LMAX + 1):
        for qb in range((L + 127) // 128):
            trips = set()
            for w in range(4):
                q0 = qb * 128 + w * 32
                steps, t = _tiled_walk(plan, qb, w, L)
                trips.add(t)
                if q0 >= L:
                    continue                                                        # clamped queries: never stored
                last = min(q0 + 31, L - 1)
                assert steps[0] == 0 and steps == sorted(set(steps)), (L, qb, w)     # from step 0, ascending, each once
                covered = set()
                for kb in steps:
                    assert kb <= last, (L, qb, w, kb)                                # no step wholly above the wave's last query
                    covered.update(range(kb, min(kb + 32, L)))
                assert covered >= set(range(last + 1)), (L, qb, w)                   # every key j <= i of every query i of the wave
                assert all(kb // 64 < t for kb in steps)                             # ... inside the blocks the workgroup loads
            assert len(trips) == 1, (L, qb, trips)                                   # one barrier count for the four waves


def test_resident_walk(plan):
    for L in range(1, LMAX + 1):
        cap = (L + 31) // 32
        for w in range(cap):
            steps = (C.c_int * cap)()
            n = plan.tfc_mfma_walk(w, L, steps, cap)
            assert list(steps[:n]) == list(range(0, min(cap * 32, w * 32 + 32), 32)), (L, w)


def test_f32m_tiles_hold_the_diagonal_and_nothing_above(plan):
    for L in range(1, LMAX + 1):
        for q0 in range(0, L, 16):
            nt, last = plan.tfc_f32m_tiles(q0, L), min(q0 + 15, L - 1)
            assert (nt - 1) * 16 <= last < nt * 16 <= (L + 15) // 16 * 16, (L, q0, nt)


def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """the planner once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_causal_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_CAUSAL_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_causal.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and f"tfc_selfcheck({LMAX}) = 0" in r.stdout


# ---- 3. the emulated walk within the bound ----------------------------------------------------------------------------------------
CASES = AB.cases(64, 2)


@pytest.fixture(scope="module")
def references():
    return {(c, dt): CB.reference_of(AB.make_qkv(*c, dt), c[2], dt) for c in CASES for dt in ("f16", "bf16")}


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_emulated_walk_passes_the_bound(references, dtype):
    worst = 0.0
    for c in CASES:
        ref, bound = references[(c, dtype)]
        r, where = AB.ratio(CB.emulate(AB.make_qkv(*c, dtype), c[2], dtype), ref, bound)
        print(f"{dtype} {c}: err / bound {r:.3f} at {where}")
        assert r <= 1.0, (c, where)
        worst = max(worst, r)
    print(f"{dtype}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("mutation", CB.MUTATIONS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_broken_walks_fail_the_bound(references, dtype, mutation):
    smallest = float("inf")
    for c in CASES:
        if c[1] <= 1:
            continue
        ref, bound = references[(c, dtype)]
        r, _ = AB.ratio(CB.emulate(AB.make_qkv(*c, dtype), c[2], dtype, mutation), ref, bound)
        print(f"{dtype} {mutation} {c}: err / bound {r:.3g}")
        assert r > 1.0, c
        smallest = min(smallest, r)
    print(f"{dtype} {mutation}: smallest err / bound {smallest:.3g}")


def test_causal_reference_is_the_plain_one_where_they_must_agree():
    """the last query sees every key: its row of the causal reference and bound is tf_attn_bound's own"""
    for c in CASES[:4]:
        qkv = AB.make_qkv(*c, "f16")
        (o, b), (po, pb) = CB.reference_of(qkv, c[2], "f16"), AB.reference_of(qkv, c[2], "f16")
        assert torch.equal(o[:, -1], po[:, -1]) and torch.equal(b[:, -1], pb[:, -1])
        assert torch.equal(o[:, 0], qkv[:, 0, 2 * o.shape[-1]:].double())           # row 0 is v[0]


# ---- 4. the mask helper -----------------------------------------------------------------------------------------------------------
def test_mask_helper():
    from flope_amd import tf_encoder as E
    L = 7
    sub = torch.nn.Transformer.generate_square_subsequent_mask(L)
    above = torch.ones(L, L, dtype=torch.bool).triu(1)
    assert E._mask_is_causal(sub, L) is True
    assert E._mask_is_causal(sub.double(), L) is True and E._mask_is_causal(sub.half(), L) is True
    assert E._mask_is_causal(above, L) is True
    assert E._mask_is_causal(None, L) is False
    assert E._mask_is_causal(torch.zeros(L, L), L) is False and E._mask_is_causal(torch.zeros(L, L, dtype=torch.bool), L) is False
    assert E._mask_is_causal(torch.zeros(1, 1), 1) is False and E._mask_is_causal(torch.zeros(1, 1, dtype=torch.bool), 1) is False
    hole = above.clone()
    hole[4, 2] = True
    with pytest.raises(ValueError, match=r"mask\[4, 2\]"):
        E._mask_is_causal(hole, L)
    fhole = sub.clone()
    fhole[2, 5] = 0.0
    with pytest.raises(ValueError, match=r"mask\[2, 5\]"):
        E._mask_is_causal(fhole, L)
    with pytest.raises(ValueError, match=r"mask\[0, 1\]"):
        E._mask_is_causal(torch.ones(L, L, dtype=torch.bool).triu(2), L)             # a shifted diagonal: key i + 1 visible
    with pytest.raises(ValueError, match=r"mask\[0, 0\]"):
        E._mask_is_causal(torch.ones(L, L, dtype=torch.bool).triu(0), L)             # shifted the other way: the diagonal masked
    with pytest.raises(ValueError, match=r"mask\[0, 1\]"):
        E._mask_is_causal(above.t(), L)                                              # causal transposed
    with pytest.raises(ValueError, match=r"mask\[0, 1\]"):
        E._mask_is_causal(sub.t(), L)
    with pytest.raises(ValueError, match=r"mask\[1, 0\]"):
        E._mask_is_causal(torch.full((L, L), -1.0).tril(-1) + sub, L)                # a finite additive bias is not a mask here
    for wrong in (torch.zeros(L, L + 1), torch.zeros(L - 1, L - 1, dtype=torch.bool), torch.zeros(2, L, L), above[None]):
        with pytest.raises(ValueError, match="mask must be"):
            E._mask_is_causal(wrong, L)
    with pytest.raises(ValueError, match="mask must be"):
        E._mask_is_causal(torch.zeros(L, L, dtype=torch.int64), L)


def test_the_option_is_documented_and_adds_no_symbol():
    import re
    from flope_amd import _lib
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert '"causal" (default 0; 0 or 1, FLOPE_EINVAL outside)' in header
    declared = set(re.findall(r"\b(flope_[a-z0-9_]+)\s*\(", header))
    assert not [n for n in declared if "causal" in n] and not [n for n in _lib.SIGNATURES if "causal" in n]
    assert _lib.load().flope_tf_set_option(None, b"causal", 1) == _lib.EINVAL        # no handle, no option


# ---- 5. the option and the FLOP counts (a handle needs a device) -------------------------------------------------------------------
@pytest.mark.gpu
def test_option_values_and_flop_counts():
    from flope_amd import _lib
    from flope_amd.tf_encoder import TransformerEncoder
    i, d, o, H, nl, ff = dims = (16, 32, 9, 4, 2, 64)
    enc = TransformerEncoder(*dims, dtype="f32", max_tokens=64)
    assert enc.set_option("causal", 0) == 0
    for bad in (-1, 2, 7):
        assert enc.set_option("causal", bad) == _lib.EINVAL
        assert "causal is 0 or 1" in enc.lib.flope_tf_last_error(enc.handle).decode()
    assert enc.set_option("causal", 1) == 0 and enc.set_option("causal", 0) == 1     # the previous value comes back
    lens = [15, 1, 7, 12, 3, 15]
    lin = lambda M: M * i * d + M * d * o + nl * (M * d * 3 * d + M * d * d + 2 * M * d * ff)
    plain = lambda ls: 2.0 * (lin(sum(ls)) + nl * 2 * d * sum(n * n for n in ls))
    causal = lambda ls: 2.0 * (lin(sum(ls)) + nl * d * sum(n * (n + 1) for n in ls))
    assert enc.flops(6, 15) == plain([15] * 6) and enc.flops(6, 15, lengths=lens) == plain(lens)
    assert enc.flops(6, 15, is_causal=True) == causal([15] * 6) and enc.flops(6, 15, lengths=lens, is_causal=True) == causal(lens)
    assert enc.flops(6, 15) == plain([15] * 6), "a plain call after a causal one is non-causal again"
    assert enc.flops(1, 1, is_causal=True) == enc.flops(1, 1)                        # one key either way
    enc.close()
