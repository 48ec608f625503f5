"""The window on the 16-bit MFMA attention kernels (option "window_mfma") without a device:

  1. the planner's constexpr functions the WINDOW instantiations of tf_attn_mfma and tf_attn_tiled call (flope_amd/csrc/tf_attn_plan.h
     through tests/host_harness/harness_tf_window16.cpp) against brute force for every length up to 300, every window up to L + 2 and
     every wave, and once more in a stand-alone program under AddressSanitizer + UBSan;
  2. tf_attn_pick_window as a table;
  3. the emulation of the windowed 32-key-step walk with the guarded maximum (tests/tf_attn_window16_bound.py) passes the element-wise
     bound on every case, each of six broken copies fails on the cases named here, and is neutral where it must be;
  4. the option's values (needs a handle, hence a device: marked gpu).
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest
import torch

import tf_attn_bound as AB
import tf_attn_window16_bound as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMAX = 300
DT_BF16, DT_F16, DT_F32 = 0, 1, 2
GENERIC, MFMA64, TILED, F32M = 0, 1, 2, 3


def _so(name):
    rel = os.path.join("tests", "host_harness", name)
    if not os.path.exists(os.path.join(ROOT, rel)):
        subprocess.check_call(["make", "-C", ROOT, rel])
    return C.CDLL(os.path.join(ROOT, rel))


@pytest.fixture(scope="module")
def plan():
    return _so("libflope_host_tf_window16.so")


@pytest.fixture(scope="module")
def causal_plan():
    return _so("libflope_host_tf_causal.so")


@pytest.fixture(scope="module")
def attn_plan():
    return _so("libflope_host_tf_attn.so")


# ---- 1. the planner --------------------------------------------------------------------------------------------------------------
def _lo(i, W):
    return max(0, i + 1 - W) if W > 0 else 0


def _tiled_walk(plan, qb, w, L, W):
    cap = (L + 31) // 32
    steps = (C.c_int * cap)()
    first, end = C.c_int(-1), C.c_int(-1)
    n = plan.tfw16_tiled_walk(qb, w, L, W, steps, cap, C.byref(first), C.byref(end))
    assert 0 <= n <= cap
    return list(steps[:n]), first.value, end.value


def test_closed_forms(plan):
    for W in range(0, LMAX + 3):
        for q0 in range(0, LMAX, 32):
            lo = _lo(q0, W)
            assert plan.tfw16_first_step(q0, W) == lo // 32 * 32
            for kb in range(0, LMAX + 32, 32):
                assert plan.tfw16_step_taken(q0, kb, W) == int(kb <= q0 + 31 and kb + 31 >= lo), (q0, kb, W)
        for qb in range((LMAX + 127) // 128):
            assert plan.tfw16_tiled_first_block(qb, W) == _lo(qb * 128, W) // 64
    assert plan.tfw16_first_step(64, 0) == 0 and plan.tfw16_first_step(64, 64) == 0 and plan.tfw16_first_step(64, 33) == 32
    assert plan.tfw16_first_step(64, 32) == 32 and plan.tfw16_first_step(64, 1) == 64
    # the issue's example: W = 64, query q0 starts at q0 - 63 in step q0 - 64, query q0 + 31 at q0 - 32
    assert plan.tfw16_first_step(128, 64) == 64 and _lo(128 + 31, 64) == 96


def test_tiled_walk_against_brute_force(plan, causal_plan):
    """every visible pair in a taken step, every taken step in a loaded block and useful, one contiguous block range per workgroup
    that ends where the causal one ends; W = 0 and W >= L: the causal walk"""
    for L in list(range(1, 70)) + list(range(70, LMAX + 1, 7)) + [127, 128, 129, 255, 256, 257, LMAX]:
        for W in range(0, L + 3):
            for qb in range((L + 127) // 128):
                ranges = set()
                for w in range(4):
                    q0 = qb * 128 + w * 32
                    steps, first, end = _tiled_walk(plan, qb, w, L, W)
                    ranges.add((first, end))
                    assert 0 <= first < end == causal_plan.tfc_tiled_blocks(qb, L), (L, W, qb)
                    assert all(first <= kb // 64 < end for kb in steps), (L, W, qb, w)
                    if q0 >= L:
                        continue                                                    # clamped queries: never stored
                    last = min(q0 + 31, L - 1)
                    assert steps == sorted(set(steps)) and steps[-1] == q0, (L, W, qb, w)
                    covered = set()
                    for kb in steps:
                        covered.update(range(kb, min(kb + 32, L)))
                        assert any(_lo(q, W) <= k <= q for q in range(q0, last + 1) for k in range(kb, min(kb + 32, L))), (L, W, qb, w, kb)
                    for q in range(q0, last + 1):
                        assert covered >= set(range(_lo(q, W), q + 1)), (L, W, qb, w, q)
                    if W == 0 or W >= L:
                        cap = (L + 31) // 32
                        cs = (C.c_int * cap)()
                        trips = C.c_int(-1)
                        n = causal_plan.tfc_tiled_walk(qb, w, L, cs, cap, C.byref(trips))
                        assert steps == list(cs[:n]) and first == 0 and end == trips.value, (L, W, qb, w)
                assert len(ranges) == 1, (L, W, qb, ranges)                          # one trip, load and barrier count for the four waves


def test_resident_walk(plan):
    for L in range(1, LMAX + 1):
        cap = (L + 31) // 32
        for W in range(0, L + 3):
            for w in range(cap):
                steps = (C.c_int * cap)()
                n = plan.tfw16_mfma_walk(w, L, W, steps, cap)
                assert list(steps[:n]) == list(range(_lo(w * 32, W) // 32 * 32, w * 32 + 32, 32)), (L, W, w)


def test_a_wave_can_start_on_a_step_one_of_its_queries_does_not_see(plan):
    """why the step needs the guard: W = 64, the wave of query 128 starts at step 64, and its query 159 sees keys 96 .. 159 only"""
    assert plan.tfw16_first_step(128, 64) == 64 and _lo(159, 64) == 96 > 64 + 31
    # ... and where it cannot happen: W = 33 (query q0 + 31 starts at q0 - 1, inside step q0 - 32), W = 1
    for q0 in range(32, LMAX, 32):
        assert _lo(q0 + 31, 33) <= plan.tfw16_first_step(q0, 33) + 31 and _lo(q0 + 31, 1) <= plan.tfw16_first_step(q0, 1) + 31


def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """the planner once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_window16_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_WINDOW16_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_window16.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and f"tfw16_selfcheck({LMAX}) = 0" in r.stdout


# ---- 2. the pick under a window ---------------------------------------------------------------------------------------------------
def test_pick_window_table(plan, attn_plan):
    n = seen_mfma = seen_tiled = 0
    for dtype, dh, L, g, f, t, wm, al in itertools.product((DT_BF16, DT_F16, DT_F32), (8, 32, 40, 64, 96, 128, 160), (1, 512, 513, 2500),
                                                            (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1)):
        got = plan.tfw16_pick(dtype, dh, L, g, f, t, wm, al)
        base = attn_plan.tf_attn_pick(dtype, dh, L, g, f, t, al)
        if not wm or dtype == DT_F32 or not al:
            want = GENERIC                                                           # option 0, float32, misaligned
        else:
            want = base if base in (MFMA64, TILED) else GENERIC
        assert got == want, (dtype, dh, L, g, f, t, wm, al)
        seen_mfma += got == MFMA64
        seen_tiled += got == TILED
        n += 1
    assert n == 3 * 7 * 4 * 2 * 2 * 3 * 2 * 2 and seen_mfma and seen_tiled
    assert plan.tfw16_pick(DT_F16, 64, 512, 0, 0, 0, 1, 1) == MFMA64 and plan.tfw16_pick(DT_F16, 64, 513, 0, 0, 0, 1, 1) == GENERIC
    assert plan.tfw16_pick(DT_F16, 64, 513, 0, 0, 1, 1, 1) == TILED and plan.tfw16_pick(DT_BF16, 64, 100, 0, 0, 2, 1, 1) == TILED
    assert plan.tfw16_pick(DT_F16, 64, 100, 1, 0, 2, 1, 1) == GENERIC                # option generic wins
    assert plan.tfw16_pick(DT_F32, 64, 100, 0, 1, 2, 1, 1) == GENERIC                # tf_attn_f32m has no window


# ---- 3. the emulated walk within the bound ----------------------------------------------------------------------------------------
# where a wave's first step holds a key of every one of its queries (W = 33, W = 1) or the window is the whole sequence (W >= L)
NEUTRAL_GUARD = [((2, 129, 2, 64), 33), ((1, 161, 2, 32), 1), ((1, 33, 3, 32), 40)]
CAUGHT_GUARD = [c for c in WB.CASES if c not in NEUTRAL_GUARD]                       # W = 8, 32, 64, 100, 130
PLAIN_CAUSAL = ((1, 33, 3, 32), 40)
MASK_MUTATIONS = ["nowin", "from0", "wavewin", "offbyone"]


@pytest.fixture(scope="module")
def references():
    return {(c, W, dt): WB.reference_of(AB.make_qkv(*c, dt), c[2], dt, W) for c, W in WB.CASES for dt in ("f16", "bf16")}


@pytest.fixture(scope="module")
def walks():
    return {(c, W, dt): WB.emulate(AB.make_qkv(*c, dt), c[2], dt, W) for c, W in WB.CASES for dt in ("f16", "bf16")}


def test_cases_are_the_named_ones():
    assert [W for _, W in CAUGHT_GUARD] == [8, 64, 100, 32, 130] and len(WB.CASES) == 8
    for c, W in CAUGHT_GUARD:                                                        # some wave starts on a step its last query does not see
        L = c[1]
        assert any(WB.window_lo(min(q0 + 31, L - 1), W) > (WB.window_lo(q0, W) & ~31) + 31 for q0 in range(0, L, 32)), (c, W)
    for c, W in NEUTRAL_GUARD:
        L = c[1]
        assert not any(WB.window_lo(min(q0 + 31, L - 1), W) > (WB.window_lo(q0, W) & ~31) + 31 for q0 in range(0, L, 32)), (c, W)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_emulated_walk_passes_the_bound(references, walks, dtype):
    worst = 0.0
    for c, W in WB.CASES:
        ref, bound = references[(c, W, dtype)]
        r, where = AB.ratio(walks[(c, W, dtype)], ref, bound)
        print(f"{dtype} {c} W={W}: err / bound {r:.3f} at {where}")
        assert r <= 1.0, (c, W, where)
        worst = max(worst, r)
    print(f"{dtype}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_without_the_guard_the_walk_is_not_finite(references, walks, dtype):
    for c, W in CAUGHT_GUARD:
        got = WB.emulate(AB.make_qkv(*c, dtype), c[2], dtype, W, "noguard")
        r, where = AB.ratio(got, *references[(c, W, dtype)])
        print(f"{dtype} noguard {c} W={W}: err / bound {r} at {where}, {int((~torch.isfinite(got.float())).sum())} non-finite elements")
        assert not bool(torch.isfinite(got.float()).all()) and r > 1.0, (c, W)
    for c, W in NEUTRAL_GUARD:                                                       # every query sees a key in its wave's first step
        assert torch.equal(WB.emulate(AB.make_qkv(*c, dtype), c[2], dtype, W, "noguard"), walks[(c, W, dtype)]), (c, W)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_a_first_step_from_the_last_query_fails_the_bound(references, walks, dtype):
    for c, W in CAUGHT_GUARD:
        r, _ = AB.ratio(WB.emulate(AB.make_qkv(*c, dtype), c[2], dtype, W, "latefirst"), *references[(c, W, dtype)])
        print(f"{dtype} latefirst {c} W={W}: err / bound {r:.3g}")
        assert r > 1.0, (c, W)
    for c, W in NEUTRAL_GUARD:                                                       # first and last query start in the same step
        assert torch.equal(WB.emulate(AB.make_qkv(*c, dtype), c[2], dtype, W, "latefirst"), walks[(c, W, dtype)]), (c, W)


@pytest.mark.parametrize("mutation", MASK_MUTATIONS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_broken_masks_fail_the_bound(references, walks, dtype, mutation):
    smallest = float("inf")
    for c, W in WB.CASES:
        got = WB.emulate(AB.make_qkv(*c, dtype), c[2], dtype, W, mutation)
        if W >= c[1]:                                                                # plain causal: nothing to get wrong
            assert torch.equal(got, walks[(c, W, dtype)]), (c, W)
            continue
        r, _ = AB.ratio(got, *references[(c, W, dtype)])
        print(f"{dtype} {mutation} {c} W={W}: err / bound {r:.3g}")
        assert r > 1.0, (c, W)
        smallest = min(smallest, r)
    print(f"{dtype} {mutation}: smallest err / bound {smallest:.3g}")


def test_every_mutation_is_neutral_on_plain_causal_and_the_reference_agrees(walks):
    import tf_attn_causal_bound as CB
    c, W = PLAIN_CAUSAL
    assert (c, W) in WB.CASES and W >= c[1]
    for dtype in ("f16", "bf16"):
        qkv = AB.make_qkv(*c, dtype)
        for mutation in WB.MUTATIONS:
            assert torch.equal(WB.emulate(qkv, c[2], dtype, W, mutation), walks[(c, W, dtype)]), mutation
        assert torch.equal(walks[(c, W, dtype)], CB.emulate(qkv, c[2], dtype))       # the causal walk's bits
        (o, b), (co, cb) = WB.reference_of(qkv, c[2], dtype, W), CB.reference_of(qkv, c[2], dtype)
        assert torch.equal(o, co) and torch.equal(b, cb)
    qkv = AB.make_qkv(1, 200, 1, 96, "f16")                                          # W = 1: every row is its own v
    o, _ = WB.reference_of(qkv, 1, "f16", 1)
    assert torch.equal(o, qkv[..., 2 * 96:].double())


def test_the_option_is_documented_and_adds_no_symbol():
    import re
    from flope_amd import _lib
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert '"window_mfma" (default 0; 0 or 1, FLOPE_EINVAL outside' in header
    declared = set(re.findall(r"\b(flope_[a-z0-9_]+)\s*\(", header))
    assert not [n for n in declared if "window_mfma" in n] and not [n for n in _lib.SIGNATURES if "window_mfma" in n]
    assert _lib.load().flope_tf_set_option(None, b"window_mfma", 1) == _lib.EINVAL   # no handle, no option


# ---- 4. the option's values (a handle needs a device) -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_option_values():
    from flope_amd import _lib
    from flope_amd.tf_encoder import TransformerEncoder
    dims = (16, 32, 9, 4, 2, 64)
    for dtype in ("f16", "f32"):                                                     # float32 handles store it and ignore it
        enc = TransformerEncoder(*dims, dtype=dtype, max_tokens=64)
        assert enc.set_option("window_mfma", 0) == 0                                 # the default
        for bad in (-1, 2, 7):
            assert enc.set_option("window_mfma", bad) == _lib.EINVAL
            assert "window_mfma is 0 or 1" in enc.lib.flope_tf_last_error(enc.handle).decode()
        assert enc.set_option("window_mfma", 1) == 0 and enc.set_option("window_mfma", 1) == 1 and enc.set_option("window_mfma", 0) == 1
        enc.close()
    enc = TransformerEncoder(*dims, dtype="f16", max_tokens=64, window_mfma=1)
    assert enc.set_option("window_mfma", 1) == 1
    enc.close()
    with pytest.raises(ValueError, match="window_mfma must be 0 or 1"):
        TransformerEncoder(*dims, dtype="f16", max_tokens=64, window_mfma=2)
