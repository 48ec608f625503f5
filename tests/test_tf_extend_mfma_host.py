"""Option "extend_mfma"  without a device:

  1. the planner tf_attn16_extend and flope_tf_stream_attention_extend call (flope_amd/csrc/tf_encoder_stream.h through
     tests/host_harness/harness_tf_extend16.cpp) against brute force written here in plain words: every (pos0, len, capacity <= 8, W), the
     same grid scaled by 32-key steps with a token more and less, random larger cases, the launch, the eligibility rule for head_dim 1 ..
     299, the hook's refusals, and once more in a stand-alone program under AddressSanitizer + UBSan;
  2. the emulation of the kernel's walk (tests/tf_extend_mfma_emul.py): its chunk rows are, bit for bit, the rows the aligned emulations of
     tf_attn_tiled / tf_attn_mfma give the whole track (the per-query independence the device contract rests on), they pass the element-wise
     bound at every shape of the device list, each broken copy exceeds it at a shape of the list, and a NaN in a cache row that holds no
     visible key reaches the output only through the copy that does not write zeros.
"""
import ctypes as C
import os
import random
import subprocess

import pytest
import torch

import tf_attn_bound as AB
import tf_attn_causal_bound as CB
import tf_attn_window16_bound as WB
import tf_extend_mfma_emul as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_BF16, DT_F16, DT_F32 = 0, 1, 2
ZERO, CACHE, CHUNK = 0, 1, 2
OK, COUNT, LENGTH, CACHED, TOKENS = 0, -1, -5, -8, -9


@pytest.fixture(scope="module")
def plan():
    rel = os.path.join("tests", "host_harness", "libflope_host_tf_extend16.so")
    if not os.path.exists(os.path.join(ROOT, rel)):
        subprocess.check_call(["make", "-C", ROOT, rel])
    lib = C.CDLL(os.path.join(ROOT, rel))
    lib.tfx_out_row.restype = C.c_longlong
    return lib


# ---- 1. the planner --------------------------------------------------------------------------------------------------------------
def _lo(p, W):
    return max(0, p + 1 - W) if W > 0 else 0


def _brute(plan, pos0, ln, capacity, W):
    """One chunk of `ln` tokens behind a track of pos0, in plain words.  The cache in front of the call: a linear one holds key j in row j,
    a ring the last `capacity` keys, key j in row j % capacity."""
    held = {}
    for j in range(max(0, pos0 - capacity) if W else 0, pos0):
        held[j % capacity if W else j] = j
    Labs = pos0 + ln
    kinds, rows = (C.c_int * 64)(), (C.c_int * 64)()
    ny = (ln + 127) // 128
    assert not plan.tfx_block_live(ln, ny) and all(plan.tfx_block_live(ln, y) for y in range(ny))
    for y in range(ny):
        first_q, last_q = pos0 + 128 * y, pos0 + min(128 * y + 127, ln - 1)
        lo_wg = _lo(first_q, W)
        assert plan.tfx_lo(pos0, y, W) == lo_wg
        t0, t1 = plan.tfx_first_block(pos0, y, W), plan.tfx_last_block(pos0, ln, y)
        assert (t0, t1) == (lo_wg // 64, last_q // 64)
        source = {}
        for t in range(t0, t1 + 2):                                   # t1 + 1: loaded behind the last block, read by nobody
            plan.tfx_block_keys(t, pos0, ln, capacity, W, y, kinds, rows)
            for r in range(64):
                j = 64 * t + r
                assert j not in source
                source[j] = (kinds[r], rows[r])
                if j < lo_wg or j >= Labs:
                    assert kinds[r] == ZERO, (j, "a key outside [lo_wg, Labs) is a zero row")
                elif j >= pos0:
                    assert (kinds[r], rows[r]) == (CHUNK, j - pos0), (j, "a key of the call comes from its chunk row")
                else:
                    assert kinds[r] == CACHE and 0 <= rows[r] < capacity and held.get(rows[r]) == j, (j, "a cached row holds that key")
        for w in range(4):
            q0 = plan.tfx_q0(pos0, y, w)
            assert q0 == first_q + 32 * w
            for p in range(q0, min(q0 + 32, Labs)):
                assert plan.tfx_out_row(1000, pos0, p) == 1000 + (p - pos0)
                for j in range(_lo(p, W), p + 1):                     # every visible key: in a loaded block, in a step the wave takes
                    assert t0 <= j // 64 <= t1 and j in source and source[j][0] != ZERO
                    assert plan.tfx_step_taken(q0, j & ~31, Labs, W)
            # ... and the wave takes no step wholly above its last query or at / past Labs
            for kb in range(max(0, t0 - 1) * 64, (t1 + 2) * 64, 32):
                if kb > q0 + 31 or kb >= Labs:
                    assert not plan.tfx_step_taken(q0, kb, Labs, W)


def test_every_small_chunk_against_brute_force(plan):
    n = 0
    for capacity in range(1, 9):
        for W in range(0, capacity + 1):
            for pos0 in range(0, 2 * capacity + 2):
                for ln in range(1, 2 * capacity + 3):
                    if not W and pos0 + ln > capacity:
                        continue
                    _brute(plan, pos0, ln, capacity, W)
                    assert plan.tfx_walk(pos0, ln, capacity, W) == 0
                    n += 1
    assert n == 7080


def test_the_grid_scaled_by_steps_and_random_larger_chunks(plan):
    """the same (pos0, len, capacity, W) times 32, with a token more and less: the harness's own walk on all of them, the walk written here
    on every thirteenth, and on random chunks of up to three query blocks over rings of up to 700 rows"""
    n = 0
    for c in range(1, 5):
        for w in range(0, c + 1):
            for a in range(0, 2 * c + 2):
                for l in range(1, 2 * c + 3):
                    for da in (-1, 0, 1):
                        for dl in (-1, 0, 1):
                            capacity, W, pos0, ln = 32 * c, 32 * w, 32 * a + da, 32 * l + dl
                            if pos0 < 0 or (not W and pos0 + ln > capacity):
                                continue
                            assert plan.tfx_walk(pos0, ln, capacity, W) == 0, (pos0, ln, capacity, W)
                            if n % 13 == 0:
                                _brute(plan, pos0, ln, capacity, W)
                            n += 1
    rng = random.Random(11)
    for _ in range(60):
        capacity = rng.randint(1, 700)
        W = rng.choice([0, 1, rng.randint(1, capacity), capacity])
        ln = rng.randint(1, 330)
        pos0 = rng.randint(0, 3000) if W else rng.randint(0, max(0, capacity - ln))
        if not W and pos0 + ln > capacity:
            continue
        assert plan.tfx_walk(pos0, ln, capacity, W) == 0, (pos0, ln, capacity, W)
        _brute(plan, pos0, ln, capacity, W)
    # the last positions the kernel's int arithmetic is written for
    top = plan.tfx_pos_max()
    assert top == 2 ** 31 - 1 - 256
    assert plan.tfx_positions_ok(top - 300, 300) and not plan.tfx_positions_ok(top - 299, 300) and not plan.tfx_positions_ok(-1, 1)
    assert plan.tfx_walk(top - 300, 300, 64, 33) == 0
    _brute(plan, top - 300, 300, 64, 33)


def test_launch_covers_ragged_lengths(plan):
    out = (C.c_longlong * 4)()
    for hd, lds in ((32, 16384), (64, 32768), (96, 49152), (128, 65536)):
        for max_len in (1, 7, 127, 128, 129, 256, 257, 4096):
            plan.tfx_launch(3, 6, max_len, hd, out)
            assert (out[0], out[2], out[3]) == (18, 256, lds)
            assert out[1] == (max_len + 127) // 128
            # a shorter sequence of the same call: its live query blocks are a prefix of the grid, the others leave
            for ln in (1, max_len // 2 + 1, max_len):
                live = [y for y in range(out[1]) if plan.tfx_block_live(ln, y)]
                assert live == list(range((ln + 127) // 128))


def test_eligibility_rule(plan):
    for hd in range(1, 300):
        for H in (1, 3):
            want = hd in (32, 64, 96, 128)
            assert plan.tfx_ok(DT_F16, hd, hd * H) == want and plan.tfx_ok(DT_BF16, hd, hd * H) == want
            assert not plan.tfx_ok(DT_F32, hd, hd * H)
    assert not plan.tfx_ok(DT_F16, 0, 0) and not plan.tfx_ok(DT_F16, 64, 0) and not plan.tfx_ok(DT_F16, 64, 68)


def test_refusals_of_the_hook(plan):
    out = (C.c_int * 4)()
    arr = lambda *v: (C.c_int * len(v))(*v)
    call = lambda tracks, cap, W, maxtok, n, L, lens, cached: plan.tfx_check_hook(tracks, cap, W, maxtok, n, L, lens, cached, out)
    assert call(3, 16, 0, 64, 3, 9, arr(5, 9, 2), arr(0, 8, 1)) == OK and list(out) == [-1, 9, 5, 7]
    assert call(3, 8, 8, 64, 3, 9, arr(5, 9, 2), arr(0, 8, 1)) == OK and out[1] == 8            # a ring: lengths may pass the capacity
    assert call(3, 16, 5, 64, 1, 40, arr(40), arr(30)) == OK and list(out) == [-1, 5, 10, 10]
    for n in (0, -1, 4):
        assert call(3, 16, 0, 64, n, 9, arr(5, 9, 2, 1), arr(0, 8, 1, 0)) == COUNT
    assert call(3, 16, 0, 2, 3, 9, arr(5, 9, 2), arr(0, 8, 1)) == COUNT                         # n > max_tokens
    assert call(3, 16, 0, 64, 3, 0, arr(5, 9, 2), arr(0, 8, 1)) == COUNT
    assert call(3, 16, 0, 64, 3, 9, None, arr(0, 8, 1)) == COUNT and call(3, 16, 0, 64, 3, 9, arr(5, 9, 2), None) == COUNT
    for bad_len in (0, -3, 10):
        assert call(3, 16, 0, 64, 3, 9, arr(5, bad_len, 2), arr(0, 0, 1)) == LENGTH and out[0] == 1
    assert call(3, 8, 0, 64, 3, 9, arr(5, 9, 2), arr(0, 8, 1)) == LENGTH and out[0] == 1         # a linear state: above capacity
    for bad_cached in (-1, 2, 7):
        assert call(3, 16, 0, 64, 3, 9, arr(5, 9, 2), arr(0, 8, bad_cached)) == CACHED and out[0] == 2
    assert call(3, 16, 0, 6, 3, 9, arr(5, 9, 2), arr(0, 8, 1)) == TOKENS
    assert list(out) == [-1, -1, -1, -1]                                                        # a refusal writes nothing but the index


def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """the planner once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_extend16_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_EXTEND16_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_harness", "harness_tf_extend16.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "tfx_selfcheck = 0" in r.stdout, r.stdout + r.stderr


# ---- 2. the emulation ------------------------------------------------------------------------------------------------------------
CASES = EM.all_cases()


def test_cases_are_the_named_ones():
    assert EM.LINEAR == [(0, 1, 2, 32), (0, 33, 1, 64), (31, 2, 2, 64), (63, 66, 2, 64), (100, 130, 1, 96), (500, 12, 2, 64)]
    assert EM.RAGGED == ((0, 65, 200), (7, 1, 40), 2, 128)
    assert EM.WINDOWED == [(70, 70, 150, 45, 2, 64), (70, 96, 150, 45, 2, 64), (70, 70, 150, 100, 2, 64), (1, 16, 20, 20, 2, 32), (33, 64, 30, 70, 1, 128)]
    assert len(CASES) == 14


@pytest.fixture(scope="module")
def references():
    """(O, bound) of the whole track, per case and dtype: computed once"""
    out = {}
    for dtype in ("f16", "bf16"):
        for case in CASES:
            W, _, c, m, H, hd = case
            qkv = EM.track_qkv(c, m, H, hd, dtype)
            out[(case, dtype)] = WB.reference_of(qkv, H, dtype, W) if W else CB.reference_of(qkv, H, dtype)
    return out


@pytest.fixture(scope="module")
def walks():
    out = {}
    for dtype in ("f16", "bf16"):
        for case in CASES:
            W, cap, c, m, H, hd = case
            out[(case, dtype)] = EM.emulate(EM.track_qkv(c, m, H, hd, dtype), H, dtype, c, W, cap)
    return out


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_chunk_rows_are_the_aligned_walks_rows_in_bits(walks, dtype):
    for case in CASES:
        W, _, c, m, H, hd = case
        qkv = EM.track_qkv(c, m, H, hd, dtype)
        whole = WB.emulate(qkv, H, dtype, W) if W else CB.emulate(qkv, H, dtype)
        assert torch.equal(walks[(case, dtype)], whole[:, c:]), case


def test_any_split_of_a_track_gives_one_set_of_bits():
    """a track of 70 tokens as one chunk, as 31 + 1 + 33 + 5 and as seventy chunks of one, linear and under a window on a small ring"""
    for W, cap in ((0, 70), (8, 11), (8, 8)):
        qkv = AB.make_qkv(1, 70, 2, 32, "f16")
        whole = WB.emulate(qkv, 2, "f16", W) if W else CB.emulate(qkv, 2, "f16")
        for split in ([70], [31, 1, 33, 5], [1] * 70):
            at = 0
            for m in split:
                got = EM.emulate(qkv[:, :at + m], 2, "f16", at, W, cap)
                assert torch.equal(got, whole[:, at:at + m]), (W, cap, split, at)
                at += m


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_emulated_walk_passes_the_bound(references, walks, dtype):
    worst = 0.0
    for case in CASES:
        O, bound = references[(case, dtype)]
        c = case[2]
        r, where = AB.ratio(walks[(case, dtype)], O[:, c:], bound[:, c:])
        print(f"{dtype} {case}: err / bound {r:.3g} at {where}")
        assert r <= 1.0, (case, r, where)
        worst = max(worst, r)
    print(f"{dtype}: worst err / bound {worst:.3g}")


# where each broken copy must show, in f16: (mutation, cases of the list)
BROKEN = {
    "alignedlast": [(0, 33, 31, 2, 2, 64), (0, 129, 63, 66, 2, 64), (70, 70, 150, 45, 2, 64)],
    "relmask": [(0, 33, 31, 2, 2, 64), (0, 512, 500, 12, 2, 64), (33, 64, 30, 70, 1, 128)],
    "nowrap": [(70, 70, 150, 45, 2, 64), (70, 96, 150, 45, 2, 64), (70, 70, 150, 100, 2, 64)],
    "stalechunk": [(0, 1, 0, 1, 2, 32), (0, 129, 63, 66, 2, 64), (70, 70, 150, 100, 2, 64)],
    "boundary": [(0, 33, 31, 2, 2, 64), (0, 230, 100, 130, 1, 96), (1, 16, 20, 20, 2, 32)],
}


@pytest.mark.parametrize("mutation", sorted(BROKEN))
def test_broken_copies_fail_the_bound(references, mutation):
    for case in BROKEN[mutation]:
        assert case in CASES
        W, cap, c, m, H, hd = case
        got = EM.emulate(EM.track_qkv(c, m, H, hd, "f16"), H, "f16", c, W, cap, mutation)
        O, bound = references[(case, "f16")]
        r, _ = AB.ratio(got, O[:, c:], bound[:, c:])
        print(f"{mutation} {case}: err / bound {r:.3g}")
        assert r > 1.0, (mutation, case, r)


def test_a_nan_below_the_window_needs_the_zero_rows(references, walks):
    """stale cache rows full of NaN, a ring's rows below the call's first window among them: the correct walk never reads one (same bits as over finite garbage, finite), the copy that leaves the
    rows outside [lo_wg, Labs) as they are multiplies p = 0 by NaN in the PV product"""
    shown = []
    for case in EM.WINDOWED:
        W, cap, c, m, H, hd = case
        qkv = EM.track_qkv(c, m, H, hd, "f16")
        good = EM.emulate(qkv, H, "f16", c, W, cap, None, stale="nan")
        assert torch.isfinite(good.float()).all() and torch.equal(good, walks[(case, "f16")]), case
        bad = EM.emulate(qkv, H, "f16", c, W, cap, "nozero", stale="nan")
        if not torch.isfinite(bad.float()).all():
            shown.append(case)
    # a ring with rows below the window (capacity > W), a ring that is not full yet, a window of one key
    assert {(70, 96, 150, 45, 2, 64), (1, 16, 20, 20, 2, 32), (33, 64, 30, 70, 1, 128)} <= set(shown), shown
    # a linear cache: the rows at and past Labs of the last block
    W, cap, c, m, H, hd = CASES[2]
    qkv = EM.track_qkv(c, m, H, hd, "f16")
    assert torch.equal(EM.emulate(qkv, H, "f16", c, W, cap + 40, None, stale="nan"), walks[(CASES[2], "f16")])
    assert not torch.isfinite(EM.emulate(qkv, H, "f16", c, W, cap + 40, "nozero", stale="nan").float()).all()
