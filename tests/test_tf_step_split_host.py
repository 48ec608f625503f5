"""Option step_split without a device:

  1. the planner of flope_amd/csrc/tf_encoder_stream.h through tests/host_harness/harness_tf_split.cpp against brute force: for every
     visible-key count 1 .. 4096 the partition gives each key to exactly one (wave, block, lane) and one lane group of the value pass;
     for windows with every lo % capacity a key's cache row is its ring row; the cached / chunk source of every key of an extend query
     agrees with tf_extend_cached / tf_extend_chunk0; tf_split_lds knows no position; the launches cover their work; tf_step_split_ok
     is the rule it states; the checks of flope_tf_stream_attention;
  2. the same once more in a stand-alone program under AddressSanitizer + UBSan;
  3. tests/tf_step_split_bound.py: the bound passes the emulation of the row's walk at every shape tests/test_gpu_tf_step_split.py
     uses (headroom printed), and every broken copy of the emulation exceeds it at a shape of that list;
  4. the C-ABI: _lib.SIGNATURES holds both symbols, they refuse NULL, the header declares them.
"""
import ctypes as C
import os
import subprocess

import pytest
import torch

import tf_step_split_bound as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, COUNT, LENGTH = 0, -1, -5


@pytest.fixture(scope="module")
def plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_split.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_split.so"])
    lib = C.CDLL(path)
    lib.tfs_lds.restype = C.c_longlong
    return lib


# ---- 1. the planner ---------------------------------------------------------------------------------------------------------------------
def test_every_key_has_one_wave_block_and_lane(plan):
    assert (plan.tfs_waves(), plan.tfs_block()) == (4, 64)
    owner, taker = (C.c_int * 4096)(), (C.c_int * 4096)()
    for L in range(1, 4097):
        lps = (1, 2, 8, 16, 32, 64, 4)[L % 7]
        assert plan.tfs_walk_partition(L, lps, owner, taker) == 0, (L, lps)
        assert list(owner[:L]) == [1] * L and list(taker[:L]) == [1] * L, (L, lps)
        nb = -(-L // 64)
        assert plan.tfs_blocks(L) == nb
        assert [plan.tfs_wave_blocks(L, w) for w in range(4)] == [len(range(w, nb, 4)) for w in range(4)], L
    for k in range(0, 4096):                                                    # brute force, in plain words
        assert (plan.tfs_key_block(k), plan.tfs_key_lane(k), plan.tfs_block_wave(k // 64)) == (k // 64, k % 64, (k // 64) % 4)
    for lps in (1, 2, 4, 8, 16, 32, 64):                                        # every lane-group width at the sizes around a block
        for L in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513):
            assert plan.tfs_walk_partition(L, lps, owner, taker) == 0
            assert list(owner[:L]) == [1] * L and list(taker[:L]) == [1] * L, (L, lps)


def test_ring_rows_for_every_first_slot(plan):
    """a window's keys, counted from lo, land in their ring rows for every lo % capacity; the count from lo knows no capacity"""
    for capacity in (1, 2, 3, 7, 70, 96):
        for W in sorted({1, min(2, capacity), capacity // 2 or 1, capacity}):
            for slo in range(capacity):
                lo = slo + 3 * capacity
                rows = [plan.tfs_cache_row(k, slo, capacity) for k in range(W - 1)]      # the cached keys of a full window
                assert rows == [(lo + k) % capacity for k in range(W - 1)], (capacity, W, slo)
                assert len(set(rows)) == len(rows)


def test_extend_key_sources_agree_with_the_extend_planner(plan):
    ext = C.CDLL(os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_extend.so")) if os.path.exists(
        os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_extend.so")) else None
    cached, row = C.c_int(), C.c_int()
    for capacity in range(1, 8):
        for W in range(0, capacity + 1):
            for pos0 in range(0, 2 * capacity + 2):
                for ln in range(1, capacity + 3):
                    if W == 0 and pos0 + ln > capacity:
                        continue
                    for i in range(ln):
                        p = pos0 + i
                        lo = max(0, p + 1 - W) if W else 0
                        srcs = []
                        for k in range(p - lo + 1):
                            plan.tfs_extend_key(pos0, i, capacity, W, k, C.byref(cached), C.byref(row))
                            srcs.append((cached.value, row.value))
                        want = [(1, (j % capacity if W else j)) if j < pos0 else (0, j - pos0) for j in range(lo, p + 1)]
                        assert srcs == want, (pos0, ln, capacity, W, i)
                        if ext is not None:
                            assert sum(c for c, _ in srcs) == ext.tfe_cached(pos0, lo)
                            chunk = [r for c, r in srcs if not c]
                            assert chunk[0] == ext.tfe_chunk0(pos0, lo) and chunk[-1] == i


def test_lds_rule_and_launches(plan):
    for hd in (8, 32, 64, 128):
        assert plan.tfs_lds(hd) == 4 * (64 + 2 + hd) * 4                        # four probability rows, four (m, l, o[hd]); no position in it
    assert plan.tfs_lds(128) <= 64 * 1024
    out3, out4 = (C.c_longlong * 3)(), (C.c_longlong * 4)()
    for n in (1, 2, 3, 256):
        for H in (1, 2, 6):
            plan.tfs_step_launch(n, H, 64, out3)
            assert list(out3) == [n * H, 256, plan.tfs_lds(64)]                 # one workgroup per (row, head)
            for lens in ([1], [1, 2, 7], [255, 256, 257], [300, 1], [4096]):
                plan.tfs_extend_launch(n, H, max(lens), 64, out4)
                gx, gy, block, lds = list(out4)
                assert (gx, block, lds) == (n * H, 256, plan.tfs_lds(64)) and gy == min(max(lens), 256)
                for ln in lens:                                                 # workgroup y takes queries y, y + gy, ..
                    assert sorted(i for y in range(gy) for i in range(y, ln, gy)) == list(range(ln))


def test_split_ok_is_the_rule_it_states(plan):
    for hd in range(1, 300):
        for dtype, esz in (("f32", 4), ("f16", 2), ("bf16", 2)):
            ve = 16 // esz
            lps = hd // ve
            want = hd % ve == 0 and lps <= 64 and lps & (lps - 1) == 0
            assert bool(plan.tfs_ok(hd, esz)) == want == sb.step_split_ok(hd, dtype), (hd, esz)
            if want:
                assert plan.tfs_vec_ok(hd, esz) and plan.tfs_lanes(hd, esz) == lps
    for hd in (8, 32, 64, 128):
        assert plan.tfs_ok(hd, 4) and plan.tfs_ok(hd, 2)
    assert not plan.tfs_ok(6, 4) and not plan.tfs_ok(6, 2) and not plan.tfs_ok(96, 2) and not plan.tfs_ok(0, 4)


def test_attention_checks(plan):
    bad, mp = C.c_int(-1), C.c_int(-1)

    def chk(tracks, capacity, window, max_tokens, n, L, lengths):
        arr = None if lengths is None else (C.c_int * len(lengths))(*lengths)
        return plan.tfs_check_attention(tracks, capacity, window, max_tokens, n, L, arr, C.byref(bad), C.byref(mp))

    assert chk(3, 8, 0, 64, 0, 4, None) == COUNT and chk(3, 8, 0, 64, 4, 4, None) == COUNT and chk(3, 8, 0, 2, 3, 4, None) == COUNT
    assert chk(3, 8, 0, 64, 2, 4, [4, 0]) == LENGTH and bad.value == 1
    assert chk(3, 8, 0, 64, 2, 4, [5, 1]) == LENGTH and bad.value == 0
    assert chk(3, 8, 0, 64, 2, 9, [8, 9]) == LENGTH and bad.value == 1          # a linear state: above capacity
    assert chk(3, 8, 0, 64, 2, 9, [8, 1]) == OK and mp.value == 7
    assert chk(3, 8, 5, 64, 2, 40, [40, 3]) == OK and mp.value == 4             # a ring takes any length; min(len, W) - 1
    assert chk(3, 8, 5, 64, 3, 2, None) == OK and mp.value == 1


# ---- 2. under the sanitizers ------------------------------------------------------------------------------------------------------------
def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """the planner once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_split_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_SPLIT_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_split.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "tfs_selfcheck = 0" in r.stdout


# ---- 3. the bound against the emulation and its broken copies -----------------------------------------------------------------------------
def _shapes():
    """(n, L, H, hd, lengths, W, capacity) of every launch of the GPU tests"""
    out = [(n, L, H, hd, None, 0, None) for n, L, H, hd in sb.CASES]
    out.append((*sb.RAGGED[0], tuple(sb.RAGGED[1]), 0, None))
    n, L, H, hd, W, caps = sb.WINDOW_CASE
    out += [(n, L, H, hd, None, W, c) for c in caps]
    return out


DTYPES = ["f32", "f16", "bf16"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_bound_passes_the_emulation(dtype):
    worst = 0.0
    for n, L, H, hd, lengths, W, cap in _shapes():
        qkv = sb.make_qkv(n, L, H, hd, dtype)
        ref, bound = sb.reference(n, L, H, hd, dtype, lengths, W)
        r, where = sb.ratio(sb.emulate(qkv, H, dtype, lengths, W, cap), ref, bound)
        print(f"{dtype} n={n} L={L} H={H} hd={hd} lengths={lengths} W={W} cap={cap}: max |err| / bound = {r:.3f} at {where} (headroom {1 / max(r, 1e-30):.1f}x)")
        assert r <= 1.0, (dtype, n, L, H, hd, lengths, W, cap, r, where)
        worst = max(worst, r)
    assert worst > 0.0


def test_the_ring_capacity_is_invisible_to_the_emulation():
    n, L, H, hd, W, caps = sb.WINDOW_CASE
    qkv = sb.make_qkv(n, L, H, hd, "f32")
    a, b = (sb.emulate(qkv, H, "f32", None, W, c) for c in caps)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("mutation", sb.MUTATIONS)
def test_every_broken_copy_exceeds_the_bound(mutation, dtype):
    caught = []
    for n, L, H, hd, lengths, W, cap in _shapes():
        qkv = sb.make_qkv(n, L, H, hd, dtype)
        ref, bound = sb.reference(n, L, H, hd, dtype, lengths, W)
        r, _ = sb.ratio(sb.emulate(qkv, H, dtype, lengths, W, cap, mutation=mutation), ref, bound)
        print(f"{mutation} {dtype} n={n} L={L} H={H} hd={hd} W={W} cap={cap}: max |err| / bound = {r:.3g}")
        if r > 1.0:
            caught.append((n, L, H, hd, W, cap))
    assert caught, f"{mutation} in {dtype} stays within the bound at every shape"


# ---- 4. the C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_refuse_null():
    from flope_amd import _lib
    lib = _lib.load()
    for name in ("flope_tf_stream_step_plan", "flope_tf_stream_attention"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.flope_tf_stream_step_plan(None) == _lib.EINVAL
    assert b"NULL stream state" in lib.flope_tf_last_error(None)
    assert lib.flope_tf_stream_attention(None, None, 1, 1, None, None, None) == _lib.EINVAL
    assert (_lib.TF_STEP_ROW, _lib.TF_STEP_SPLIT) == (0, 1)
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert "int flope_tf_stream_step_plan(flope_tf_stream s);" in header
    assert "int flope_tf_stream_attention(flope_tf_stream s, const void* qkv_dev, int n, int seq_len, const int* lengths_host, void* att_dev, void* stream);" in header
    assert "#define FLOPE_TF_STEP_ROW         0" in header and "#define FLOPE_TF_STEP_SPLIT       1" in header
