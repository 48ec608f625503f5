"""The streaming forward of the encoder (flope_tf_stream_*) without a device: the planner header
flope_amd/csrc/tf_encoder_stream.h through tests/host_harness/harness_tf_stream.cpp against brute force --

  1. the LDS figure of tf_attn_step covers 4 (pos + 1) floats at every position up to the limit, and the constexpr capacity limit is
     the largest capacity whose figure fits (and at least 4096);
  2. every refusal of step / prefill / reset names the right index and moves nothing; an accepted call advances exactly the named
     tracks and its table holds (track, position) per row;
  3. the launches of the two kernels cover their work, and the 16-byte-vector rules are the divisibility they state;
  4. the same once more in a stand-alone program under AddressSanitizer + UBSan;
  5. the C-ABI: _lib.SIGNATURES holds the new symbols (tests/test_host.py holds the header to them), and without a device the
     constructor already fails, so open_stream is unreachable.
"""
import ctypes as C
import os
import random
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, COUNT, RANGE, DUPLICATE, FULL, LENGTH, OPEN = 0, -1, -2, -3, -4, -5, -6


@pytest.fixture(scope="module")
def plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_stream.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_stream.so"])
    lib = C.CDLL(path)
    lib.tfs_step_lds.restype = lib.tfs_lds_max.restype = C.c_longlong
    return lib


def _ints(vals):
    return None if vals is None else (C.c_int * len(vals))(*vals)


def _step(plan, pos, capacity, max_tokens, rows, n=None):
    """one call on the positions `pos` (a list, updated in place) -> (code, bad, max_pos, table)"""
    tracks = len(pos)
    n = (len(rows) if rows is not None else tracks) if n is None else n
    p, tab, bad, mp = _ints(pos), (C.c_int * (2 * max(tracks, 1)))(), C.c_int(-7), C.c_int(-7)
    rc = plan.tfs_step(p, tracks, capacity, max_tokens, n, _ints(rows), tab, C.byref(bad), C.byref(mp))
    pos[:] = list(p)
    return rc, bad.value, mp.value, list(tab[:2 * n]) if rc == OK else None


def _brute_step(pos, capacity, max_tokens, rows, n):
    """the issue's rules in plain words -> (code, bad)"""
    tracks = len(pos)
    if n < 1 or n > min(tracks, max_tokens) or (rows is None and n != tracks):
        return COUNT, -1
    named = list(range(tracks)) if rows is None else rows[:n]
    for r, t in enumerate(named):
        if not 0 <= t < tracks:
            return RANGE, r
        if t in named[:r]:
            return DUPLICATE, r
    for r, t in enumerate(named):
        if pos[t] >= capacity:
            return FULL, r
    return OK, -1


# ---- 1. LDS and the capacity limit ------------------------------------------------------------------------------------------------------
def test_lds_figure_and_capacity_limit(plan):
    limit, lds_max = plan.tfs_max_capacity(), plan.tfs_lds_max()
    assert limit >= 4096 and lds_max >= 64 * 1024
    for p in range(limit):
        assert 4 * (p + 1) * 4 <= plan.tfs_step_lds(p) <= lds_max, p         # 4 waves x (pos + 1) floats
    assert plan.tfs_step_lds(limit - 1) <= lds_max < plan.tfs_step_lds(limit)  # the largest capacity whose last position fits
    assert plan.tfs_check_open(1, limit) == OK and plan.tfs_check_open(1, limit + 1) == OPEN
    assert plan.tfs_check_open(1, 1) == OK and plan.tfs_check_open(1, 0) == OPEN and plan.tfs_check_open(0, 1) == OPEN and plan.tfs_check_open(-3, 4) == OPEN
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert f"capacity <= {limit} (kTfStreamMaxCapacity" in header


# ---- 2. the argument checks -------------------------------------------------------------------------------------------------------------
def test_step_against_brute_force(plan):
    rng = random.Random(5)
    for trial in range(3000):
        tracks, capacity = rng.randint(1, 7), rng.randint(1, 4)
        max_tokens = rng.choice([1, 2, tracks, tracks + 3])
        pos = [rng.randint(0, capacity) for _ in range(tracks)]
        kind = rng.random()
        if kind < 0.2:
            rows, n = None, rng.choice([tracks, tracks, tracks - 1, tracks + 1, 0])
        else:
            n = rng.randint(0, tracks + 1)
            pool = list(range(-1, tracks + 1)) if kind < 0.5 else list(range(tracks))
            rows = [rng.choice(pool) for _ in range(n)] if kind < 0.7 else (rng.sample(range(tracks), min(n, tracks)) + [0] * max(0, n - tracks))
        before = list(pos)
        want, wbad = _brute_step(before, capacity, max_tokens, rows, n)
        rc, bad, mp, tab = _step(plan, pos, capacity, max_tokens, rows, n)
        assert rc == want, (trial, before, capacity, max_tokens, rows, n)
        if rc != OK:
            assert pos == before and (bad == wbad), (trial, rc, bad, wbad)       # nothing moves; the index named is the first offender
            continue
        named = list(range(tracks)) if rows is None else rows[:n]
        assert tab == [v for t in named for v in (t, before[t])]
        assert mp == max(before[t] for t in named)
        assert pos == [p + (t in named) for t, p in enumerate(before)]           # exactly the named tracks, by one


def test_each_refusal_of_step_names_its_row(plan):
    pos = [0, 2, 1, 2]
    assert _step(plan, pos, 2, 64, [0, 2, 1])[:2] == (FULL, 2)
    assert _step(plan, pos, 2, 64, None)[:2] == (FULL, 1)
    assert _step(plan, pos, 2, 64, [2, 0, 2])[:2] == (DUPLICATE, 2)
    assert _step(plan, pos, 2, 64, [2, 4, 4])[:2] == (RANGE, 1)
    assert _step(plan, pos, 2, 64, [-1])[:2] == (RANGE, 0)
    assert _step(plan, pos, 2, 64, [])[0] == COUNT and _step(plan, pos, 2, 64, [0, 1, 2, 3, 0])[0] == COUNT
    assert _step(plan, pos, 2, 1, [0, 2])[0] == COUNT                            # n > max_tokens
    assert _step(plan, pos, 2, 64, None, n=3)[0] == COUNT                        # a NULL list takes every track
    assert pos == [0, 2, 1, 2]
    rc, _, mp, tab = _step(plan, pos, 2, 64, [2, 0])
    assert (rc, mp, tab, pos) == (OK, 1, [2, 1, 0, 0], [1, 2, 2, 2])


def test_prefill_and_reset_checks(plan):
    def prefill(pos, capacity, seq_len, lengths, rows, n):
        p, bad = _ints(pos), C.c_int(-7)
        rc = plan.tfs_prefill(p, len(pos), capacity, n, seq_len, _ints(lengths), _ints(rows), C.byref(bad))
        pos[:] = list(p)
        return rc, bad.value

    pos = [5, 5, 5, 5]
    assert prefill(pos, 6, 8, [6, 7, 8], [3, 1, 0], 3) == (LENGTH, 1) and pos == [5, 5, 5, 5]
    assert prefill(pos, 6, 7, None, [3, 1], 2) == (LENGTH, 0)
    assert prefill(pos, 6, 6, [1, 2], [1, 1], 2) == (DUPLICATE, 1)
    assert prefill(pos, 6, 6, [1, 2], [1, 4], 2) == (RANGE, 1)
    assert prefill(pos, 6, 6, [1, 2, 3], None, 3)[0] == COUNT and prefill(pos, 6, 6, [1] * 5, [0, 1, 2, 3, 0], 5)[0] == COUNT
    assert prefill(pos, 6, 6, [], [], 0)[0] == COUNT and pos == [5, 5, 5, 5]
    assert prefill(pos, 6, 8, [6, 1], [3, 1], 2) == (OK, -1)
    assert pos == [5, 1, 5, 6]                                                   # the named tracks hold their lengths, the others what they held
    assert prefill(pos, 6, 4, None, None, 4)[0] == OK and pos == [4, 4, 4, 4]

    def reset(tracks, rows, n):
        bad = C.c_int(-7)
        return plan.tfs_check_reset(tracks, n, _ints(rows), C.byref(bad)), bad.value

    assert reset(4, None, 0)[0] == OK and reset(4, None, 99)[0] == OK            # NULL: every track
    assert reset(4, [3, 0, 3], 3)[0] == OK                                       # a track named twice is reset once
    assert reset(4, [3, 4], 2) == (RANGE, 1) and reset(4, [-1], 1) == (RANGE, 0) and reset(4, [], 0)[0] == COUNT


# ---- 3. launches and vector rules -------------------------------------------------------------------------------------------------------
def test_launches_cover_their_work(plan):
    out = (C.c_longlong * 3)()
    for n in (1, 2, 3, 5, 256, 4096):
        for H in (1, 2, 5, 6):
            for mp in (0, 1, 63, 64, 511, 4095):
                plan.tfs_step_launch(n, H, mp, out)
                grid, block, lds = list(out)
                assert block == 256 and (grid - 1) * 4 < n * H <= grid * 4          # one wave per (row, head), four per workgroup
                assert lds == plan.tfs_step_lds(mp) == 16 * (mp + 1)
    for n, L, units in ((1, 1, 1), (3, 50, 64), (6, 15, 60), (256, 257, 192)):
        plan.tfs_cache_fill_launch(n, L, units, out)
        grid, block, lds = list(out)
        assert block == 256 and lds == 0 and (grid - 1) * 256 < n * L * units <= grid * 256
    assert plan.tfs_vec(4) == 4 and plan.tfs_vec(2) == 8
    for esz in (2, 4):
        for dim in range(1, 200):
            assert plan.tfs_step_vec_ok(dim, esz) == plan.tfs_cache_fill_vec_ok(dim, esz) == int(dim * esz % 16 == 0)


# ---- 4. under the sanitizers ------------------------------------------------------------------------------------------------------------
def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """the planner once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_stream_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_STREAM_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_stream.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "tfs_selfcheck = 0" in r.stdout


# ---- 5. the C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_bound_and_the_constructor_fails_without_a_device():
    from flope_amd import _lib
    lib = _lib.load()
    for name in ("flope_tf_stream_open", "flope_tf_stream_close", "flope_tf_stream_reset", "flope_tf_stream_position", "flope_tf_stream_step",
                 "flope_tf_stream_prefill"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    out = C.c_void_p()
    assert lib.flope_tf_stream_open(None, 1, 1, C.byref(out)) == _lib.EINVAL and not out.value      # no handle, no state
    assert lib.flope_tf_stream_step(None, None, 1, None, None, None) == _lib.EINVAL
    assert lib.flope_tf_stream_close(None) == 0
    if not torch.cuda.is_available():
        from flope_amd.tf_encoder import TransformerEncoder
        with pytest.raises(RuntimeError):
            TransformerEncoder(16, 32, 9, 4, 2, 64)
