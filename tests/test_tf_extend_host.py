"""flope_tf_stream_extend without a device: the planner in flope_amd/csrc/tf_encoder_stream.h through
tests/host_harness/harness_tf_extend.cpp against brute force --

  1. a few thousand random extend calls on linear and windowed states: which refusal fires, the index it names and "nothing moved";
     for an accepted call the table, smax, the LDS bytes and the new positions;
  2. for every (pos0, len, capacity, W) of a small range: the append writes exactly the slots of the chunk's last min(len, capacity)
     tokens, each once; behind it every key a later query can see is in its slot; the cached keys a chunk query reads are keys the
     pre-call ring still holds -- with the append behind the attention, and the brute force shows the other order failing at
     capacity == W from len = 2 on;
  3. both launches cover their work for ragged lengths;
  4. the same once more in a stand-alone program under AddressSanitizer + UBSan;
  5. the C-ABI: _lib.SIGNATURES holds the symbol and the entry point refuses NULL.
"""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, COUNT, RANGE, DUPLICATE, FULL, ROOM = 0, -1, -2, -3, -4, -7
V_BATCH, V_LENGTH, V_TOKENS = 99, 98, 97          # tf_varlen_plan's codes as the harness passes them on (+ 100)
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_extend.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_extend.so"])
    lib = C.CDLL(path)
    lib.tfe_lds_max.restype = C.c_longlong
    return lib


def _ints(vals):
    return None if vals is None else (C.c_int * max(len(vals), 1))(*vals)


def _extend(plan, pos, capacity, window, max_tokens, n, seq_len, lengths, rows):
    """one call on the positions `pos` (a list, updated in place) -> (code, bad, smax, table, offsets)"""
    tracks = len(pos)
    p, bad, smax = _ints(pos), C.c_int(-7), C.c_int(-7)
    tab, off = (C.c_int * (2 * max(n, tracks, 1)))(), (C.c_int * (max(n, 0) + 1))()
    rc = plan.tfe_extend(p, tracks, capacity, window, max_tokens, n, seq_len, _ints(lengths), _ints(rows), tab, off, C.byref(bad), C.byref(smax))
    pos[:] = list(p)[:tracks]
    return rc, bad.value, smax.value, (list(tab[:2 * n]) if rc == OK else None), (list(off[:n + 1]) if rc == OK else None)


def _brute(pos, capacity, window, max_tokens, n, seq_len, lengths, rows):
    """the issue's rules in plain words -> (code, bad)"""
    tracks = len(pos)
    if n <= 0:
        return V_BATCH, -1
    lens = [seq_len] * n if lengths is None else lengths
    for b in range(n):
        if not 1 <= lens[b] <= seq_len:
            return V_LENGTH, b
    if sum(lens) > max_tokens:
        return V_TOKENS, -1
    if n > tracks or (rows is None and n != tracks):
        return COUNT, -1
    named = list(range(tracks)) if rows is None else rows
    for b, t in enumerate(named):
        if not 0 <= t < tracks:
            return RANGE, b
        if t in named[:b]:
            return DUPLICATE, b
    for b, t in enumerate(named):
        if window:
            if pos[t] + lens[b] > INT_MAX:
                return FULL, b
        elif pos[t] + lens[b] > capacity:
            return ROOM, b
    return OK, -1


# ---- 1. the argument checks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("windowed", [False, True], ids=["linear", "ring"])
def test_extend_against_brute_force(plan, windowed):
    rng = random.Random(11 + windowed)
    seen = set()
    for trial in range(3000):
        tracks, capacity = rng.randint(1, 6), rng.randint(1, 6)
        window = rng.randint(1, capacity) if windowed else 0
        seq_len = rng.randint(1, 8)
        if windowed:
            pos = [rng.choice([0, rng.randint(0, 20), INT_MAX - rng.randint(0, 9)]) for _ in range(tracks)]
        else:
            pos = [rng.randint(0, capacity) for _ in range(tracks)]
        kind = rng.random()
        if kind < 0.2:
            rows, n = None, rng.choice([tracks, tracks, tracks - 1, tracks + 1, 0])
        else:
            n = rng.randint(0, tracks + 1)
            pool = list(range(-1, tracks + 1)) if kind < 0.4 else list(range(tracks))
            rows = [rng.choice(pool) for _ in range(n)] if kind < 0.5 else (rng.sample(range(tracks), min(n, tracks)) + [0] * max(0, n - tracks))
        r = rng.random()
        if r < 0.25:
            lengths = None
        elif r < 0.4:
            lengths = [rng.randint(0, seq_len + 1) for _ in range(max(n, 0))]
        else:
            lengths = [rng.randint(1, min(seq_len, 3)) for _ in range(max(n, 0))]
        max_tokens = rng.choice([1, 4, 1000, 1000])
        before = list(pos)
        want, wbad = _brute(before, capacity, window, max_tokens, n, seq_len, lengths, rows)
        rc, bad, smax, tab, off = _extend(plan, pos, capacity, window, max_tokens, n, seq_len, lengths, rows)
        args = (trial, before, capacity, window, max_tokens, n, seq_len, lengths, rows)
        assert rc == want, args
        seen.add(rc)
        if rc != OK:
            assert pos == before, args                                           # nothing moves
            if wbad >= 0:
                assert bad == wbad, args                                         # the index named is the first offender
            continue
        lens = [seq_len] * n if lengths is None else lengths
        named = list(range(tracks)) if rows is None else rows
        assert tab == [v for t in named for v in (t, before[t])], args
        assert off == [sum(lens[:b]) for b in range(n + 1)], args
        vis = [min(before[t] + l, window) if window else before[t] + l for t, l in zip(named, lens)]
        assert smax == max(vis), args
        out = (C.c_longlong * 4)()
        plan.tfe_extend_launch(n, 3, max(lens), smax, out)
        assert out[3] == 4 * smax * 4 <= plan.tfe_lds_max(), args                 # 4 waves x smax floats
        want_pos = list(before)
        for t, l in zip(named, lens):
            want_pos[t] += l
        assert pos == want_pos, args                                             # exactly the named tracks, by their lengths
    assert seen >= ({OK, COUNT, RANGE, DUPLICATE, V_BATCH, V_LENGTH, V_TOKENS} | ({FULL} if windowed else {ROOM})), seen


def test_each_refusal_names_its_index(plan):
    pos = [0, 2, 1, 3]
    assert _extend(plan, pos, 3, 0, 64, 3, 2, [1, 2, 2], [0, 2, 1])[:2] == (ROOM, 2)           # 2 + 2 > 3
    assert _extend(plan, pos, 3, 0, 64, 4, 1, None, None)[:2] == (ROOM, 3)                       # a full track takes nothing
    assert _extend(plan, pos, 3, 0, 64, 3, 2, [1, 1, 1], [2, 0, 2])[:2] == (DUPLICATE, 2)
    assert _extend(plan, pos, 3, 0, 64, 3, 2, [1, 1, 1], [2, 4, 4])[:2] == (RANGE, 1)
    assert _extend(plan, pos, 3, 0, 64, 1, 2, [1], [-1])[:2] == (RANGE, 0)
    assert _extend(plan, pos, 3, 0, 64, 5, 2, [1] * 5, [0, 1, 2, 3, 0])[0] == COUNT             # n > tracks
    assert _extend(plan, pos, 3, 0, 64, 3, 2, [1] * 3, None)[0] == COUNT                         # a NULL list takes every track
    assert _extend(plan, pos, 3, 0, 64, 0, 2, [], [])[0] == V_BATCH
    assert _extend(plan, pos, 3, 0, 64, 2, 2, [1, 3], [0, 2])[:2] == (V_LENGTH, 1)
    assert _extend(plan, pos, 3, 0, 64, 2, 2, [0, 1], [0, 2])[:2] == (V_LENGTH, 0)
    assert _extend(plan, pos, 3, 0, 3, 2, 2, [2, 2], [0, 2])[0] == V_TOKENS
    assert _extend(plan, pos, 3, 0, 64, 2, 2, [0, 1], [0, 9])[:2] == (V_LENGTH, 0)               # tf_varlen_plan's checks come first
    assert pos == [0, 2, 1, 3]
    rc, _, smax, tab, off = _extend(plan, pos, 3, 0, 64, 3, 3, [3, 1, 2], [0, 1, 2])             # each filled exactly to capacity
    assert (rc, smax, tab, off, pos) == (OK, 3, [0, 0, 1, 2, 2, 1], [0, 3, 4, 6], [3, 3, 3, 3])
    assert _extend(plan, pos, 3, 0, 64, 1, 1, [1], [1])[:2] == (ROOM, 0)                         # ... and the next call is refused
    # a ring: a chunk longer than the capacity, a position up to INT_MAX, smax bounded by the window
    pos = [5, INT_MAX - 3]
    rc, _, smax, tab, off = _extend(plan, pos, 4, 3, 64, 2, 9, [9, 3], None)
    assert (rc, smax, tab, pos) == (OK, 3, [0, 5, 1, INT_MAX - 3], [14, INT_MAX])
    assert _extend(plan, pos, 4, 3, 64, 2, 1, None, [0, 1])[:2] == (FULL, 1) and pos == [14, INT_MAX]
    pos = [0, 1]
    assert _extend(plan, pos, 8, 5, 64, 2, 2, [2, 1], None)[2] == 2                              # a young track: min(W, pos0 + len)


# ---- 2. the cache rows: what the append writes, what a query reads ----------------------------------------------------------------------
def test_append_rows_and_chunk_keys_exhaustively(plan):
    for capacity in range(1, 9):
        for W in range(0, capacity + 1):
            for pos0 in range(0, 2 * capacity + 2):
                for ln in range(1, 2 * capacity + 3):
                    if W == 0 and pos0 + ln > capacity:
                        continue
                    assert plan.tfe_walk(pos0, ln, capacity, W, 0) == 0, (pos0, ln, capacity, W)
                    # brute force on sets, independent of the harness' walk
                    rows = {}
                    for i in range(ln):
                        if W == 0 or plan.tfe_append_writes(i, ln, capacity):
                            r = plan.tfe_append_slot(pos0, i, capacity) if W else pos0 + i
                            assert 0 <= r < capacity and r not in rows, (pos0, ln, capacity, W, i)
                            rows[r] = pos0 + i
                    last = range(max(0, ln - capacity), ln) if W else range(ln)
                    assert rows == {((pos0 + i) % capacity if W else pos0 + i): pos0 + i for i in last}, (pos0, ln, capacity, W)
                    for i in range(ln):
                        p = pos0 + i
                        lo = max(0, p + 1 - W) if W else 0
                        assert plan.tfe_window_lo(p, W) == lo
                        assert plan.tfe_cached(pos0, lo) == len([j for j in range(lo, p + 1) if j < pos0])
                        assert plan.tfe_chunk0(pos0, lo) == min(j for j in range(lo, p + 1) if j >= pos0) - pos0
                    assert plan.tfe_keys(pos0, ln, W) == max(min(pos0 + i + 1, W) if W else pos0 + i + 1 for i in range(ln))


def test_the_append_in_front_of_the_attention_would_lose_keys(plan):
    """the hazard: with the other order a chunk's earlier query reads a ring row a later token of the same chunk has taken"""
    for capacity in range(2, 9):
        for W in range(1, capacity + 1):
            for pos0 in range(0, 2 * capacity + 2):
                for ln in range(1, 2 * capacity + 3):
                    # in plain words: the first query's first cached key exists and its row is taken by a token of the chunk
                    lo = max(0, pos0 + 1 - W)
                    lost = lo < pos0 and lo + capacity <= pos0 + ln - 1
                    assert plan.tfe_walk(pos0, ln, capacity, W, 1) == (3 if lost else 0), (pos0, ln, capacity, W)
                    if pos0 >= W - 1 and W >= 2:
                        assert lost == (ln >= capacity - W + 2)
    for capacity in range(2, 9):                                                 # capacity == W: every chunk of two tokens
        for ln in range(2, 12):
            assert plan.tfe_walk(capacity, ln, capacity, capacity, 1) == 3 and plan.tfe_walk(capacity, ln, capacity, capacity, 0) == 0
        assert plan.tfe_walk(capacity, 1, capacity, capacity, 1) == 0


# ---- 3. launches ------------------------------------------------------------------------------------------------------------------------
def test_launches_cover_their_work(plan):
    out = (C.c_longlong * 4)()
    for n in (1, 2, 3, 256):
        for H in (1, 2, 5, 6):
            for lens in ([1], [1, 2, 7, 3], [4], [5, 1], [255, 256, 257], [300, 1], [4096]):
                for smax in (1, 64, 512, 4096):
                    plan.tfe_extend_launch(n, H, max(lens), smax, out)
                    gx, gy, block, lds = list(out)
                    assert (gx, block, lds) == (n * H, 256, 16 * smax) and 1 <= gy <= 64
                    for ln in lens:                                              # wave w of workgroup y starts at query 4 y + w and strides 4 gy
                        got = sorted(i for y in range(gy) for w in range(4) for i in range(4 * y + w, ln, 4 * gy))
                        assert got == list(range(ln)), (lens, gy)
                    assert gy == min(-(-max(lens) // 4), 64)
    out3 = (C.c_longlong * 3)()
    for n, L, units in ((1, 1, 1), (3, 50, 64), (6, 15, 60), (256, 32, 96)):
        plan.tfe_append_launch(n, L, units, out3)
        grid, block, lds = list(out3)
        assert block == 256 and lds == 0 and (grid - 1) * 256 < n * L * units <= grid * 256


# ---- 4. under the sanitizers ------------------------------------------------------------------------------------------------------------
def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """the planner once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_extend_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_EXTEND_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_extend.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "tfe_selfcheck = 0" in r.stdout


# ---- 5. the C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_bound_and_refuses_null():
    from flope_amd import _lib
    lib = _lib.load()
    assert "flope_tf_stream_extend" in _lib.SIGNATURES and hasattr(lib, "flope_tf_stream_extend")
    assert _lib.SIGNATURES["flope_tf_stream_extend"] == _lib.SIGNATURES["flope_tf_stream_prefill"]
    assert lib.flope_tf_stream_extend(None, None, 1, 1, None, None, None, None) == _lib.EINVAL
    assert b"NULL stream state" in lib.flope_tf_last_error(None)
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert "int flope_tf_stream_extend(flope_tf_stream s, const float* x_dev, int n, int seq_len, const int* lengths_host, const int* tracks_host," in header
