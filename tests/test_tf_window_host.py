"""Sliding-window causal attention and the ring cache of a windowed stream state without a device:

  1. the fixture recorded from the reference module under the banded mask (tests/golden/tf_window_fixture.npz; float and bool mask,
     W = 4 and W = L) pins the test-side fp64 restatement (tests/tf_attn_window_bound.py), and W = L is the causal fixture;
  2. the planner functions the kernels and the host call (flope_amd/csrc/tf_attn_plan.h: tf_window_lo; tf_encoder_stream.h: the slot,
     the rows a fill writes, the two row runs of a step, the windowed checks) through tests/host_harness/harness_tf_window.cpp against
     brute force for every L <= 300 and W <= L + 2, and on 3,000 random call sequences against a model of the ring;
  3. the same once more in a stand-alone program under AddressSanitizer + UBSan;
  4. the Python mask helper _mask_window;
  5. the C-ABI: _lib.SIGNATURES holds the new symbol, NULL arguments are refused.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import tf_attn_causal_bound as CB
import tf_attn_window_bound as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMAX = 300
INT_MAX = 2 ** 31 - 1
OK, COUNT, RANGE, DUPLICATE, FULL, LENGTH, OPEN = 0, -1, -2, -3, -4, -5, -6


# ---- 1. the reference's banded runs -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    path = os.path.join(ROOT, "tests", "golden", "tf_window_fixture.npz")
    assert os.path.getsize(path) < 100 * 1024
    f = np.load(path, allow_pickle=False)
    sd = {k[4:]: f[k] for k in f.files if k.startswith("sd::")}
    return f["x"], int(f["W"]), f["y_window"], f["y_window_bool"], f["y_window_L"], sd


def test_fixture_pins_the_window_restatement(fixture):
    x, W, y, yb, yl, sd = fixture
    assert x.shape == (6, 15, 16) and y.shape == yb.shape == yl.shape == (6, 15, 9) and W == 4
    e = float(np.abs(WB.window_forward(sd, x, W) - y).max())
    eb = float(np.abs(WB.window_forward(sd, x, W) - yb).max())
    print(f"fp64 window restatement vs the reference under the banded mask: float {e:.2e}, bool {eb:.2e}")
    assert e < 1e-5 and eb < 1e-5
    away = float(np.abs(CB.causal_forward(sd, x, 4) - y).max())
    print(f"(the causal restatement is {away:.2f} away: the fixture is a windowed one)")
    assert away > 0.1


def test_window_L_is_the_causal_fixture(fixture):
    x, _, _, _, yl, sd = fixture
    c = np.load(os.path.join(ROOT, "tests", "golden", "tf_causal_fixture.npz"), allow_pickle=False)
    assert np.array_equal(c["x"], x) and np.array_equal(c["y_causal"], yl)          # the reference itself: a band of W = L is the causal mask
    for W in (15, 16, 0):
        assert float(np.abs(WB.window_forward(sd, x, W) - yl).max()) < 1e-5
    assert np.array_equal(WB.window_forward(sd, x, 15), CB.causal_forward(sd, x, 4))


def test_prefix_and_ragged_properties_of_the_restatement(fixture):
    x, W, _, _, _, sd = fixture
    full = WB.window_forward(sd, x, W)
    for n in (1, 4, 5, 14):
        assert float(np.abs(WB.window_forward(sd, x[:, :n], W) - full[:, :n]).max()) < 1e-12
    lengths = [15, 1, 7, 12, 3, 15]
    rag = WB.window_forward(sd, x, W, lengths)
    for b, n in enumerate(lengths):
        assert float(np.abs(rag[b, :n] - full[b, :n]).max()) < 1e-12 and np.array_equal(rag[b, n:], np.broadcast_to(sd["out_layer.bias"], (15 - n, 9)))
    # row t depends on rows t - 2 (W - 1) .. t only (two layers): the window has forgotten what lies before
    x2 = x.copy()
    x2[:, :5] = 7.0
    assert float(np.abs(WB.window_forward(sd, x2, W)[:, 11:] - full[:, 11:]).max()) < 1e-12


# ---- 2. the planner ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_window.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_window.so"])
    lib = C.CDLL(path)
    lib.tfw_step_lds.restype = lib.tfw_lds_max.restype = C.c_longlong
    return lib


def _ints(vals):
    return None if vals is None else (C.c_int * len(vals))(*vals)


def test_lo_against_brute_force(plan):
    lo, keys = (C.c_int * LMAX)(), (C.c_int * LMAX)()
    i = np.arange(LMAX)
    for L in range(1, LMAX + 1):
        for W in range(0, L + 3):
            plan.tfw_lo_table(L, W, lo, keys)
            want = np.maximum(0, i[:L] + 1 - W) if W > 0 else np.zeros(L, dtype=np.int64)
            assert np.array_equal(np.frombuffer(lo, dtype=np.int32)[:L], want), (L, W)
            assert np.array_equal(np.frombuffer(keys, dtype=np.int32)[:L], i[:L] - want + 1), (L, W)
    for p in (INT_MAX - 1, INT_MAX - 2, 2 ** 30):
        for W in (1, 2, 256, 4096):
            assert plan.tfw_lo(p, W) == p + 1 - W and plan.tfw_keys(p, W) == W
        assert plan.tfw_lo(p, 0) == 0


def test_slot_and_fill_against_brute_force(plan):
    row = (C.c_int * (LMAX + 2))()
    for cap in list(range(1, 40)) + [63, 64, 65, 96, 255, 256, 300, 4096]:
        for p in list(range(0, 3 * cap + 2, max(1, cap // 7))) + [INT_MAX - 1, INT_MAX]:
            assert plan.tfw_slot(p, cap) == p % cap
    for L in range(1, LMAX + 1):
        for cap in (1, 2, 3, 4, 6, 7, 15, 16, 64, 70, 96, L - 1, L, L + 1):
            if cap < 1:
                continue
            plan.tfw_fill_table(L, cap, row)
            got = list(row[:L])
            kept = list(range(max(0, L - cap), L))                              # exactly the last min(len, capacity) tokens ...
            assert [i for i in range(L) if got[i] >= 0] == kept, (L, cap)
            assert [got[i] for i in kept] == [i % cap for i in kept] and len(set(got[i] for i in kept)) == len(kept), (L, cap)   # ... each row once
    assert plan.tfw_fill_writes(-1, 5, 8) == 0 and plan.tfw_fill_writes(5, 5, 8) == 0


def test_open_check(plan):
    limit = plan.tfw_max_capacity()
    assert plan.tfw_check_open(1, limit, limit) == OK and plan.tfw_check_open(1, limit + 1, limit) == OPEN
    assert plan.tfw_check_open(3, 8, 8) == OK and plan.tfw_check_open(3, 8, 1) == OK
    for tracks, cap, W in ((3, 8, 9), (3, 8, 0), (3, 8, -1), (0, 8, 4), (3, 0, 0), (3, 0, 1)):
        assert plan.tfw_check_open(tracks, cap, W) == OPEN, (tracks, cap, W)
    # the score rows of the widest window fit what a launch gets
    assert plan.tfw_step_lds(limit - 1) <= plan.tfw_lds_max()


def test_step_rows_and_overwrite_against_brute_force(plan):
    """every step of a track: the rows read hold keys lo .. p - 1 in key order, and the row overwritten is outside the window"""
    buf = (C.c_int * 4096)()
    for cap in (1, 2, 3, 4, 6, 7, 16, 64, 70, 96):
        for W in sorted({1, 2, 3, cap // 2, cap - 1, cap} - {0}):
            if W > cap:
                continue
            ring = {}
            for p in range(0, 3 * cap + 70):
                lo = max(0, p + 1 - W)
                assert ring.get(p % cap, -1) < lo, (cap, W, p)                     # what the step overwrites no query of this call sees
                ring[p % cap] = p
                m = plan.tfw_step_rows(p, W, cap, buf)
                rows = list(buf[:m])
                assert m == p - lo and [ring[r] for r in rows] == list(range(lo, p)), (cap, W, p)
                assert rows == [plan.tfw_score_row(p, W, cap, j) for j in range(m)]
                slo = lo % cap
                assert plan.tfw_run0(slo, m, cap) == min(m, cap - slo)
    for cap, W, start in ((4096, 4096, INT_MAX - 5000), (256, 256, INT_MAX - 300), (96, 70, INT_MAX - 400), (6, 4, 0), (7, 7, 50)):
        assert plan.tfw_selfcheck_ring(cap, W, start, min(399, INT_MAX - 1 - start)) == 0, (cap, W, start)


def _step(plan, pos, W, max_tokens, rows, n=None):
    tracks = len(pos)
    n = (len(rows) if rows is not None else tracks) if n is None else n
    p, tab, bad, mp = _ints(pos), (C.c_int * (2 * max(tracks, 1)))(), C.c_int(-7), C.c_int(-7)
    rc = plan.tfw_step(p, tracks, W, max_tokens, n, _ints(rows), tab, C.byref(bad), C.byref(mp))
    pos[:] = list(p)
    return rc, bad.value, mp.value, list(tab[:2 * n]) if rc == OK else None


def _prefill(plan, pos, seq_len, lengths, rows, n):
    p, bad = _ints(pos), C.c_int(-7)
    rc = plan.tfw_prefill(p, len(pos), n, seq_len, _ints(lengths), _ints(rows), C.byref(bad))
    pos[:] = list(p)
    return rc, bad.value


def _brute_rows(tracks, limit, rows, n):
    if n < 1 or n > min(tracks, limit) or (rows is None and n != tracks):
        return COUNT, -1
    named = list(range(tracks)) if rows is None else rows[:n]
    for r, t in enumerate(named):
        if not 0 <= t < tracks:
            return RANGE, r
        if t in named[:r]:
            return DUPLICATE, r
    return OK, -1


def test_random_call_sequences_on_a_model_of_the_ring(plan):
    """3,000 sequences of step / prefill / reset: every refusal names its index and moves nothing; after every accepted call the
    positions, the table, max_pos and LDS are the brute-force ones, and the rows a step reads hold exactly its window's keys"""
    rng = random.Random(26)
    buf, frow = (C.c_int * 64)(), (C.c_int * 64)()
    for trial in range(3000):
        tracks, cap = rng.randint(1, 5), rng.randint(1, 7)
        W = rng.randint(1, cap)
        max_tokens = rng.choice([1, 2, tracks, tracks + 3])
        pos = [0] * tracks
        ring = [dict() for _ in range(tracks)]                                  # row -> absolute position held
        if rng.random() < 0.1:
            pos[rng.randrange(tracks)] = INT_MAX                                # a full track: holds nothing the model reads
        for call in range(rng.randint(3, 14)):
            kind = rng.random()
            before = list(pos)
            if kind < 0.15:                                                     # reset
                rows = None if rng.random() < 0.3 else [rng.randint(-1, tracks) for _ in range(rng.randint(0, 3))]
                bad = C.c_int(-7)
                rc = plan.tfw_check_reset(tracks, 0 if rows is None else len(rows), _ints(rows), C.byref(bad))
                if rows is None:
                    want = (OK, -1)
                elif not rows:
                    want = (COUNT, -1)
                else:
                    off = [r for r, t in enumerate(rows) if not 0 <= t < tracks]
                    want = (RANGE, off[0]) if off else (OK, -1)
                assert (rc, bad.value) == want, (trial, call)
                if rc == OK:
                    for t in (range(tracks) if rows is None else rows):
                        pos[t] = 0
                        ring[t] = {}                                            # stale rows: the model forgets them, so a read of one fails below
                continue
            n = rng.randint(0, tracks + 1)
            rows = None if rng.random() < 0.2 else ([rng.randint(-1, tracks) for _ in range(n)] if rng.random() < 0.3
                                                    else rng.sample(range(tracks), min(n, tracks)))
            if rows is not None:
                n = len(rows) if rng.random() < 0.9 else n
                rows = rows + [0] * max(0, n - len(rows))
            elif rng.random() < 0.7:
                n = tracks
            if kind < 0.4:                                                      # prefill: any length, longer than the capacity included
                seq_len = rng.randint(1, 20)
                lengths = None if rng.random() < 0.3 else [rng.randint(1, seq_len) for _ in range(max(n, 0))]
                want, wbad = _brute_rows(tracks, tracks, rows, n)
                rc, bad = _prefill(plan, pos, seq_len, lengths, rows, n)
                assert (rc, bad) == (want, wbad), (trial, call, rows, n)
                if rc != OK:
                    assert pos == before
                    continue
                named = list(range(tracks)) if rows is None else rows[:n]
                for b, t in enumerate(named):
                    ln = seq_len if lengths is None else lengths[b]
                    assert pos[t] == ln
                    ring[t] = {}
                    plan.tfw_fill_table(ln, cap, frow)
                    for i in range(ln):
                        if frow[i] >= 0:
                            ring[t][frow[i]] = i
                assert [pos[t] for t in range(tracks) if t not in named] == [before[t] for t in range(tracks) if t not in named]
                continue
            want, wbad = _brute_rows(tracks, max_tokens, rows, n)                # step
            if want == OK:
                named = list(range(tracks)) if rows is None else rows[:n]
                full = [r for r, t in enumerate(named) if before[t] == INT_MAX]
                if full:
                    want, wbad = FULL, full[0]
            rc, bad, mp, tab = _step(plan, pos, W, max_tokens, rows, n)
            assert (rc, bad) == (want, wbad), (trial, call, before, rows, n)
            if rc != OK:
                assert pos == before
                continue
            assert tab == [v for t in named for v in (t, before[t])]
            assert mp == max(min(before[t], W - 1) for t in named)              # the largest visible key count - 1 ...
            assert plan.tfw_step_lds(mp) == 16 * (mp + 1) <= 16 * W             # ... sizes LDS: bounded by W, not by the track's age
            assert pos == [p + (t in named) for t, p in enumerate(before)]
            for t in named:
                p = before[t]
                lo = max(0, p + 1 - W)
                assert ring[t].get(p % cap, -1) < lo
                ring[t][p % cap] = p
                m = plan.tfw_step_rows(p, W, cap, buf)
                assert [ring[t][r] for r in buf[:m]] == list(range(lo, p)), (trial, call, t, p)


def test_each_refusal_names_its_row_and_int_max_is_the_only_full(plan):
    pos = [0, 10 ** 9, INT_MAX, 5]
    assert _step(plan, pos, 3, 64, [0, 2, 1])[:2] == (FULL, 1)
    assert _step(plan, pos, 3, 64, None)[:2] == (FULL, 2)
    assert _step(plan, pos, 3, 64, [3, 0, 3])[:2] == (DUPLICATE, 2)
    assert _step(plan, pos, 3, 64, [3, 4])[:2] == (RANGE, 1)
    assert _step(plan, pos, 3, 64, [])[0] == COUNT and _step(plan, pos, 3, 1, [0, 1])[0] == COUNT
    assert pos == [0, 10 ** 9, INT_MAX, 5]
    rc, _, mp, tab = _step(plan, pos, 3, 64, [1, 0])
    assert (rc, mp, tab, pos) == (OK, 2, [1, 10 ** 9, 0, 0], [1, 10 ** 9 + 1, INT_MAX, 5])       # far past any capacity: not full
    pos = [INT_MAX - 1]
    assert _step(plan, pos, 3, 64, None)[0] == OK and pos == [INT_MAX] and _step(plan, pos, 3, 64, None)[:2] == (FULL, 0)
    pos = [1, 1]
    assert _prefill(plan, pos, 500, [500, 3], [1, 0], 2) == (OK, -1) and pos == [3, 500]         # no capacity in this check at all
    assert _prefill(plan, pos, 5, None, [1, 1], 2) == (DUPLICATE, 1) and _prefill(plan, pos, 5, None, [2], 1) == (RANGE, 0) and pos == [3, 500]


# ---- 3. under the sanitizers ------------------------------------------------------------------------------------------------------
def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """the planner once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_window_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_WINDOW_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_window.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "tfw_selfcheck = 0" in r.stdout


# ---- 4. the mask helper -----------------------------------------------------------------------------------------------------------
def test_mask_window_accepts_what_it_should():
    from flope_amd import tf_encoder as E
    L = 7
    sub = torch.nn.Transformer.generate_square_subsequent_mask(L)
    above = torch.ones(L, L, dtype=torch.bool).triu(1)
    # everything _mask_is_causal accepts, with its answer
    for m in (None, torch.zeros(L, L), torch.zeros(L, L, dtype=torch.bool)):
        assert E._mask_window(m, L) == (False, 0) and E._mask_is_causal(m, L) is False
    for m in (sub, sub.double(), sub.half(), above):
        assert E._mask_window(m, L) == (True, 0) and E._mask_is_causal(m, L) is True
    assert E._mask_window(torch.zeros(1, 1), 1) == (False, 0)
    # the banded mask, every W in 1 .. L - 1, float and bool
    for W in range(1, L):
        for dt in (torch.float32, torch.float64, torch.float16, torch.bool):
            assert E._mask_window(WB.band_mask(L, W, dt), L) == (True, W), (W, dt)
        with pytest.raises(ValueError):
            E._mask_is_causal(WB.band_mask(L, W), L)                            # the old helper keeps refusing it
    assert E._mask_window(WB.band_mask(L, L), L) == (True, 0) and E._mask_window(WB.band_mask(L, L + 3, torch.bool), L) == (True, 0)


def test_mask_window_refuses_what_it_should():
    from flope_amd import tf_encoder as E
    L = 7
    sub = torch.nn.Transformer.generate_square_subsequent_mask(L)
    above = torch.ones(L, L, dtype=torch.bool).triu(1)
    hole = above.clone()
    hole[4, 2] = True
    fhole = sub.clone()
    fhole[2, 5] = 0.0
    # what tests/test_tf_causal_host.py holds _mask_is_causal to refuse, with the same entries named
    for m, pat in ((hole, r"mask\[4, 2\]"), (fhole, r"mask\[2, 5\]"), (torch.ones(L, L, dtype=torch.bool).triu(2), r"mask\[0, 1\]"),
                   (torch.ones(L, L, dtype=torch.bool).triu(0), r"mask\[0, 0\]"), (above.t(), r"mask\[0, 1\]"), (sub.t(), r"mask\[0, 1\]"),
                   (torch.full((L, L), -1.0).tril(-1) + sub, r"mask\[1, 0\]")):
        with pytest.raises(ValueError, match=pat):
            E._mask_window(m, L)
    for wrong in (torch.zeros(L, L + 1), torch.zeros(L - 1, L - 1, dtype=torch.bool), torch.zeros(2, L, L), above[None], torch.zeros(L, L, dtype=torch.int64)):
        with pytest.raises(ValueError, match="mask must be"):
            E._mask_window(wrong, L)
    # a band with one flaw: the first entry off the band of the window its first masked entry starts
    for dt in (torch.float32, torch.bool):
        b = WB.band_mask(L, 3, dt)
        b[5, 3] = True if dt == torch.bool else float("-inf")                  # inside the window, masked
        with pytest.raises(ValueError, match=r"mask\[5, 3\].*window 3"):
            E._mask_window(b, L)
        b = WB.band_mask(L, 3, dt)
        b[6, 2] = False if dt == torch.bool else 0.0                           # below the window, clear
        with pytest.raises(ValueError, match=r"mask\[6, 2\].*window 3"):
            E._mask_window(b, L)
        b = WB.band_mask(L, 3, dt)
        b[1, 4] = False if dt == torch.bool else 0.0                           # above the diagonal, clear: not even causal
        with pytest.raises(ValueError, match=r"mask\[1, 4\]"):
            E._mask_window(b, L)
    two = WB.band_mask(L, 2, torch.bool)
    two[4:] = WB.band_mask(L, 3, torch.bool)[4:]                                # two windows in one mask
    with pytest.raises(ValueError, match=r"mask\[4, 2\].*window 2"):
        E._mask_window(two, L)
    nan = WB.band_mask(L, 3)
    nan[3, 0] = float("nan")
    with pytest.raises(ValueError, match=r"mask\[3, 0\]"):
        E._mask_window(nan, L)


# ---- 5. the C-ABI -----------------------------------------------------------------------------------------------------------------
def test_symbol_is_bound_documented_and_refuses_null():
    import re
    from flope_amd import _lib
    lib = _lib.load()
    assert "flope_tf_stream_open_window" in _lib.SIGNATURES and hasattr(lib, "flope_tf_stream_open_window")
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert re.search(r"int flope_tf_stream_open_window\(flope_tf_handle h, int tracks, int capacity, int window, flope_tf_stream\* out\);", header)
    assert '"window" (default 0; FLOPE_EINVAL below 0' in header
    out = C.c_void_p(5)
    assert lib.flope_tf_stream_open_window(None, 1, 4, 2, C.byref(out)) == _lib.EINVAL and not out.value      # no handle, no state
    assert lib.flope_tf_stream_open_window(None, 1, 4, 2, None) == _lib.EINVAL
    assert lib.flope_tf_set_option(None, b"window", 4) == _lib.EINVAL
    if not torch.cuda.is_available():
        from flope_amd.tf_encoder import TransformerEncoder
        with pytest.raises(RuntimeError):
            TransformerEncoder(16, 32, 9, 4, 2, 64)
