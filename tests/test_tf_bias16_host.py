"""The host side of a compiled bias on the 16-bit MFMA attention (option "bias_mfma"; flope_amd/csrc/tf_attn_mask.h through
tests/host_harness/harness_tf_bias16.cpp) without a device:

  1. tf_attn_pick_biased written out literally over dtype x head_dim x the options x alignment; no head_dim that tf_attn_tiled serves is
     refused for scratch (all four instantiations were built without), and the pick says so;
  2. the device layout bits | first | last | bias | start | tiles: the new offsets, the entries on a 16-byte boundary, and the two old
     functions (tf_bias_dev_bias_at, tf_bias_dev_bytes) with the values tests/test_tf_bias_host.py pins;
  3. tf_bias16_lane_index against numpy brute force: for every lane of every taken step of every corner length the index lies inside row
     min(query, n - 1) of plane h (or 0), its column is the key kb + 16 u + 4 g + q (clamped to L - 1 where that key lies past the row:
     such a key is never seen), and no index is formed for a skipped step;
  4. the same properties once more in a stand-alone program with its own main under -fsanitize=address,undefined, its planes sized
     exactly, compiled and run here as a child process (nothing is loaded into Python under a sanitizer);
  5. the option and id 7 in the header text and in the binding.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 300]
BF16, F16, F32 = 0, 1, 2
BIASED, BIASED16 = 6, 7
QB, KB = 128, 64


@pytest.fixture(scope="module")
def H():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_bias16.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_bias16.so"])
    lib = C.CDLL(path)
    lib.tf_bias16_lane_index.restype = lib.tf_bias16_walk.restype = C.c_longlong
    lib.tf_bias16_walk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.tf_bias16_dev_layout.argtypes = [C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_longlong)]
    return lib


# ---- 1. the pick ----------------------------------------------------------------------------------------------------------------------
def test_dtype_codes_are_the_headers():
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    for name, v in (("FLOPE_DT_F32", F32), ("FLOPE_DT_F16", F16), ("FLOPE_DT_BF16", BF16)):
        assert f"#define {name:<19} {v} " in header, name


def test_pick_written_out(H):
    assert H.tf_bias16_attn_id() == BIASED16
    want = {}
    for dtype in (F32, F16, BF16):
        for hd in (6, 32, 64, 96, 128, 160):
            for generic in (0, 1):
                for opt in (0, 1):
                    for aligned in (0, 1):
                        want[dtype, hd, generic, opt, aligned] = BIASED
    for dtype in (F16, BF16):
        for hd in (32, 64, 96, 128):
            want[dtype, hd, 0, 1, 1] = BIASED16
    assert sum(v == BIASED16 for v in want.values()) == 8
    for key, v in want.items():
        assert H.tf_bias16_pick(*key) == v, key
    for bad in (2, -1, 3):                                       # the entry point refuses them; the pick itself takes 1 alone
        assert H.tf_bias16_pick(F16, 64, 0, bad, 1) == BIASED


def test_no_head_dim_is_refused_for_scratch(H):
    """the sixteen BIASED instantiations were built without scratch (head_dim 128 by loading per query tile with dword
    loads), so the list of built head_dims is the list tf_attn_tiled serves; a head_dim outside it keeps id 6"""
    assert [hd for hd in range(1, 300) if H.tf_bias16_built(hd)] == [32, 64, 96, 128]
    assert [hd for hd in range(1, 300) if H.tf_bias16_pick(F16, hd, 0, 1, 1) == BIASED16] == [32, 64, 96, 128]


# ---- 2. the layout --------------------------------------------------------------------------------------------------------------------
def test_layout(H):
    out = (C.c_longlong * 5)()
    for L in SIZES + [2, 15, 96, 130, 4096]:
        words, nqb = (L + 31) // 32, (L + QB - 1) // QB
        at = (L * words + 2 * L) * 4
        for planes in (1, 4, 6):
            for entries in (1, 7, 1000):
                H.tf_bias16_dev_layout(L, planes, entries, out)
                bias_at, start_at, tiles_at, total, old_total = list(out)
                assert bias_at == at and old_total == at + planes * L * L * 4, "the two old functions keep their values"
                assert start_at == old_total and start_at % 4 == 0, "the map starts where the planes end"
                assert tiles_at % 16 == 0 and 0 <= tiles_at - (start_at + (nqb + 1) * 4) < 16
                assert total == tiles_at + entries * 16
        if L % 4 == 0:
            assert at % 16 == 0, "a plane row starts on a 16-byte boundary where L is a multiple of 4"


# ---- 3. the lane index against brute force --------------------------------------------------------------------------------------------
def _allowed(L, rep, rng):
    a = rng.random((L, L)) < (0.02, 0.4, 0.97, 1.0)[rep % 4]
    a[np.arange(L), np.arange(L)] = True                          # every corner leaves every row a key
    if rep % 4 == 1 and L > 64:
        a[:, 64:128] = False                                      # a key block nobody lists: trip index and block index differ
        a[np.arange(L), np.arange(L)] = True
    return a


def _corners(L):
    """every corner length up to L = 129; above, the lengths around every step, block and query-block edge"""
    if L <= 129:
        return list(range(1, L + 1))
    return sorted({n for n in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 256, 257, L - 1, L) if 1 <= n <= L})


def _brute(a, L, planes, n, h):
    """every (row, column) the walk forms for a sequence of n tokens, in walk order, from the definition: a step is taken by a wave where
    its 32 x 32 tile of the WHOLE mask (rows and keys below L) holds an allowed pair, its key block is listed (always, then) and starts
    below n"""
    rows, cols = [], []
    u, g, q = np.meshgrid(np.arange(2), np.arange(4), np.arange(4), indexing="ij")
    key_off = (16 * u + 4 * g + q).reshape(-1)                   # in (u, g, q) order
    for qb in range((n + QB - 1) // QB):
        for kblock in range((L + KB - 1) // KB):
            if kblock * KB >= n or not a[qb * QB:(qb + 1) * QB, kblock * KB:(kblock + 1) * KB].any():
                continue
            for s in range(2):
                kb = kblock * KB + 32 * s
                if kb >= n:
                    continue
                for w in range(4):
                    r0 = qb * QB + 32 * w
                    if not a[r0:r0 + 32, kb:kb + 32].any():
                        continue
                    for lane in range(32):
                        rows.append(np.full(32, min(r0 + lane, n - 1)))
                        cols.append(np.minimum(kb + key_off, L - 1))
    if not rows:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(rows), np.concatenate(cols)


def test_lane_index_against_brute_force(H):
    rng = np.random.default_rng(44)
    Hh, total = 3, 0
    for L in SIZES:
        for rep in range(4):
            a = _allowed(L, rep, rng)
            a8 = np.ascontiguousarray(a, dtype=np.uint8)
            planes = Hh if rep % 2 else 1
            for n in _corners(L):
                for h in ((0, Hh - 1) if planes > 1 else (1,)):
                    cnt = H.tf_bias16_walk(a8.ctypes.data, L, planes, n, h, None)
                    idx = np.full(cnt + 1, -7, dtype=np.int64)
                    assert H.tf_bias16_walk(a8.ctypes.data, L, planes, n, h, idx.ctypes.data) == cnt and idx[cnt] == -7
                    idx = idx[:cnt]
                    rows, cols = _brute(a, L, planes, n, h)
                    assert len(rows) == cnt, (L, rep, n, "no index is formed for a skipped step, one for every lane of a taken one")
                    plane = h if planes > 1 else 0
                    assert np.array_equal(idx, (plane * L + rows) * L + cols), (L, rep, n, h)
                    if cnt:
                        assert idx.min() >= plane * L * L and idx.max() < (plane + 1) * L * L <= planes * L * L
                        assert np.array_equal(idx % L, cols) and np.array_equal(idx // L - plane * L, rows)
                        assert rows.max() <= n - 1 and cols.max() <= L - 1
                    total += cnt
    assert total > 5_000_000


def test_lane_index_by_hand(H):
    f = H.tf_bias16_lane_index
    L = 300
    assert f(L, 1, 300, 5, 0, 0, 0, 0, 0) == 0                                        # one plane: every head reads plane 0
    assert f(L, 6, 300, 5, 0, 0, 0, 0, 0) == 5 * L * L
    assert f(L, 6, 300, 2, 7, 64, 1, 3, 2) == (2 * L + 7) * L + 64 + 16 + 12 + 2      # the key's own column, not 8 g + 4 u + q
    assert f(L, 6, 130, 2, 131, 64, 0, 0, 0) == (2 * L + 129) * L + 64                # a query past n: row n - 1, stride L
    assert f(L, 6, 300, 2, 299, 288, 0, 3, 0) == (2 * L + 299) * L + 299              # key 300 = L: clamped to L - 1 ...
    assert f(L, 6, 300, 2, 299, 288, 1, 3, 3) == (2 * L + 299) * L + 299              # ... and key 319
    assert f(L, 6, 300, 5, 299, 288, 1, 3, 3) == 6 * L * L - 1                        # the last entry of the planes, never one behind
    for L, kb, vec in ((300, 256, 1), (300, 288, 0), (257, 0, 0), (256, 224, 1), (128, 96, 1), (64, 32, 1), (33, 0, 0), (32, 0, 1), (4, 0, 0)):
        assert H.tf_bias16_step_vec(L, kb) == vec, (L, kb)


# ---- 4. the same under AddressSanitizer + UBSan, as a program of its own --------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """the host functions once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_bias16_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_BIAS16_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_bias16.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "48 biases" in r.stdout and ", 0 failures" in r.stdout


# ---- 5. the header and the binding ----------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_option():
    from flope_amd import _lib
    assert _lib.TF_ATTN_BIASED16 == BIASED16 and _lib.TF_ATTN_BIASED == BIASED
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert '"bias_mfma" (default 0; 0 or 1, FLOPE_EINVAL outside; returns the old value' in header
    assert "FLOPE_TF_ATTN_BIASED16 = 7" in header and "never USED" in header
    plan = open(os.path.join(ROOT, "flope_amd", "csrc", "tf_attn_plan.h")).read()
    assert "FLOPE_TF_ATTN_BIASED16 = 7," in plan and "FLOPE_TF_ATTN_BIASED = 6 " in plan
    import inspect
    from flope_amd.tf_encoder import TransformerEncoder
    assert inspect.signature(TransformerEncoder.__init__).parameters["bias_mfma"].default == 0
