"""The planner of option "skinny_ln" without a device (flope_amd/csrc/tf_skinny_plan.h, which tf_gemm_skinny_ln calls per lane, through
tests/host_harness/harness_tf_skinny_ln.cpp).

  1. tf_skinny_ln_ok against a brute-force statement of the rule: M in 0 .. 40, model_dim in {64, 128, 384, 512, 576, 640}, every
     combination of the options and of what the consumer is;
  2. the summation order: for d in {128, 256, 384, 512} and rows of 16-bit values (large common offsets, mixed magnitudes, an all-equal
     row, signed zeros), tf_layernorm_vec's 64-lane butterfly over the per-vector partials and the planner's in-lane tree plus two
     cross-lane steps give the same float32 bit patterns for the sum and for the sum of squared deviations;
  3. two broken copies of the order are noticed: the tree in ascending bit order, and the empty slots skipped;
  4. the post-norm rows: for d in {128, 384, 512} and MT in {1, 2} every element of rows 0 .. 16 MT - 1 is stored exactly once and
     nothing outside; broken assignments are noticed;
  5. the same once more as a stand-alone program under -fsanitize=address,undefined (nothing is loaded into Python under a sanitizer);
  6. the new entry points are declared, bound and exported; the Python surface that needs no device.
"""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = (128, 256, 384, 512)


@pytest.fixture(scope="module")
def H():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_skinny_ln.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_skinny_ln.so"])
    lib = C.CDLL(path)
    lib.tf_skinny_ln_h_ok.argtypes = [C.c_int] * 5
    lib.tf_skinny_ln_h_vec_ok.argtypes = [C.c_int] * 2
    lib.tf_skinny_ln_h_consts.argtypes = [C.c_void_p]
    lib.tf_skinny_ln_h_order.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.tf_skinny_ln_h_cover.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def S():
    """the harness of option skinny: tf_skinny_ok of the consumer"""
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_skinny.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_skinny.so"])
    lib = C.CDLL(path)
    lib.tf_skinny_h_ok.argtypes = [C.c_int] * 6
    return lib


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------------
def test_ok_against_the_rule_by_brute_force(H, S):
    """true exactly where option skinny takes the consumer (a 16-bit handle, a packed image, a 16-bit result, generic off, skinny == 1,
    1 <= M <= 32), skinny_ln == 1, the consumer reads the normalised rows as they are (Kp == K == model_dim), model_dim % 64 == 0 and
    <= 512, and launch_layernorm would run tf_layernorm_vec"""
    taken = 0
    for M in range(0, 41):
        for d in (64, 128, 384, 512, 576, 640):
            for d16, sk, gen, pk, ln in itertools.product((0, 1), repeat=5):
                sk_ok = bool(S.tf_skinny_h_ok(d16, sk, gen, pk, 0, M))
                assert sk_ok == bool(d16 and pk and not gen and sk == 1 and 1 <= M <= 32)
                for K, Kp in ((d, d), (4 * d, 4 * d), (d - 8, d), (d, d + 64)):
                    want = sk_ok and ln == 1 and K == Kp == d and d % 64 == 0 and d <= 512 and bool(H.tf_skinny_ln_h_vec_ok(d16, d))
                    assert bool(H.tf_skinny_ln_h_ok(int(sk_ok), ln, K, Kp, d)) == want, (M, d, d16, sk, gen, pk, ln, K, Kp)
                    taken += want
    assert taken == 32 * 4                                              # 32 row counts, d in {64, 128, 384, 512}, one option combination
    for ln in (-1, 2, 3):                                                # only the value 1 turns it on
        assert not H.tf_skinny_ln_h_ok(1, ln, 384, 384, 384)
    for d in (72, 96, 200):                                              # whole 16-byte vectors, but no whole chunks
        assert not H.tf_skinny_ln_h_ok(1, 1, d, d, d)
    # launch_layernorm's own rule, which the fold must agree with
    for d in (8, 64, 72, 2048, 2056, 4, 100):
        assert bool(H.tf_skinny_ln_h_vec_ok(1, d)) == (d % 8 == 0 and d <= 2048) and not H.tf_skinny_ln_h_vec_ok(0, d)


def test_constants(H):
    c = (C.c_int * 4)()
    H.tf_skinny_ln_h_consts(c)
    slots, steps, x0, x1 = list(c)
    assert slots == 16 and 1 << steps == slots and (x0, x1) == (32, 16)   # 16 slots x 4 lane groups = tf_layernorm_vec's 64 lanes


# ---- 2. the order --------------------------------------------------------------------------------------------------------------------------
def _rows(d, bf16):
    """16-bit patterns [rows, d]: normal rows, large common offsets, mixed magnitudes, an all-equal row, signed zeros"""
    rng = np.random.default_rng(1000 + d + bf16)
    n = rng.standard_normal((40, d)).astype(np.float32)
    fam = [n[:8], 100.0 + n[8:16], -300.0 + 0.01 * n[16:20],
           n[20:28] * np.exp2(rng.integers(-12, 10, size=(8, d))).astype(np.float32),
           np.full((1, d), 0.7, np.float32), np.full((1, d), -1234.5, np.float32),
           np.zeros((1, d), np.float32), -np.zeros((1, d), np.float32),
           np.where(rng.random((4, d)) < 0.5, -0.0, 0.0).astype(np.float32),
           np.where(rng.random((4, d)) < 0.7, -0.0, n[28:32]).astype(np.float32)]
    x = np.concatenate(fam)
    if bf16:
        return (x.view(np.uint32) >> 16).astype(np.uint16)               # truncation: any finite bfloat16 pattern will do
    return x.astype(np.float16).view(np.uint16)


def _order(H, d, row, bf16, broken=0):
    out = (C.c_uint32 * 4)()
    row = np.ascontiguousarray(row, dtype=np.uint16)
    assert H.tf_skinny_ln_h_order(d, row.ctypes.data, bf16, broken, out) == 0
    return list(out)


@pytest.mark.parametrize("bf16", (0, 1), ids=("f16", "bf16"))
@pytest.mark.parametrize("d", DS)
def test_the_lane_tree_is_the_wave_butterfly_in_bits(H, d, bf16):
    rows = _rows(d, bf16)
    assert (rows[-1] == 0x8000).any() and (rows[-9] == 0x8000).all()      # the signed zeros are there
    for i, row in enumerate(rows):
        ws, ls, wv, lv = _order(H, d, row, bf16)
        assert (ws, wv) == (ls, lv), (d, i, hex(ws), hex(ls), hex(wv), hex(lv))


# ---- 3. broken copies of the order -----------------------------------------------------------------------------------------------------------
def test_broken_orders_are_noticed(H):
    """ascending bit order changes the association at every d; skipping the empty slots changes it where 2 d / 64 is no power of two
    (d = 384: a tree over 12 slots), and is the same tree at 128, 256 and 512"""
    for bf16 in (0, 1):
        for d in DS:
            rows = _rows(d, bf16)
            asc = sum(o[0] != o[1] or o[2] != o[3] for o in (_order(H, d, r, bf16, 1) for r in rows))
            assert asc > 0, (d, bf16)
            skip = sum(o[0] != o[1] or o[2] != o[3] for o in (_order(H, d, r, bf16, 2) for r in rows))
            assert (skip > 0) == (d == 384), (d, bf16, skip)


# ---- 4. the post-norm rows -------------------------------------------------------------------------------------------------------------------
def cover(H, d, N, MT, broken=0):
    fails = (C.c_longlong * 3)()
    rc = H.tf_skinny_ln_h_cover(d, N, MT, broken, fails)
    got = dict(zip(("cover", "bounds", "meaning"), list(fails)))
    assert rc == int(any(got.values()))
    return got


@pytest.mark.parametrize("MT", (1, 2))
@pytest.mark.parametrize("d", (128, 384, 512))
def test_every_element_of_h_is_stored_once(H, d, MT):
    for N in (128, d, 3 * d, 1536):
        if N % 128 == 0:
            assert cover(H, d, N, MT) == {"cover": 0, "bounds": 0, "meaning": 0}, (d, N, MT)


def test_broken_assignments_are_noticed(H):
    """every wave storing chunk ft % nch (elements stored more than once); ks dropped from the offset (half the row never stored);
    token tile 1 stored 16 rows further (outside the rows)"""
    for d in (128, 384, 512):
        got = cover(H, d, 1536, 2, 1)
        assert got["cover"] > 0 and got["bounds"] == 0, got
        got = cover(H, d, 384, 1, 2)
        assert got["cover"] > 0 and got["bounds"] == 0, got
        got = cover(H, d, 384, 2, 4)
        assert got["bounds"] > 0 and got["cover"] > 0, got
        assert cover(H, d, 384, 1, 4) == {"cover": 0, "bounds": 0, "meaning": 0}       # (there is no tile 1 at MT = 1)


# ---- 5. the same under AddressSanitizer + UBSan, as a program of its own ---------------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """every shape once in a stand-alone program of its own (host code only, nothing loaded into python): the stores are made into a
    buffer of exactly 16 MT d 2 bytes"""
    exe = str(tmp_path / "tf_skinny_ln_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_SKINNY_LN_MAIN",
                           "-std=c++17", "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_skinny_ln.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "24 shapes, 512 rows, 0 failures" in r.stdout


# ---- 6. the surface ----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from flope_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    for name in ("flope_tf_linear_ln", "flope_tf_linear_ln_plan", "flope_tf_last_ln"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define FLOPE_TF_LIN_SKINNY_LN\s+6\b", header) and _lib.TF_LIN_SKINNY_LN == 6
    assert '"skinny_ln"' in header


def test_python_surface_without_a_device():
    import inspect
    from flope_amd.tf_encoder import TransformerEncoder
    assert inspect.signature(TransformerEncoder.__init__).parameters["skinny_ln"].default == 0
    assert list(inspect.signature(TransformerEncoder.linear_ln).parameters) == ["self", "name", "x", "weight", "bias", "relu", "out", "normed"]
    assert list(inspect.signature(TransformerEncoder.linear_ln_plan).parameters) == ["self", "name", "rows"]
    assert isinstance(TransformerEncoder.last_ln, property)
