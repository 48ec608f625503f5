"""The host side of a compiled additive bias (flope_amd/csrc/tf_attn_mask.h through tests/host_harness/harness_tf_bias.cpp; DESIGN.md
39) without a device:

  1. the bit words derived from the -inf entries (they are tf_mask_pack's for that allowed set), first / last, and both validators a
     bias adds -- a +inf / NaN entry, a plane whose allowed set differs from plane 0's -- against brute force in numpy on random
     biases of 1 and 4 planes at the sizes tests/test_tf_mask_host.py uses, the named (plane, row, col) checked;
  2. every refusal by hand, NULL arguments, the device layout and the index of an entry;
  3. the two new symbols in _lib.SIGNATURES, and alibi_bias against its formula;
  4. the same properties once more in a stand-alone program with its own main under -fsanitize=address,undefined, compiled and run
     here as a child process (nothing is loaded into Python under a sanitizer).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 15, 31, 32, 33, 63, 64, 65, 96, 127, 128, 130]
u32p, i32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_float)
NINF = np.float32(-np.inf)


@pytest.fixture(scope="module")
def H():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_bias.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_bias.so"])
    lib = C.CDLL(path)
    lib.tf_bias_dev_bias_at.restype = lib.tf_bias_dev_bytes.restype = lib.tf_bias_index.restype = C.c_long
    return lib


def fp(a):
    return a.ctypes.data_as(f32p)


def pack(H, bias):
    L = bias.shape[-1]
    bits = np.full(L * H.tf_bias_words(L), 0xffffffff, dtype=np.uint32)
    H.tf_bias_pack(fp(bias), L, bits.ctypes.data_as(u32p))
    return bits


def mask_pack(H, allow):
    L = allow.shape[0]
    a = np.ascontiguousarray(allow, dtype=np.uint8)
    bits = np.full(L * H.tf_bias_words(L), 0xffffffff, dtype=np.uint32)
    H.tf_bias_mask_pack(a.ctypes.data_as(C.POINTER(C.c_ubyte)), L, bits.ctypes.data_as(u32p))
    return bits


def brute_pack(allow):
    L = allow.shape[0]
    w = (L + 31) // 32
    bits = np.zeros((L, w), dtype=np.uint64)
    for j in range(L):
        bits[:, j // 32] |= allow[:, j].astype(np.uint64) << np.uint64(j % 32)
    return bits.astype(np.uint32).reshape(-1)


def found(fn, bias):
    """(1 / 0, (plane, row, col)) of a validator; the triple stays (-7, -7, -7) where nothing is found"""
    out = (C.c_int * 3)(-7, -7, -7)
    planes, L = bias.shape[0], bias.shape[-1]
    return fn(fp(bias), L, planes, out), tuple(out)


def first_in_order(wrong):
    """the first True of a [planes, L, L] bool array in (plane, row, col) order, or None"""
    idx = np.flatnonzero(wrong.reshape(-1))
    return None if not len(idx) else tuple(int(v) for v in np.unravel_index(idx[0], wrong.shape))


def random_biases(n_per_size=60, seed=4):
    rng = np.random.default_rng(seed)
    for L in SIZES:
        for planes in (1, 4):
            for rep in range(n_per_size if L <= 65 else n_per_size // 4):
                allow = rng.random((L, L)) < rng.choice([0.0, 0.02, 0.3, 0.6, 0.98, 1.0])
                if rep % 3 == 0:
                    allow[np.arange(L), np.arange(L)] = True
                bias = (2 * rng.standard_normal((planes, L, L))).astype(np.float32)
                bias[:, ~allow] = NINF
                yield L, planes, allow, np.ascontiguousarray(bias), rng


# ---- 1. against brute force ---------------------------------------------------------------------------------------------------------
def test_words_tables_and_validators_against_brute_force(H):
    n = 0
    for L, planes, allow, bias, rng in random_biases():
        bits = pack(H, bias)
        assert np.array_equal(bits, brute_pack(allow)) and np.array_equal(bits, mask_pack(H, allow)), (L, planes)
        first, last = np.full(L, -7, dtype=np.int32), np.full(L, -7, dtype=np.int32)
        H.tf_bias_first_last(bits.ctypes.data_as(u32p), L, first.ctypes.data_as(i32p), last.ctypes.data_as(i32p))
        any_key = allow.any(axis=1)
        assert np.array_equal(first, np.where(any_key, allow.argmax(axis=1), L)), L
        assert np.array_equal(last, np.where(any_key, L - 1 - allow[:, ::-1].argmax(axis=1), -1)), L
        empty = np.flatnonzero(~any_key)
        assert H.tf_bias_empty_row(bits.ctypes.data_as(u32p), L) == (int(empty[0]) if len(empty) else -1)
        assert found(H.tf_bias_nonfinite, bias) == (0, (-7, -7, -7))
        assert found(H.tf_bias_plane_differs, bias) == (0, (-7, -7, -7))
        # a few +inf / NaN entries anywhere: the first in (plane, row, col) order is named
        bad = bias.copy()
        wrong = rng.random(bias.shape) < 3.0 / bias.size
        wrong.reshape(-1)[rng.integers(bias.size)] = True
        bad[wrong] = np.where(rng.random(int(wrong.sum())) < 0.5, np.float32(np.inf), np.float32(np.nan))
        assert found(H.tf_bias_nonfinite, bad) == (1, first_in_order(wrong)), (L, planes)
        if planes > 1:
            # a few entries of the later planes flipped between masked and finite: the first that differs from plane 0 is named
            dif = bias.copy()
            flip = rng.random(bias.shape) < 3.0 / bias.size
            flip[0] = False
            flip[1:].reshape(-1)[rng.integers((planes - 1) * L * L)] = True
            dif[flip] = np.where(dif[flip] == NINF, np.float32(-1e30), NINF)
            assert found(H.tf_bias_plane_differs, dif) == (1, first_in_order(flip)), (L, planes)
            assert np.array_equal(pack(H, dif), bits)                               # the words are plane 0's
        n += 1
    assert n >= 1000


# ---- 2. by hand -----------------------------------------------------------------------------------------------------------------------------
def test_each_refusal_by_hand(H):
    b = np.zeros((4, 33, 33), dtype=np.float32)
    b[:, 5, 32] = NINF
    assert found(H.tf_bias_nonfinite, b)[0] == 0 and found(H.tf_bias_plane_differs, b)[0] == 0       # -inf is a value a bias may hold
    c = b.copy(); c[2, 7, 32] = np.inf
    assert found(H.tf_bias_nonfinite, c) == (1, (2, 7, 32))
    c[1, 30, 0] = np.nan                                                            # an earlier plane wins
    assert found(H.tf_bias_nonfinite, c) == (1, (1, 30, 0))
    c[1, 2, 31] = np.inf                                                            # an earlier row of it wins
    assert found(H.tf_bias_nonfinite, c) == (1, (1, 2, 31))
    d = b.copy(); d[3, 5, 32] = -1e30                                               # allowed in plane 3, masked in plane 0
    assert found(H.tf_bias_plane_differs, d) == (1, (3, 5, 32))
    d[1, 0, 0] = NINF                                                               # masked in plane 1, allowed in plane 0
    assert found(H.tf_bias_plane_differs, d) == (1, (1, 0, 0))
    assert found(H.tf_bias_plane_differs, d[:1].copy())[0] == 0                     # one plane cannot disagree
    e = np.full((1, 15, 15), -3.5, dtype=np.float32)
    e[0, 9] = NINF                                                                  # a row without a key
    assert H.tf_bias_empty_row(pack(H, e).ctypes.data_as(u32p), 15) == 9
    e[0, 9, 14] = -1e38                                                             # a huge finite value is a key
    assert H.tf_bias_empty_row(pack(H, e).ctypes.data_as(u32p), 15) == -1
    z = np.zeros((1, 4, 4), dtype=np.float32)
    z[0, 1, 2] = -0.0                                                               # the sign of a zero does not mask
    assert np.array_equal(pack(H, z), np.full(4, 0xf, dtype=np.uint32))


def test_null_arguments(H):
    out = (C.c_int * 3)(-7, -7, -7)
    b = np.zeros((1, 2, 2), dtype=np.float32)
    assert H.tf_bias_nonfinite(None, 2, 1, out) == -1 and H.tf_bias_nonfinite(fp(b), 2, 1, None) == -1
    assert H.tf_bias_plane_differs(None, 2, 1, out) == -1 and H.tf_bias_plane_differs(fp(b), 2, 1, None) == -1
    assert tuple(out) == (-7, -7, -7)
    bits = np.full(2, 0xffffffff, dtype=np.uint32)
    H.tf_bias_pack(None, 2, bits.ctypes.data_as(u32p))
    H.tf_bias_pack(fp(b), 2, None)
    assert (bits == 0xffffffff).all()


def test_layout_and_index(H):
    assert H.tf_bias_attn_id() == 6
    for L in SIZES:
        words = (L + 31) // 32
        at = (L * words + 2 * L) * 4                                                # bits | first | last | bias
        assert H.tf_bias_dev_bias_at(L) == at and at % 4 == 0
        for planes in (1, 4):
            assert H.tf_bias_dev_bytes(L, planes) == at + planes * L * L * 4
            for h in range(4):
                for i, j in ((0, 0), (L - 1, L - 1), (L // 2, L - 1), (L - 1, 0)):
                    assert H.tf_bias_index(L, planes, h, i, j) == ((h if planes > 1 else 0) * L + i) * L + j < planes * L * L
    assert H.tf_bias_dev_bytes(4096, 1) - H.tf_bias_dev_bias_at(4096) == 64 << 20    # a plane at L = 4096 is 64 MiB


# ---- 3. the binding and the helper --------------------------------------------------------------------------------------------------
def test_signatures_hold_the_new_symbols():
    from flope_amd import _lib
    assert _lib.SIGNATURES["flope_tf_bias_create"][0] is C.c_int and len(_lib.SIGNATURES["flope_tf_bias_create"][1]) == 5
    assert _lib.SIGNATURES["flope_tf_mask_bias_planes"] == (C.c_int, [C.c_void_p])
    assert _lib.TF_ATTN_BIASED == 6
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    assert "int flope_tf_bias_create(" in header and "int flope_tf_mask_bias_planes(" in header


def test_alibi_bias_is_its_formula():
    import torch
    from flope_amd.tf_encoder import alibi_bias
    slopes = [2.0 ** -(h + 1) for h in range(4)]
    for L in (1, 15, 33):
        for causal in (True, False):
            b = alibi_bias(L, slopes, causal=causal)
            assert b.dtype == torch.float32 and tuple(b.shape) == (4, L, L)
            for h in range(4):
                for i in range(L):
                    for j in range(L):
                        want = float("-inf") if causal and j > i else -slopes[h] * abs(i - j)
                        assert b[h, i, j].item() == np.float32(want), (L, h, i, j)
    assert torch.equal(alibi_bias(15, slopes), alibi_bias(15, slopes, causal=True))        # causal by default
    assert tuple(alibi_bias(7, [0.5]).shape) == (1, 7, 7)
    assert tuple(alibi_bias(7, torch.tensor([0.5, 0.25])).shape) == (2, 7, 7)


# ---- 4. the same under AddressSanitizer + UBSan, as a program of its own --------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """the host functions once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_bias_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_BIAS_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_bias.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "440 biases, 0 failures" in r.stdout
