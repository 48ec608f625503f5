"""The host side of a compiled attention mask (flope_amd/csrc/tf_attn_mask.h through tests/host_harness/harness_tf_mask.cpp; DESIGN.md
37) without a device:

  1. packing, the first / last tables, both validators, the per-length check and the pair counts against brute force in numpy on a
     few thousand random masks, word and trip boundaries among the sizes;
  2. the masked launch: the generic kernel's grid and block, its rows covered exactly once, the LDS figure written out here;
  3. every refusal the validators make, by hand;
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
u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def H():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_mask.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_mask.so"])
    lib = C.CDLL(path)
    lib.tf_mask_pairs.restype = lib.tf_mask_pairs_len.restype = C.c_longlong
    lib.tf_mask_lds_words_at.restype = C.c_long
    return lib


def pack(H, allow):
    L = allow.shape[0]
    a = np.ascontiguousarray(allow, dtype=np.uint8)
    bits = np.full(L * H.tf_mask_words(L), 0xffffffff, dtype=np.uint32)
    H.tf_mask_pack(a.ctypes.data_as(C.POINTER(C.c_ubyte)), L, bits.ctypes.data_as(u32p))
    return bits


def first_last(H, bits, L):
    first, last = np.full(L, -7, dtype=np.int32), np.full(L, -7, dtype=np.int32)
    H.tf_mask_first_last(bits.ctypes.data_as(u32p), L, first.ctypes.data_as(i32p), last.ctypes.data_as(i32p))
    return first, last


def padding_bit(H, bits, L):
    out = (C.c_int * 2)()
    H.tf_mask_padding_bit(bits.ctypes.data_as(u32p), L, out)
    return tuple(out)


def brute_pack(allow):
    L = allow.shape[0]
    w = (L + 31) // 32
    bits = np.zeros((L, w), dtype=np.uint64)
    for j in range(L):
        bits[:, j // 32] |= allow[:, j].astype(np.uint64) << np.uint64(j % 32)
    return bits.astype(np.uint32).reshape(-1)


def random_masks(n_per_size=200, seed=3):
    rng = np.random.default_rng(seed)
    for L in SIZES:
        for rep in range(n_per_size if L <= 65 else n_per_size // 4):
            allow = rng.random((L, L)) < rng.choice([0.0, 0.02, 0.3, 0.6, 0.98, 1.0])
            if rep % 3 == 0:
                allow[np.arange(L), np.arange(L)] = True
            yield L, allow


# ---- 1. against brute force ---------------------------------------------------------------------------------------------------------
def test_words(H):
    assert [H.tf_mask_words(L) for L in (1, 31, 32, 33, 64, 65, 130)] == [1, 1, 1, 2, 2, 3, 5]


def test_tables_validators_and_counts_against_brute_force(H):
    n = 0
    for L, allow in random_masks():
        bits = pack(H, allow)
        assert np.array_equal(bits, brute_pack(allow)), L
        first, last = first_last(H, bits, L)
        any_key = allow.any(axis=1)
        want_first = np.where(any_key, allow.argmax(axis=1), L)
        want_last = np.where(any_key, L - 1 - allow[:, ::-1].argmax(axis=1), -1)
        assert np.array_equal(first, want_first) and np.array_equal(last, want_last), L
        empty = np.flatnonzero(~any_key)
        assert H.tf_mask_empty_row(bits.ctypes.data_as(u32p), L) == (int(empty[0]) if len(empty) else -1)
        assert padding_bit(H, bits, L) == (-1, -1)
        assert H.tf_mask_pairs(bits.ctypes.data_as(u32p), L) == int(allow.sum())
        for ln in sorted({1, L, max(1, L // 2), min(L, 32), min(L, 33), min(L, 64), min(L, 65), max(1, L - 1)}):
            corner = allow[:ln, :ln]
            bad = np.flatnonzero(~corner.any(axis=1))
            assert H.tf_mask_length_row(first.ctypes.data_as(i32p), L, ln) == (int(bad[0]) if len(bad) else -1), (L, ln)
            assert H.tf_mask_pairs_len(bits.ctypes.data_as(u32p), L, ln) == int(corner.sum()), (L, ln)
        n += 1
    assert n >= 2000


def test_every_length_of_one_mask(H):
    rng = np.random.default_rng(9)
    allow = rng.random((130, 130)) < 0.05
    bits = pack(H, allow)
    first, _ = first_last(H, bits, 130)
    for ln in range(1, 131):
        corner = allow[:ln, :ln]
        bad = np.flatnonzero(~corner.any(axis=1))
        assert H.tf_mask_length_row(first.ctypes.data_as(i32p), 130, ln) == (int(bad[0]) if len(bad) else -1)
        assert H.tf_mask_pairs_len(bits.ctypes.data_as(u32p), 130, ln) == int(corner.sum())


# ---- 2. the launch ----------------------------------------------------------------------------------------------------------------------
def test_launch_is_the_generic_one_plus_the_mask_rows(H):
    assert H.tf_mask_attn_id() == 4
    for L in SIZES:
        for max_len in sorted({1, L, max(1, L // 3)}):
            out = (C.c_long * 4)()
            H.tf_mask_launch(6, 3, 2, max_len, L, out)
            gx, gy, block, lds = out
            assert (gx, block) == (6, 256) and gy == min(64, (max_len + 3) // 4)
            assert lds == 4 * max_len * 4 + 4 * ((L + 31) // 32) * 4           # four score rows of floats, four mask rows of words
            assert H.tf_mask_lds_words_at(max_len) == 4 * max_len
            seen = np.zeros(max_len, dtype=int)                                # wave w of workgroup y: rows 4 y + w, + 4 grid_y, ..
            for y in range(gy):
                for w in range(4):
                    seen[4 * y + w::4 * gy] += 1
            assert (seen == 1).all()
    out = (C.c_long * 4)()
    H.tf_mask_launch(64, 1, 2, 4096, 4096, out)                                # the longest sequence of a default handle fits the 160 KiB
    assert out[3] == 4 * 4096 * 4 + 4 * 128 * 4 <= 160 * 1024 and out[1] == 64


# ---- 3. every refusal, by hand ----------------------------------------------------------------------------------------------------------
def test_row_without_a_key_is_found(H):
    allow = np.ones((33, 33), dtype=bool)
    assert H.tf_mask_empty_row(pack(H, allow).ctypes.data_as(u32p), 33) == -1
    allow[32] = False
    assert H.tf_mask_empty_row(pack(H, allow).ctypes.data_as(u32p), 33) == 32
    allow[7] = False
    assert H.tf_mask_empty_row(pack(H, allow).ctypes.data_as(u32p), 33) == 7
    allow[7, 32] = True                                                       # its only key is in the second word
    assert H.tf_mask_empty_row(pack(H, allow).ctypes.data_as(u32p), 33) == 32


def test_padding_bits_are_found_and_do_not_count_as_keys(H):
    allow = np.zeros((33, 33), dtype=bool)
    allow[:, 0] = True
    bits = pack(H, allow)
    bits[2 * 5 + 1] |= np.uint32(1 << 1)                                       # row 5, column 33
    assert padding_bit(H, bits, 33) == (33, 5)
    bits[2 * 3 + 1] |= np.uint32(1 << 31)                                      # row 3, column 63: the earlier row wins
    assert padding_bit(H, bits, 33) == (63, 3)
    first, last = first_last(H, bits, 33)
    assert (first == 0).all() and (last == 0).all()
    assert H.tf_mask_pairs(bits.ctypes.data_as(u32p), 33) == 33
    only_pad = np.zeros(2 * 33, dtype=np.uint32)
    only_pad[0::2] = 1
    only_pad[2 * 9], only_pad[2 * 9 + 1] = 0, 2                                 # row 9: nothing but a padding bit
    assert H.tf_mask_empty_row(only_pad.ctypes.data_as(u32p), 33) == 9
    full = np.full(2, 0xffffffff, dtype=np.uint32)                            # L = 64: no padding columns at all
    assert padding_bit(H, np.tile(full, 64), 64) == (-1, -1)


def test_length_whose_corner_leaves_a_row_without_keys(H):
    allow = np.tril(np.ones((15, 15), dtype=bool))
    allow[4] = False
    allow[4, 9] = True                                                        # row 4 sees key 9 only
    first, _ = first_last(H, pack(H, allow), 15)
    fp = first.ctypes.data_as(i32p)
    assert [H.tf_mask_length_row(fp, 15, n) for n in (1, 4, 5, 9, 10, 15)] == [-1, -1, 4, 4, -1, -1]


# ---- 4. the same under AddressSanitizer + UBSan, as a program of its own --------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """the host functions once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_mask_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_MASK_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_mask.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "440 masks, 0 failures" in r.stdout
