"""The tile map of a compiled attention mask (flope_amd/csrc/tf_attn_mask.h through tests/host_harness/harness_tf_mask16.cpp; DESIGN.md
38) without a device:

  1. the lists, colany and the classes against brute force in numpy (tests/tf_attn_mask16_bound.tile_map) on random masks at 1 %, 40 %
     and 99 %, causal, band, block-diagonal and prefix masks, at every length where a word, a step, a key block or a query block ends;
  2. the corner prefix for every n, and the word every lane of every taken step loads;
  3. tf_attn_pick_masked written out literally, the launch, the layout of the device allocation;
  4. the same properties once more in a stand-alone program with its own main under -fsanitize=address,undefined, compiled and run
     here as a child process (nothing is loaded into Python under a sanitizer).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tf_attn_mask16_bound as M16      # noqa: E402
import tf_attn_mask_bound as MB         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 257, 300]
u32p, i32p, i64p = C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
DT_BF16, DT_F16, DT_F32 = 0, 1, 2


@pytest.fixture(scope="module")
def H():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_mask16.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_mask16.so"])
    lib = C.CDLL(path)
    lib.tf_mask16_build.restype = lib.tf_mask16_lane_word.restype = C.c_longlong
    lib.tf_mask16_class.argtypes = [C.c_uint32, C.c_int, C.c_int]
    return lib


def masks(L):
    """(name, allowed bool [L, L] numpy), every row with a key"""
    rng = np.random.default_rng(1000 + L)
    for dens in (0.01, 0.40, 0.99):
        a = rng.random((L, L)) < dens
        empty = ~a.any(axis=1)
        a[empty, rng.integers(0, L, size=int(empty.sum()))] = True
        yield f"random{dens}", a
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    yield "causal", j <= i
    for W in (1, 33, 100):
        yield f"band{W}", (j <= i) & (j > i - W)
    yield "band+-3", np.abs(j - i) <= 3
    yield "prefix", (j <= i) | (j < 5)
    for blocks in ([32, 64, 33], [4, 1, 33, 65, 27], [128, 1, 96, 32]):
        lens = []
        while sum(lens) < L:
            lens.append(min(blocks[len(lens) % len(blocks)], L - sum(lens)))
        yield f"blocks{blocks}", MB.block_diagonal(lens).numpy()
        yield f"blocks{blocks}causal", MB.block_diagonal(lens, causal=True).numpy()


def build(H, allowed):
    L = allowed.shape[0]
    a = np.ascontiguousarray(allowed, dtype=np.uint8)
    nw = (L + 31) // 32
    bits = np.full(L * nw, 0xffffffff, dtype=np.uint32)
    H.tf_mask16_pack(a.ctypes.data_as(C.POINTER(C.c_ubyte)), L, bits.ctypes.data_as(u32p))
    nqb = H.tf_mask16_query_blocks(L)
    start = np.full(nqb + 1, -7, dtype=np.int32)
    n = H.tf_mask16_build(bits.ctypes.data_as(u32p), L, start.ctypes.data_as(i32p), None)
    tiles = np.full((n, 4), 0xdeadbeef, dtype=np.uint32)
    assert H.tf_mask16_build(bits.ctypes.data_as(u32p), L, start.ctypes.data_as(i32p), tiles.ctypes.data_as(u32p)) == n
    return bits, start, tiles


# ---- 1. lists, colany and classes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_tile_map_against_brute_force(H, L):
    assert H.tf_mask16_query_blocks(L) == (L + 127) // 128 and H.tf_mask16_key_blocks(L) == (L + 63) // 64
    for name, a in masks(L):
        bits, start, tiles = build(H, a)
        want = M16.tile_map(a)
        assert len(want) == len(start) - 1 and start[0] == 0, name
        covered = np.zeros_like(a)
        for qb, lst in enumerate(want):
            got = tiles[start[qb]:start[qb + 1]]
            assert len(got) >= 1, (name, qb, "every query block lists a block")
            assert [int(t[0]) for t in got] == [kblock for kblock, _, _ in lst], (name, qb)      # exactly the blocks with a pair, ascending
            assert all(int(got[i][0]) < int(got[i + 1][0]) for i in range(len(got) - 1))
            for t, (kblock, colany, cls) in zip(got, lst):
                sub = a[qb * 128:(qb + 1) * 128, kblock * 64:(kblock + 1) * 64]
                assert sub.any(), "a listed block holds an allowed pair"
                bitsany = (int(t[1]) | (int(t[2]) << 32))
                assert [(bitsany >> r) & 1 for r in range(64)] == [int(c) for c in colany], (name, qb, kblock)
                assert int(t[3]) >> 16 == 0
                for w in range(4):
                    for s in range(2):
                        tile = sub[32 * w:32 * w + 32, 32 * s:32 * s + 32]
                        c = H.tf_mask16_class(int(t[3]), w, s)
                        assert c == cls[w][s], (name, qb, kblock, w, s)
                        assert (c == 2) == (tile.size > 0 and bool(tile.all())) and (c == 0) == (not tile.any())
                        if c:
                            covered[qb * 128 + 32 * w:qb * 128 + 32 * w + 32, kblock * 64 + 32 * s:kblock * 64 + 32 * s + 32] = True
        assert not (a & ~covered).any(), (name, "every allowed pair lies in a listed block and in a step of class some or all")
        out = (C.c_longlong * 5)()
        H.tf_mask16_stats(L, start.ctypes.data_as(i32p), tiles.ctypes.data_as(u32p), out)
        st = M16.tile_stats(a)
        assert list(out) == [st[k] for k in ("query_blocks", "blocks_listed", "steps_none", "steps_some", "steps_all")], name
        assert out[2] + out[3] + out[4] == 8 * out[1]


# ---- 2. the corner, and the words the lanes load -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_corner_prefix_and_lane_words(H, L):
    nw = (L + 31) // 32
    for name, a in masks(L):
        if not (name.startswith("random") or name in ("causal", "band33", "prefix")):
            continue
        bits, start, tiles = build(H, a)
        tp = tiles.ctypes.data_as(u32p)
        for qb in range(len(start) - 1):
            kbs = tiles[start[qb]:start[qb + 1], 0].astype(np.int64)
            for n in range(1, L + 1):
                got = H.tf_mask16_corner(tp, int(start[qb]), int(start[qb + 1]), n)
                assert got == int((kbs * 64 < n).sum()), (name, qb, n)
                assert (kbs[:got] * 64 < n).all(), "a prefix"
                if qb * 128 >= n or not (n == L or n % 37 == 0 or n in (1, 33, 65)):
                    continue
                if a[:n, :n].any(axis=1).all():                                   # a length the entry points accept
                    assert got >= 1
                for e in range(start[qb], start[qb] + got):
                    for s in range(2):
                        kb = int(tiles[e, 0]) * 64 + 32 * s
                        if kb >= n:
                            continue
                        for w in range(4):
                            if H.tf_mask16_class(int(tiles[e, 3]), w, s) != 1:
                                continue
                            for lane_q in range(32):
                                query = qb * 128 + 32 * w + lane_q
                                idx = H.tf_mask16_lane_word(L, n, query, kb)
                                assert idx == min(query, n - 1) * nw + kb // 32 and 0 <= idx < L * nw, (name, qb, n, query, kb)
    seen = sorted(H.tf_mask16_lane_bit(u, g, q) for u in range(2) for g in range(4) for q in range(4))
    assert seen == list(range(32))
    assert all(H.tf_mask16_lane_bit(u, g, q) == 16 * u + 4 * g + q for u in range(2) for g in range(4) for q in range(4))


def test_lane_word_holds_the_keys_of_its_step(H):
    """bit tf_mask_lane_bit(u, g, q) of word tf_mask_lane_word is the allowed bit of key kb + 16 u + 4 g + q"""
    L = 129
    a = next(m for name, m in masks(L) if name == "random0.4")
    bits, _, _ = build(H, a)
    for query in (0, 31, 32, 100, 128):
        for kb in (0, 32, 64, 96, 128):
            word = int(bits[H.tf_mask16_lane_word(L, L, query, kb)])
            for u in range(2):
                for g in range(4):
                    for q in range(4):
                        key = kb + 16 * u + 4 * g + q
                        assert (word >> H.tf_mask16_lane_bit(u, g, q)) & 1 == (int(a[query, key]) if key < L else 0)


# ---- 3. the pick, the launch, the allocation ----------------------------------------------------------------------------------------------
def test_pick_written_out(H):
    assert H.tf_mask16_attn_id() == 5
    for dtype in (DT_BF16, DT_F16, DT_F32):
        for hd in (6, 16, 32, 48, 64, 96, 128, 160, 256):
            for generic in (0, 1):
                for opt in (0, 1):
                    for aligned in (0, 1):
                        want = 5 if (dtype in (DT_BF16, DT_F16) and opt == 1 and generic == 0 and hd in (32, 64, 96, 128) and aligned == 1) else 4
                        assert H.tf_mask16_pick(dtype, hd, generic, opt, aligned) == want, (dtype, hd, generic, opt, aligned)


def test_launch_is_the_tiled_one(H):
    for hd, lds in ((32, 16384), (64, 32768), (96, 49152), (128, 65536)):
        for max_len in (1, 127, 128, 129, 300, 2048):
            out = (C.c_long * 4)()
            H.tf_mask16_launch(hd, 3, 2, max_len, out)
            assert tuple(out) == (6, (max_len + 127) // 128, 256, lds)          # grid (B H, query blocks), 4 waves, the ring alone


def test_device_layout(H):
    for L in LENGTHS:
        nw, nqb = (L + 31) // 32, (L + 127) // 128
        out = (C.c_longlong * 3)()
        H.tf_mask16_dev_layout(L, 11, out)
        assert out[0] == (L * nw + 2 * L) * 4                                    # bits | first | last | start | entries
        assert out[1] % 16 == 0 and out[0] + (nqb + 1) * 4 <= out[1] < out[0] + (nqb + 1) * 4 + 16
        assert out[2] == out[1] + 11 * 16


# ---- 4. the same under AddressSanitizer + UBSan, as a program of its own --------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """the tile map once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_mask16_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_MASK16_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_harness", "harness_tf_mask16.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "130 masks, 0 failures" in r.stdout
