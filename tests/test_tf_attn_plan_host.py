"""Which attention kernel an encoder launch takes (flope_amd/csrc/tf_attn_plan.h, the one function flope_tf_forward and
flope_tf_attention go through), on the CPU through tests/host_harness/harness_tf_attn.cpp.

The table is checked over dtype x head_dim x seq_len x the three options x alignment.  With attn_tiled = 0 the choice must be the
one the two conditions made that stood inline in run_forward before the header existed; they are written out here literally:

    16-bit:   !opt_generic && d / H == 64 && Lp <= 512                      (Lp = (L + 31) / 32 * 32)       -> tf_attn_mfma
    float32:  opt_f32m && dh % 4 == 0 && dh <= 128 && lds <= 160 * 1024                                        -> tf_attn_f32m
              lds = (16 * (((L + 15) & ~15) + 4) + 3 * nt * 256) * 4,  nt = dh <= 16 ? 1 : dh <= 32 ? 2 : dh <= 64 ? 4 : 8
    otherwise tf_attn_generic
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_BF16, DT_F16, DT_F32 = 0, 1, 2
GENERIC, MFMA64, TILED, F32M = 0, 1, 2, 3
HEAD_DIMS = [8, 32, 40, 64, 96, 128, 160]
SEQ_LENS = [1, 512, 513, 577]


@pytest.fixture(scope="module")
def plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_attn.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_attn.so"])
    lib = C.CDLL(path)
    lib.tf_attn_lds_bytes.restype = C.c_long
    return lib


def parent_choice(dtype, dh, L, opt_generic, opt_f32m):
    """The two inline conditions of run_forward as they stood (buffers of the handle: always aligned)."""
    if dtype != DT_F32:
        Lp = (L + 31) // 32 * 32
        if (not opt_generic) and dh == 64 and Lp <= 512:
            return MFMA64
    if dtype == DT_F32:
        nt = 1 if dh <= 16 else 2 if dh <= 32 else 4 if dh <= 64 else 8
        lds = (16 * (((L + 15) & ~15) + 4) + 3 * nt * 256) * 4
        if opt_f32m and dh % 4 == 0 and dh <= 128 and lds <= 160 * 1024:
            return F32M
    return GENERIC


def test_ids_are_the_documented_ones(plan):
    assert [plan.tf_attn_id(i) for i in range(4)] == [GENERIC, MFMA64, TILED, F32M]
    assert plan.tf_attn_id(4) == -1


def test_option_zero_is_the_parents_choice(plan):
    n = 0
    for dtype, dh, L, g, f in itertools.product((DT_BF16, DT_F16, DT_F32), HEAD_DIMS, SEQ_LENS + [2500, 2600], (0, 1), (0, 1)):
        assert plan.tf_attn_pick(dtype, dh, L, g, f, 0, 1) == parent_choice(dtype, dh, L, g, f), (dtype, dh, L, g, f)
        n += 1
    assert n == 3 * 7 * 6 * 4
    # the parent's table has all three kernels in it (so the loop above compared something)
    assert parent_choice(DT_F16, 64, 512, 0, 0) == MFMA64 and parent_choice(DT_F16, 64, 513, 0, 0) == GENERIC
    assert parent_choice(DT_F32, 40, 577, 0, 1) == F32M and parent_choice(DT_F32, 40, 2600, 0, 1) == GENERIC


def expected(dtype, dh, L, g, f, t, aligned):
    """The rule of include/flope_amd.h ("attn_tiled"), written independently of the header."""
    if not aligned:
        return GENERIC
    base = parent_choice(dtype, dh, L, g, f)
    if dtype == DT_F32 or g:
        return base
    eligible = dh % 32 == 0 and dh <= 128
    if t == 1 and eligible and base == GENERIC:
        return TILED
    if t == 2 and eligible:
        return TILED
    return base


def test_whole_table(plan):
    seen = set()
    for dtype, dh, L, g, f, t, al in itertools.product((DT_BF16, DT_F16, DT_F32), HEAD_DIMS, SEQ_LENS, (0, 1), (0, 1), (0, 1, 2), (0, 1)):
        got = plan.tf_attn_pick(dtype, dh, L, g, f, t, al)
        assert got == expected(dtype, dh, L, g, f, t, al), (dtype, dh, L, g, f, t, al, got)
        seen.add(got)
    assert seen == {GENERIC, MFMA64, TILED, F32M}


@pytest.mark.parametrize("dtype", [DT_BF16, DT_F16])
def test_the_rule_in_words(plan, dtype):
    pick = lambda dh, L, t, g=0, al=1: plan.tf_attn_pick(dtype, dh, L, g, 0, t, al)
    # 1: only where the choice would be generic -- shapes the resident kernel takes keep it
    assert [pick(64, 512, t) for t in (0, 1, 2)] == [MFMA64, MFMA64, TILED]
    assert [pick(64, 513, t) for t in (0, 1, 2)] == [GENERIC, TILED, TILED]
    for dh in (32, 96, 128):
        for L in SEQ_LENS:
            assert [pick(dh, L, t) for t in (0, 1, 2)] == [GENERIC, TILED, TILED]
    # head widths the kernel is not built for
    for dh in (8, 40, 160):
        assert [pick(dh, 577, t) for t in (0, 1, 2)] == [GENERIC] * 3
    # generic = 1 and a misaligned pointer override everything
    assert all(pick(dh, L, t, g=1) == GENERIC for dh in HEAD_DIMS for L in SEQ_LENS for t in (0, 1, 2))
    assert all(pick(dh, L, t, al=0) == GENERIC for dh in HEAD_DIMS for L in SEQ_LENS for t in (0, 1, 2))


def test_float32_handles_ignore_the_option(plan):
    for dh, L, g, f in itertools.product(HEAD_DIMS, SEQ_LENS, (0, 1), (0, 1)):
        assert len({plan.tf_attn_pick(DT_F32, dh, L, g, f, t, 1) for t in (0, 1, 2)}) == 1
    # and 16-bit handles ignore f32mfma
    for dtype, dh, L, t in itertools.product((DT_BF16, DT_F16), HEAD_DIMS, SEQ_LENS, (0, 1, 2)):
        assert plan.tf_attn_pick(dtype, dh, L, 0, 0, t, 1) == plan.tf_attn_pick(dtype, dh, L, 0, 1, t, 1)


def test_lds_bytes_of_the_launches(plan):
    kb, ring = plan.tf_attn_tiled_kb(), plan.tf_attn_tiled_ring()
    assert kb % 32 == 0 and kb >= 32 and ring >= 2 and plan.tf_attn_tiled_queries() == 128
    for dh in (32, 64, 96, 128):
        lds = plan.tf_attn_lds_bytes(TILED, dh, 577)
        assert lds == ring * 2 * kb * dh * 2                      # ring x (K block + V block) x keys x row bytes
        assert lds <= 80 * 1024                                   # two workgroups share a CU
        assert lds == plan.tf_attn_lds_bytes(TILED, dh, 1)        # whatever the length
    assert plan.tf_attn_lds_bytes(MFMA64, 64, 512) == 512 * 256 == 131072       # what flope_tf_create allows tf_attn_mfma
    assert plan.tf_attn_lds_bytes(MFMA64, 64, 33) == 64 * 256
    assert plan.tf_attn_lds_bytes(F32M, 32, 50) == (16 * (64 + 4) + 3 * 2 * 256) * 4
    assert plan.tf_attn_lds_bytes(GENERIC, 40, 577) == 4 * 577 * 4
