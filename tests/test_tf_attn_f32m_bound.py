"""The element-wise checker of the float32 MFMA attention (tests/tf_attn_f32m_bound.py) must bite: both assertions
pass an emulation of the kernel's own passes on every shape the device test uses, and a pinned table says on which (shape, data kind)
each planted error fails which assertion, so that a later loosening of the bound shows as a diff.  CPU only; the same reference
and bounds judge the device in tests/test_gpu_tf_attn_f32m.py.  Every test prints its figures (-s).
"""
import ctypes as C
import os
import subprocess

import pytest
import torch

import tf_attn_f32m_bound as FB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_attn.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_attn.so"])
    return C.CDLL(path)


PLAN = _plan()
# the largest L of kernel id 3 per NT: (head_dim, causal); the head dims of NT 1, 4, 8
LIMIT_CASES = [(4, False), (4, True), (36, False), (128, False)]

# the shapes on which a defect changes any output at all
APPLIES = {
    "p16": lambda c: c.L > 1,
    "pbf": lambda c: c.L > 1,
    "opnd10": lambda c: c.L > 1,
    "scale64": lambda c: c.L > 1 and c.hd != 64,
    "nomask": lambda c: c.L > 1 and c.L % 16 != 0,        # one key: the copies of key 0 carry its own value
    "pair": lambda c: c.L > 64,                           # a fifth tile
    "wave3": lambda c: c.L > 12,                          # wave 3's first group is keys 12 .. 15
    "qfrag": lambda c: c.L > 1 and c.hd % 16 != 0,
    "head0v": lambda c: c.H > 1,
    "causal_lt": lambda c: True,                          # under is_causal; one key: 0 instead of v[0]
    "noshfl8": lambda c: c.L > 8,                         # lanes 8 .. 15 hold a term
}
# the smallest (L, head_dim) of the table at which each defect changes anything: it must be caught there
SMALLEST = {"scale64": (15, 4), "nomask": (15, 4), "pair": (65, 36), "wave3": (15, 4), "qfrag": (15, 4), "head0v": (1, 4),
            "causal_lt": (1, 4), "noshfl8": (15, 4)}

# mutation -> {(L, head_dim): one letter per data kind of that shape (normal, peaked, offset; the large shapes: normal alone)}
#   b = fails both assertions, 1 = assertion 1 alone, 2 = assertion 2 alone, - = passes both
# Every defect fails BOTH assertions on every shape and data kind on which it changes anything, but for the entries below: f16
# probabilities at the widest heads, where (hd + 5) a_i has grown to the size of 2^-11 / 2^-24 -- the worst element is back under
# its bound (0.79 and 0.63 of it) and the statistic still says no (3.3 and 1.3 times the yardstick).
NOT_BOTH = {"p16": {(16, 100): "b2b", (577, 128): "2"}}
PINNED = {m: {**{(c.L, c.hd): "b" * (3 if c.L <= 33 else 1) for c in FB.CASES if APPLIES[m](c)}, **NOT_BOTH.get(m, {})} for m in APPLIES}


def _letter(r1, r2):
    return "b" if r1 > 1.0 and r2 > 1.0 else "1" if r1 > 1.0 else "2" if r2 > 1.0 else "-"


def _table(mutation):
    causal = mutation == "causal_lt"
    out = {}
    for c in FB.CASES:
        if not APPLIES[mutation](c):
            continue
        qkv = FB.make_qkv(c.kind, c.B, c.L, c.H, c.hd)
        r1, where, r2 = FB.verdict(FB.emulate(qkv, c.H, causal=causal, mutation=mutation), FB.reference(c, causal))
        print(f"{mutation:9s} {FB.case_id(c)}: max err / bound {r1:.3g} at {where}, relL2 / yardstick {r2:.3g}")
        out[(c.L, c.hd)] = out.get((c.L, c.hd), "") + _letter(r1, r2)
    return out


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    assert {c.hd for c in FB.CASES} == {4, 12, 16, 20, 32, 36, 64, 68, 100, 128}
    assert {c.L for c in FB.CASES} == {1, 15, 16, 17, 33, 64, 65, 129, 257, 577}
    assert {FB.nt_of(c.hd) for c in FB.CASES} == {FB.nt_of(hd) for hd, _ in FB.RAGGED_CASES} == {1, 2, 4, 8}
    assert all(c.H >= 2 for c in FB.CASES) and all(c.B >= 2 for c in FB.CASES if c.L <= 129)
    assert all({k for c in FB.CASES if (c.L, c.hd) == (L, hd) for k in [c.kind]} == set(FB.KINDS)
               for L, hd in {(c.L, c.hd) for c in FB.CASES if c.L <= 33})
    assert all(any(f(c) for c in FB.CASES) for f in APPLIES.values())
    assert 12 <= len({(c.L, c.hd) for c in FB.CASES}) <= 24


@pytest.mark.parametrize("causal", [False, True], ids=["fixed", "causal"])
@pytest.mark.parametrize("case", FB.CASES, ids=FB.case_id)
def test_unbroken_emulation_is_within_both_assertions(case, causal):
    qkv = FB.make_qkv(case.kind, case.B, case.L, case.H, case.hd)
    j = FB.reference(case, causal)
    r1, where, r2 = FB.verdict(FB.emulate(qkv, case.H, causal=causal), j)
    print(f"{FB.case_id(case)} causal={int(causal)}: max err / bound {r1:.4f} at {where} (headroom {1 / max(r1, 1e-4):.1f} x), "
          f"relL2 / yardstick {r2:.4f} (headroom {1 / max(r2, 1e-4):.1f} x)")
    assert r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("causal", [False, True], ids=["ragged", "ragged-causal"])
@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("hd,kind", FB.RAGGED_CASES)
def test_unbroken_emulation_of_a_ragged_batch(hd, kind, reverse, causal):
    lengths = FB.RAGGED[::-1] if reverse else FB.RAGGED
    qkv = torch.cat(FB.make_ragged(kind, lengths, 2, hd))
    r1, where, r2 = FB.verdict(FB.emulate(qkv, 2, lengths=lengths, causal=causal), FB.reference_ragged(kind, lengths, 2, hd, causal))
    print(f"hd={hd} {kind} lengths={lengths} causal={int(causal)}: max err / bound {r1:.4f} at {where}, relL2 / yardstick {r2:.4f}")
    assert r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("hd,causal", LIMIT_CASES)
def test_unbroken_emulation_at_the_lds_limit(hd, causal):
    L = FB.lds_limit(PLAN, hd)
    assert PLAN.tf_attn_pick(2, hd, L + 1, 0, 1, 0, 1) == 0
    case = FB.Case(1, L, 2, hd, "normal")
    r1, where, r2 = FB.verdict(FB.emulate(FB.make_qkv(*case[4:], *case[:4]), 2, causal=causal), FB.reference(case, causal))
    print(f"{FB.case_id(case)} causal={int(causal)}: max err / bound {r1:.4f} at {where}, relL2 / yardstick {r2:.4f}")
    assert r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("mutation", [m for m in FB.MUTATIONS if m != "rowL"])
def test_broken_emulations_fail_where_the_table_says(mutation):
    got = _table(mutation)
    assert got == PINNED[mutation], got
    if mutation in ("p16", "pbf", "opnd10"):        # a float32 mode that is quietly a 16-bit mode: assertion 1 at every small shape
        small = {k: v for k, v in got.items() if k[0] <= 33 and k[1] <= 20}
        assert len(small) >= 9 and all(set(v) <= {"b", "1"} and len(v) == 3 for v in small.values()), small
    else:
        assert all(ch != "-" for ch in got[SMALLEST[mutation]]), (mutation, SMALLEST[mutation])


def test_a_clamp_by_the_longest_sequence_reads_past_the_batch():
    """rowL: the value pass multiplies the rows behind a short sequence by probabilities of 0; behind the last sequence of the batch
    those rows are NaN, so the sequence's outputs are not finite -- in either order of the batch."""
    for lengths in (FB.RAGGED, FB.RAGGED[::-1]):
        for causal in (False, True):
            qkv = torch.cat(FB.make_ragged("normal", lengths, 2, 12))
            got = FB.emulate(qkv, 2, lengths=lengths, causal=causal, mutation="rowL")
            r1, where, r2 = FB.verdict(got, FB.reference_ragged("normal", lengths, 2, 12, causal))
            print(f"rowL lengths={lengths} causal={int(causal)}: max err / bound {r1} at {where}")
            assert r1 == float("inf") and r2 == float("inf")
            T, row0 = sum(lengths), 0
            for n in lengths:                              # a sequence whose padded tile stays inside the batch reads finite rows times 0
                past = row0 + min((n + 15) // 16 * 16, max(lengths)) > T
                assert bool(torch.isfinite(got[row0:row0 + n]).all()) != past, (lengths, row0)
                row0 += n
            assert past                                    # the last sequence always reaches the NaN rows


def test_a_non_finite_output_is_infinitely_wrong():
    c = FB.CASES[3]
    got = FB.emulate(FB.make_qkv(c.kind, c.B, c.L, c.H, c.hd), c.H).clone()
    got[1, 5, 2] = float("nan")
    r1, where, r2 = FB.verdict(got, FB.reference(c))
    assert r1 == float("inf") and where == (1, 5, 2) and r2 == float("inf")
