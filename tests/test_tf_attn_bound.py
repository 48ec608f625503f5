"""The element-wise attention checker (tests/tf_attn_bound.py) must bite: it passes an emulation of the kernel's own steps on every
shape the device test uses, and fails copies of that emulation broken the way streaming attention kernels break, one defect at a
time.  CPU only; the same reference and bound judge the device in tests/test_gpu_tf_attn_tiled.py.  Every test prints its figures
(-s).
"""
import ctypes as C
import os
import subprocess

import pytest

import tf_attn_bound as AB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ring():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_tf_attn.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_tf_attn.so"])
    lib = C.CDLL(path)
    return lib.tf_attn_tiled_kb(), lib.tf_attn_tiled_ring()


KB, RING = _ring()
CASES = AB.cases(KB, RING)

# the shapes on which a defect can show at all
APPLIES = {
    "nomask": lambda B, L, H, hd: L % 32 != 0,
    "skip": lambda B, L, H, hd: L > 32,
    "twice": lambda B, L, H, hd: L > 32,
    "ring": lambda B, L, H, hd: L > KB * RING,
    "noalpha": lambda B, L, H, hd: L > 32,
    "head0v": lambda B, L, H, hd: H > 1,
    "dims64": lambda B, L, H, hd: hd == 128,
    "scale64": lambda B, L, H, hd: hd != 64,
}


def test_the_cases_cover_what_the_kernel_can_get_wrong():
    assert KB % 32 == 0 and RING >= 2
    Ls = [c[1] for c in CASES]
    assert 1 in Ls and KB * RING + 1 in Ls and KB * RING + 33 in Ls
    assert any(L > 128 for L in Ls)                                   # a second query block
    assert {c[3] for c in CASES} == {32, 64, 96, 128}
    assert all(any(f(*c) for c in CASES) for f in APPLIES.values())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_best_keys_fall_in_the_first_and_in_the_last_step(dtype):
    """Without queries whose maximum jumps in the last step a dropped rescale cannot show; without queries whose maximum is final
    after the first step the rescale is never the identity."""
    for B, L, H, hd in CASES:
        if L <= 32:
            continue
        steps = AB.best_key_steps(AB.make_qkv(B, L, H, hd, dtype), H)
        first, last = int((steps == 0).sum()), int((steps == (L - 1) // 32).sum())
        print(f"{dtype} B={B} L={L} H={H} hd={hd}: best key in the first step for {first} queries, in the last for {last}, of {steps.numel()}")
        assert first >= steps.numel() // 8 and last >= steps.numel() // 8


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-L%d-H%d-hd%d" % c)
def test_unbroken_emulation_is_within_the_bound(dtype, case):
    B, L, H, hd = case
    qkv = AB.make_qkv(B, L, H, hd, dtype)
    ref, bound = AB.reference(B, L, H, hd, dtype)
    r, where = AB.ratio(AB.emulate(qkv, H, dtype, kb=KB, ring=RING), ref, bound)
    print(f"{dtype} B={B} L={L} H={H} hd={hd}: max err / bound {r:.3f} at {where} (headroom {1 / max(r, 1e-3):.2f} x), "
          f"median bound / rms(O) {float(bound.median() / ref.pow(2).mean().sqrt()):.2e}")
    assert r <= 1.0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("mutation", AB.MUTATIONS)
def test_broken_emulations_fail_the_bound(dtype, mutation):
    caught = []
    for case in CASES:
        if not APPLIES[mutation](*case):
            continue
        B, L, H, hd = case
        qkv = AB.make_qkv(B, L, H, hd, dtype)
        ref, bound = AB.reference(B, L, H, hd, dtype)
        r, where = AB.ratio(AB.emulate(qkv, H, dtype, mutation=mutation, kb=KB, ring=RING), ref, bound)
        print(f"{mutation:8s} {dtype} B={B} L={L} H={H} hd={hd}: max err / bound {r:.3g} at {where}")
        if r > 1.0:
            caught.append(case)
    assert caught, f"no shape shows the defect {mutation}"


def test_a_non_finite_output_is_infinitely_wrong():
    B, L, H, hd = CASES[1]
    ref, bound = AB.reference(B, L, H, hd, "f16")
    got = AB.emulate(AB.make_qkv(B, L, H, hd, "f16"), H, "f16").clone()
    got[0, 5, 7] = float("nan")
    r, where = AB.ratio(got, ref, bound)
    assert r == float("inf") and where == (0, 5, 7)
