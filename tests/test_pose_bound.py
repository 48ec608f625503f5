"""What the bounds of tests/pose_bound.py pass and what they catch, on the CPU.

1.  The golden file equals a regenerated sample of every class (inputs in bits, references to 1e-15), and the float64 and the
    mpmath reference agree on the well-conditioned classes.
2.  No case outside `degenerate` lies below gap / |M|_F = 1e-10, and the lowest a b (pose_bound's Newton term) is printed.
3.  The host compile of pose_math.h (through tests/host_harness) and the numpy emulation pass every class: Procrustes within the
    conditioning-scaled bound, every finite input a rotation, rotations and scaled rotations returned as themselves, the yaw-null
    within its bound with column 2 in bits and R itself at R00 = R01 = 0, the gap within 8 u |M|_F.
4.  Each broken copy of the emulation fails on at least one class; the test prints which, and asserts the table below.  Every class
    is needed by at least one mutation, or its purpose is stated in NOT_HIT.
"""
import ctypes as C

import numpy as np
import pytest

import pose_bound as PB
import pose_cases as PC

FP = C.POINTER(C.c_float)

# mutation -> classes it must fail on (it may fail on more; the test prints the full list)
MUST_FAIL = {
    "polar": ["sv_1e-1_neg", "sv_1e-3_neg", "reflections", "near_reflections", "gauss_1"],         # det < 0: a reflection comes back
    "transposed": ["gauss_1", "near_rotations", "sv_1e-1_pos", "s1_eq_s2", "s2_eq_s3", "signed_perms", "rotations", "gauss_1e-20", "gauss_1e20"],
    "float32": ["sv_1e-3_pos", "sv_1e-5_pos", "sv_1e-5_neg", "sv_1e-7_pos", "sv_1e-7_neg", "gauss_1e-36", "gauss_1e-32", "gauss_1e31", "gauss_1e37"],
    "second_eig": ["sv_1e-5_pos", "sv_1e-5_neg", "sv_1e-7_pos", "sv_1e-7_neg", "near_reflections"],
    "unnormalised": ["gauss_1", "near_rotations", "sv_1e-1_pos", "rotations"],
    "atan2_sign": ["yaw_rotations", "yaw_scaled", "yaw_tiny"],
    "rz": ["yaw_rotations", "yaw_scaled", "yaw_tiny"],
}
# classes no mutation has to fail on, and why they are there
NOT_HIT = {
    "degenerate": "no unique answer below the 1e-10 line: every finite input must still come back a rotation, from a bounded loop",
    "nonfinite": "GPU only: the call returns and the finite rows of the batch keep their bits",
    "yaw_zero": "the n = 0 branch: the output is the input in bits (both yaw mutations are the identity there)",
    "yaw_pi": "yaw of exactly +-pi with both signs of a zero R01: c = -1, s = +-0; the mutations differ in the sign of zeros only",
}


@pytest.fixture(scope="module")
def gold():
    return PC.load_goldens()


def _host_procrustes(h, M):
    R, path = np.empty_like(M), np.empty(len(M), dtype=np.uint8)
    h.hh_procrustes_paths(M.ctypes.data_as(FP), R.ctypes.data_as(FP), path.ctypes.data_as(C.POINTER(C.c_ubyte)), len(M))
    return R, path.astype(bool)


def _host_yaw(h, R):
    O = np.empty_like(R)
    h.hh_nullify_yaw(R.ctypes.data_as(FP), O.ctypes.data_as(FP), len(R))
    return O


def _procrustes_failures(gold, c, R):
    """-> (list of reasons the class fails, worst err / bound, worst rotation defect)"""
    M, Rr, gap, fro = gold[f"M/{c}"], gold[f"R/{c}"], gold[f"gap/{c}"], gold[f"fro/{c}"]
    ratio, acc = PB.judge_procrustes(R, Rr, gap, fro, PB.newton_ab(M, gap, fro))
    o, d = PB.rotation_defect(R)
    why = []
    if ratio.max() > 1:
        why.append(f"err / bound {ratio.max():.3g} at row {int(ratio.argmax())}")
    if max(o.max(), d.max()) > 1:
        why.append(f"not a rotation: |R R^T - I| / bound {o.max():.3g}, |det R - 1| / bound {d.max():.3g}")
    return why, float(ratio.max()), float(max(o.max(), d.max())), int(acc.sum())


def _yaw_failures(gold, c, O):
    R, Oref = gold[f"yawR/{c}"], gold[f"yawO/{c}"]
    ratio = PB.judge_yaw(O, Oref, R)
    why = [f"err / bound {ratio.max():.3g} at row {int(ratio.argmax())}"] if ratio.max() > 1 else []
    o01 = np.abs(O[:, 0, 1].astype(np.float64)) / (PB.K_YAW * PB.U64 * (np.abs(R[:, 0, 0].astype(np.float64)) + np.abs(R[:, 0, 1].astype(np.float64))) + PB.SUB32)
    if o01.max() > 1:
        why.append(f"|O01| / bound {o01.max():.3g}")
    if c == "yaw_zero" and not (O.view(np.uint32) == R.view(np.uint32)).all():
        why.append("R00 = R01 = 0: the output is not R in bits")
    return why, float(ratio.max())


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_golden_file_matches_a_regenerated_sample_and_the_two_references_agree(gold):
    pytest.importorskip("mpmath")
    take = slice(0, 64, 7)
    for c in PC.PROCRUSTES_CLASSES:
        M = PC.procrustes_class(c)
        assert (M.view(np.uint32) == gold[f"M/{c}"].view(np.uint32)).all(), c
        if c == "nonfinite":
            continue
        R, gap, fro, _ = PC.procrustes_reference(M[take])
        acc = gap / np.where(fro > 0, fro, 1) >= PC.ROTATION_ONLY_BELOW
        assert np.abs(R - gold[f"R/{c}"][take])[acc].max(initial=0) <= 1e-15 and np.allclose(gap, gold[f"gap/{c}"][take], rtol=1e-12, atol=0) and \
            np.array_equal(fro, gold[f"fro/{c}"][take]), c
        if c in PC.ACCURACY_CLASSES and gold[f"gap/{c}"].min() / gold[f"fro/{c}"].max() >= 1e-3:
            R64, g64, _, _ = PC.procrustes_reference(M[take], "f64")
            Rmp, gmp, _, _ = PC.procrustes_reference(M[take], "mp")
            # float64 SVD: backward stable, so its R is off by some 10 e |M| / gap; 64 is room for LAPACK's constant
            lim = 64 * PB.U64 * (gold[f"fro/{c}"][take] / gold[f"gap/{c}"][take])[:, None, None] + 4 * PB.U64
            assert (np.abs(R64 - Rmp) <= lim).all() and np.allclose(g64, gmp, rtol=1e-11), c
    for c in PC.YAW_CLASSES:
        R = PC.yaw_class(c)
        assert (R.view(np.uint32) == gold[f"yawR/{c}"].view(np.uint32)).all(), c
        assert np.array_equal(PC.yaw_reference(R[take]), gold[f"yawO/{c}"][take]), c


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
def test_no_accuracy_class_falls_below_the_line(gold):
    lowest, ab = {}, {}
    for c in PC.ACCURACY_CLASSES:
        M, gap, fro = gold[f"M/{c}"], gold[f"gap/{c}"], gold[f"fro/{c}"]
        lowest[c] = float((gap / fro).min())
        assert lowest[c] >= PC.ROTATION_ONLY_BELOW, (c, lowest[c])
        ab[c] = float(PB.newton_ab(M, gap, fro).min())
    print("lowest gap / |M|_F:", {c: f"{v:.2e}" for c, v in lowest.items()})
    print(f"lowest of all: {min(lowest.values()):.2e}; lowest a b where the fast path is possible: {min(ab.values()):.3g} in {min(ab, key=ab.get)} "
          f"(C of that row: {max(PB.C_JACOBI, 3120 + 126 / min(1.0, min(ab.values()))):.0f})")


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
def test_host_compile_and_emulation_pass_every_class(harness, gold):
    bad = []
    print(f"C = {PB.C:.0f} (Jacobi {PB.C_JACOBI:.0f}, Newton {PB.C_NEWTON:.0f})")
    for c in PC.FINITE_CLASSES:
        M = gold[f"M/{c}"]
        Rh, path = _host_procrustes(harness, M)
        Re, pe = PB.emulate_procrustes(M)
        (wh, rh, dh, nacc), (we, re_, de, _) = _procrustes_failures(gold, c, Rh), _procrustes_failures(gold, c, Re)
        print(f"{c:17s} {len(M):3d} rows ({nacc:2d} for accuracy)  host: err/bound {rh:.3f} rotation {dh:.3f} fallback {100 * (1 - path.mean()):3.0f} %   "
              f"emulation: err/bound {re_:.3f} rotation {de:.3f} fallback {100 * (1 - pe.mean()):3.0f} %")
        bad += [f"{c} (host): {w}" for w in wh] + [f"{c} (emulation): {w}" for w in we]
        if c in ("rotations", "signed_perms"):
            # a rotation comes back as itself: the input is a float32 rounding of a rotation, so R_ref is within u of it
            for s in (1.0, 0.37, 5e4):
                Rs, _ = _host_procrustes(harness, np.ascontiguousarray(M * np.float32(s)))
                if np.abs(Rs.astype(np.float64) - M).max() > 3 * PB.U32:
                    bad.append(f"{c} x {s}: a scaled rotation does not come back as the rotation")
    for c in PC.YAW_CLASSES:
        R = gold[f"yawR/{c}"]
        (wh, rh), (we, re_) = _yaw_failures(gold, c, _host_yaw(harness, R)), _yaw_failures(gold, c, PB.emulate_yaw(R))
        print(f"{c:17s} {len(R):3d} rows  host: err/bound {rh:.3f}   emulation: err/bound {re_:.3f}")
        bad += [f"{c} (host): {w}" for w in wh] + [f"{c} (emulation): {w}" for w in we]
    # the conditioning figure, at the project's tolerance
    for c in PC.FINITE_CLASSES:
        M, gap, fro = gold[f"M/{c}"], gold[f"gap/{c}"], gold[f"fro/{c}"]
        g = np.empty(len(M), dtype=np.float32)
        harness.hh_gap(M.ctypes.data_as(FP), g.ctypes.data_as(FP), len(M))
        r = np.abs(g.astype(np.float64) - gap) / np.where(fro > 0, PB.GAP_TOL * fro, 1.0)
        if not (np.isfinite(g).all() and r.max() <= 1):
            bad.append(f"{c}: gap off by {r.max():.3g} x 8 u |M|_F")
    assert not bad, "\n".join(bad)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def test_every_broken_copy_fails_where_stated(gold):
    table = {}
    for mu in PB.PROCRUSTES_MUTATIONS:
        table[mu] = [c for c in PC.FINITE_CLASSES if _procrustes_failures(gold, c, PB.emulate_procrustes(gold[f"M/{c}"], mu)[0])[0]]
    for mu in PB.YAW_MUTATIONS:
        table[mu] = [c for c in PC.YAW_CLASSES if _yaw_failures(gold, c, PB.emulate_yaw(gold[f"yawR/{c}"], mu))[0]]
    for mu, cs in table.items():
        print(f"{mu:13s} fails on {len(cs):2d} classes: {' '.join(cs)}")
    for mu, need in MUST_FAIL.items():
        missing = [c for c in need if c not in table[mu]]
        assert table[mu] and not missing, f"{mu} passes {missing}"
    hit = {c for cs in table.values() for c in cs}
    for c in PC.PROCRUSTES_CLASSES + PC.YAW_CLASSES:
        assert c in hit or c in NOT_HIT, f"class {c} is needed by no mutation and has no stated purpose"
