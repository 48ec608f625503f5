"""pose_math.h as the DEVICE compiles it (its own libm, FMA contraction), through the stand-alone kernels flope_procrustes,
flope_nullify_yaw and flope_compose_pose, on the named classes of tests/pose_cases.py within the bounds of tests/pose_bound.py.

The classes put on the GPU on purpose what the suite only ran on the host: the Jacobi fallback (scales outside the Newton path's
fro2 limits, gaps down to 2.5e-10 |M|_F), exact rotations with w = 0, det < 0 with a small gap, degenerate and non-finite inputs,
the yaw-null at R00 = R01 = 0, at denormal R00 / R01 and at exactly +-pi.  References come from tests/golden/pose_cases.npz.

Every launch writes into a buffer three rows longer than n, filled with a sentinel: those rows stay untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_bound as PB
import pose_cases as PC

pytestmark = pytest.mark.gpu

SENTINEL, TAIL = -7.25e11, 3
FP = C.POINTER(C.c_float)
SIZES = (1, 63, 64, 65, 129)          # a block is 64 threads


@pytest.fixture(scope="module")
def gold():
    return PC.load_goldens()


def _launch(fn, cols_out, n, *args):
    """fn(*args with "OUT" replaced by a sentinel-tailed output, stream) -> output rows [n, cols_out] on the CPU"""
    from flope_amd import _lib
    out = torch.full((n + TAIL, cols_out), SENTINEL, dtype=torch.float32, device="cuda")
    a = [out.data_ptr() if x == "OUT" else x for x in args]
    _lib.check(getattr(_lib.load(), fn)(*a, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[n:] == SENTINEL).all()), f"{fn}: a row behind the last one was written"
    return o[:n].numpy()


def _dev(a, cols):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)).cuda()


def dev_procrustes(M):
    d = _dev(M, 9)
    return _launch("flope_procrustes", 9, len(d), d.data_ptr(), "OUT", len(d)).reshape(-1, 3, 3)


def dev_yaw(R):
    d = _dev(R, 9)
    return _launch("flope_nullify_yaw", 9, len(d), d.data_ptr(), "OUT", len(d)).reshape(-1, 3, 3)


def dev_compose(R, xyz, nullify):
    d = _dev(R, 9)
    x = None if xyz is None else _dev(xyz, 3)
    return _launch("flope_compose_pose", 16, len(d), d.data_ptr(), x.data_ptr() if x is not None else None, len(d), int(nullify), "OUT").reshape(-1, 4, 4)


def _host_procrustes(h, M):
    M = np.ascontiguousarray(M, dtype=np.float32)
    R = np.empty_like(M)
    h.hh_procrustes(M.ctypes.data_as(FP), R.ctypes.data_as(FP), len(M))
    return R


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _judge(gold, c, R, rows=None):
    """-> (worst err / bound, worst rotation defect) of device rows R against class c's references (rows: which of the class)"""
    rows = slice(None) if rows is None else rows
    M, Rr, gap, fro = gold[f"M/{c}"][rows], gold[f"R/{c}"][rows], gold[f"gap/{c}"][rows], gold[f"fro/{c}"][rows]
    ratio, _ = PB.judge_procrustes(R, Rr, gap, fro, PB.newton_ab(M, gap, fro))
    o, d = PB.rotation_defect(R)
    return float(ratio.max()), float(max(o.max(), d.max()))


# ---- Procrustes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PC.FINITE_CLASSES)
def test_procrustes_class_within_its_bound_and_beside_the_host_compile(harness, gold, c):
    M, Rr, gap, fro = gold[f"M/{c}"], gold[f"R/{c}"], gold[f"gap/{c}"], gold[f"fro/{c}"]
    R = dev_procrustes(M)
    Rh = _host_procrustes(harness, M)
    rd, dd = _judge(gold, c, R)
    rh, dh = _judge(gold, c, Rh)
    same = float((_bits(R) == _bits(Rh)).all(axis=(1, 2)).mean())
    print(f"{c:17s} {len(M):3d} rows  device: err/bound {rd:.3f} rotation {dd:.3f}   host: err/bound {rh:.3f} rotation {dh:.3f}   rows equal in bits {100 * same:.0f} %")
    assert rd <= 1 and dd <= 1, (c, rd, dd)
    # the two compiles agree within the sum of their bounds (one bound each)
    bound = PB.procrustes_bound(Rr, gap, fro, PB.newton_ab(M, gap, fro))
    acc = np.isfinite(bound).all(axis=(1, 2))
    assert (np.abs(R.astype(np.float64) - Rh)[acc] <= 2 * bound[acc]).all(), c
    if c in ("rotations", "signed_perms"):
        for s in (1.0, 0.37, 5e4):
            assert np.abs(dev_procrustes(M * np.float32(s)).astype(np.float64) - M).max() <= 3 * PB.U32, (c, s, "a scaled rotation does not come back as the rotation")


def test_procrustes_rows_are_independent_of_their_neighbours_and_of_n(gold):
    """All finite classes dealt out row by row into one launch -- fast-path and fallback lanes share every wave -- give the bits of
    each class launched alone; so do the first n rows of that batch at every n around a block, and each row keeps its bound."""
    parts = [gold[f"M/{c}"] for c in PC.FINITE_CLASSES]
    mixed, order = PC.interleave(parts)
    alone = [dev_procrustes(p) for p in parts]
    want = np.stack([alone[ci][r] for ci, r in order])
    got = dev_procrustes(mixed)
    assert (_bits(got) == _bits(want)).all(), "a row's bits depend on the rows around it"
    for n in SIZES:
        g = dev_procrustes(mixed[:n])
        assert (_bits(g) == _bits(want[:n])).all(), n
        worst = max(_judge(gold, PC.FINITE_CLASSES[ci], g[i:i + 1], slice(r, r + 1)) for i, (ci, r) in enumerate(order[:n]))
        print(f"n = {n}: worst err/bound {worst[0]:.3f}, rotation {worst[1]:.3f}")
        assert worst[0] <= 1 and worst[1] <= 1, n


def test_non_finite_rows_leave_the_finite_rows_alone(gold):
    """The call returns (every loop of pose_math.h is bounded: 12 sweeps, 10 + 8 Newton steps) and the finite rows keep their bits.
    Nothing is asserted about the non-finite rows' values."""
    fin = np.concatenate([gold[f"M/{c}"][:8] for c in PC.FINITE_CLASSES])
    bad = gold["M/nonfinite"]
    mixed, order = PC.interleave([fin, bad])
    got = dev_procrustes(mixed)
    alone = dev_procrustes(fin)
    keep = np.array([i for i, (ci, _) in enumerate(order) if ci == 0])
    assert (_bits(got[keep]) == _bits(alone)).all()
    Ry = np.concatenate([gold[f"yawR/{c}"][:8] for c in PC.YAW_CLASSES])
    mixed, order = PC.interleave([Ry, bad])
    keep = np.array([i for i, (ci, _) in enumerate(order) if ci == 0])
    assert (_bits(dev_yaw(mixed)[keep]) == _bits(dev_yaw(Ry))).all()
    assert (_bits(dev_compose(mixed, None, True)[keep]) == _bits(dev_compose(Ry, None, True))).all()


# ---- yaw-null and pose assembly ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PC.YAW_CLASSES)
def test_yaw_null_class_within_its_bound(harness, gold, c):
    R, Oref = gold[f"yawR/{c}"], gold[f"yawO/{c}"]
    O = dev_yaw(R)
    Oh = np.empty_like(R)
    harness.hh_nullify_yaw(R.ctypes.data_as(FP), Oh.ctypes.data_as(FP), len(R))
    ratio, rh = PB.judge_yaw(O, Oref, R), PB.judge_yaw(Oh, Oref, R)
    o01 = np.abs(O[:, 0, 1].astype(np.float64)) / (PB.K_YAW * PB.U64 * (np.abs(R[:, 0, 0].astype(np.float64)) + np.abs(R[:, 0, 1].astype(np.float64))) + PB.SUB32)
    print(f"{c:14s} {len(R)} rows  device: err/bound {ratio.max():.3f}  |O01| / bound {o01.max():.3f}   host: err/bound {rh.max():.3f}   "
          f"rows equal in bits {100 * float((_bits(O) == _bits(Oh)).all(axis=(1, 2)).mean()):.0f} %")
    assert ratio.max() <= 1 and o01.max() <= 1, c
    assert (np.abs(O.astype(np.float64) - Oh) <= 2 * PB.yaw_bound(Oref, R)).all(), "device and host compile differ by more than their two bounds"
    if c == "yaw_zero":
        assert (_bits(O) == _bits(R)).all(), "R00 = R01 = 0: the output is not R in bits"
    for n in SIZES:
        assert (_bits(dev_yaw(R[np.arange(n) % len(R)])) == _bits(O[np.arange(n) % len(R)])).all(), n


def test_compose_pose_carries_bits(gold):
    R = np.concatenate([gold[f"yawR/{c}"] for c in PC.YAW_CLASSES])
    R = R[np.arange(129) % len(R)]
    xyz = np.random.default_rng(3).standard_normal((len(R), 3)).astype(np.float32)
    O = dev_yaw(R)
    for nullify in (0, 1):
        for x in (xyz, None):
            for n in SIZES:
                Rt = dev_compose(R[:n], None if x is None else x[:n], nullify)
                assert (_bits(Rt[:, :3, :3]) == _bits(O[:n] if nullify else R[:n])).all(), (nullify, n)
                assert (_bits(Rt[:, :3, 3]) == _bits(x[:n] if x is not None else np.zeros((n, 3)))).all(), (nullify, n)
                assert (_bits(Rt[:, 3]) == _bits(np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))).all(), (nullify, n)
