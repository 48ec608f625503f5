"""The guarded mode (flope_amd/csrc/guard.hip) as far as a CPU can see it.

1.  The conditioning figure gap(M) = s2 + sign(det M) s3 of pose_math.h (procrustes_gap3x3, the code the select kernel runs per
    crop) through tests/host_harness/harness_guard.cpp, against torch.linalg.svdvals + det in float64.  Tolerance 8 u |M|_F with
    u = 2^-24: the result is a float32 of magnitude <= sqrt(2) |M|_F computed in float64.
2.  The flag predicate !(gap >= gap_min): NaN and -inf are flagged, +inf and gap == gap_min are not.
3.  PoseResNet(compute_dtype="guard") without a GPU: constructs, keeps the reference's 124 keys, refuses a CPU tensor.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def guard():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_guard.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_guard.so"])
    lib = C.CDLL(path)
    lib.guard_flagged.argtypes = [C.c_float, C.c_float]
    return lib


def _gap(lib, M):
    """M: float32 tensor [n,3,3] -> float32 numpy [n] by the shared host / device code"""
    a = np.ascontiguousarray(M.reshape(-1, 9).numpy(), dtype=np.float32)
    out = np.empty(a.shape[0], dtype=np.float32)
    lib.guard_gap(a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def _gap_ref(M):
    """float64: s2 + sign(det M) s3 and |M|_F of the float32 matrices as given"""
    Md = M.double().reshape(-1, 3, 3)
    s = torch.linalg.svdvals(Md)
    return (s[:, 1] + torch.sign(torch.linalg.det(Md)) * s[:, 2]).numpy(), Md.flatten(1).norm(dim=1).numpy()


def _check(lib, M, what):
    got = _gap(lib, M).astype(np.float64)
    ref, fro = _gap_ref(M)
    ratio = np.abs(got - ref) / (8 * U * fro)
    worst = int(np.argmax(ratio))
    print(f"{what}: {len(got)} matrices, worst |err| / (8 u |M|_F) = {ratio[worst]:.4f} at gap/|M|_F = {ref[worst] / fro[worst]:.3e}")
    assert np.isfinite(got).all() and (ratio <= 1.0).all(), (what, worst, got[worst], ref[worst])


# ---- 1. the conditioning figure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_gap_on_random_matrices_of_both_orientations(guard, scale):
    g = torch.Generator().manual_seed(20)
    M = torch.randn(10000, 3, 3, generator=g) * scale
    det = torch.linalg.det(M.double())
    assert int((det > 0).sum()) > 4000 and int((det < 0).sum()) > 4000
    _check(guard, M, f"random, scale {scale:g}")


def _rotations(n, g):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2)).unsqueeze(1)
    return q * torch.sign(torch.linalg.det(q)).view(-1, 1, 1)


def test_gap_where_the_eigenvalues_crowd(guard):
    """What a trained head emits (near-rotations: l2 = l3 = l4 of Horn's N), what the guard exists for (small gaps down to zero:
    l1 -> l2, the Jacobi fallback), and reflections of both (all of the top three eigenvalues close)."""
    g = torch.Generator().manual_seed(21)
    n = 2000
    U_, V_ = _rotations(n, g), _rotations(n, g)
    sets = {}
    sets["near-rotations"] = (U_ + 1e-3 * torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    for k, eps in enumerate((1e-1, 1e-3, 1e-5, 1e-7, 0.0)):
        s = torch.rand(n, 3, generator=g, dtype=torch.float64)
        s[:, 0] += 0.5
        s[:, 1:] *= eps                                                      # s2 + s3 of order eps
        sets[f"s2, s3 of order {eps:g}"] = U_ @ torch.diag_embed(s) @ V_.transpose(1, 2)
    s = 1.0 + 1e-4 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    s[:, 2] *= -1
    sets["near-reflections"] = U_ @ torch.diag_embed(s) @ V_.transpose(1, 2)
    s = torch.rand(n, 3, generator=g, dtype=torch.float64) + 0.2
    s[:, 1] = s[:, 0] * (1 + 1e-9 * torch.randn(n, generator=g, dtype=torch.float64))
    sets["s1 = s2"] = U_ @ torch.diag_embed(s) @ V_.transpose(1, 2)
    for what, M in sets.items():
        _check(guard, M.float(), what)


def test_gap_known_answers(guard):
    R = _rotations(1, torch.Generator().manual_seed(22))[0].float()
    d = lambda *v: torch.diag(torch.tensor(v, dtype=torch.float32))     # noqa: E731
    cases = [(R, 2.0), (d(3, 2, 1), 3.0), (d(3, 2, -1), 1.0), (d(1, 1, -1), 0.0), (d(2, 1, 1), 2.0), (d(1, 1, 1) * 0.37, 0.74),
             (d(1, 1, 1) * 5e4, 1e5), (-d(1, 1, 1), 0.0), (d(2, 2, 1), 3.0), (d(2, 2, -1), 1.0)]
    for M, want in cases:
        got = float(_gap(guard, M[None])[0])
        assert abs(got - want) <= 8 * U * float(M.double().norm()), (M, got, want)
    _check(guard, torch.stack([M for M, _ in cases]), "known answers")
    # rank 1 and zero: gap 0 (or non-finite) -- flagged either way
    v = torch.tensor([[1.0, -2.0, 0.5]])
    rank1 = (v.T @ torch.tensor([[0.3, 0.1, -0.7]]))
    for M in (rank1, torch.zeros(3, 3)):
        got = float(_gap(guard, M[None])[0])
        assert guard.guard_flagged(got, 0.5) == 1
        assert not math.isfinite(got) or abs(got) <= 8 * U * float(M.double().norm()), got
    # a non-finite M is flagged
    for bad in (float("nan"), float("inf"), -float("inf")):
        M = torch.eye(3)
        M[1, 2] = bad
        assert guard.guard_flagged(float(_gap(guard, M[None])[0]), 0.5) == 1
    # the whole float32 range: no overflow in the intermediate squares
    for s in (1e-30, 1e30):
        got = float(_gap(guard, (R * s)[None])[0])
        assert abs(got - 2.0 * s) <= 8 * U * s * math.sqrt(3.0) * 1.001, (s, got)


# ---- 2. the flag predicate -----------------------------------------------------------------------------------------------------------
def test_flag_predicate(guard):
    gm = 0.5
    below = float(np.nextafter(np.float32(gm), np.float32(0)))
    assert guard.guard_flagged(float("nan"), gm) == 1
    assert guard.guard_flagged(-float("inf"), gm) == 1
    assert guard.guard_flagged(float("inf"), gm) == 0
    assert guard.guard_flagged(gm, gm) == 0                     # gap == gap_min: not flagged
    assert guard.guard_flagged(below, gm) == 1                  # one float32 below: flagged
    assert guard.guard_flagged(0.0, gm) == 1 and guard.guard_flagged(2.0, gm) == 0
    assert guard.guard_flagged(2.0, float("nan")) == 1          # a NaN threshold trusts nothing
    assert guard.guard_flagged(2.0, 1e9) == 1 and guard.guard_flagged(0.0, 0.0) == 0


# ---- 3. the module without a GPU --------------------------------------------------------------------------------------------------------
def test_posenet_module_in_guard_mode_without_a_gpu(state_dict, monkeypatch):
    from sunflower.models.posenet import PoseResNet
    net = PoseResNet(compute_dtype="guard")
    assert net.compute_dtype == "guard"
    assert len(net.state_dict()) == 124 and set(net.state_dict()) == set(state_dict)
    net.load_state_dict(state_dict)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.rand(1, 3, 224, 224))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.predict_rotations(torch.rand(1, 3, 224, 224))
    monkeypatch.setenv("FLOPE_DTYPE", "guard")
    assert PoseResNet().compute_dtype == "guard"
    if not torch.cuda.is_available():
        from flope_amd.engine import GuardedPoseEngine
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            GuardedPoseEngine(224, 224, 4)
