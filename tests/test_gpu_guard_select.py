"""guard_select_kernel (flope_amd/csrc/guard.hip) beyond one wave and one pass.

The kernel is one workgroup of four waves that walks the batch in passes of 256 rows: a flagged row's place in the list is the
number of flagged rows in front of it -- inside its wave (ballot), in the waves before it (LDS) and in the passes before it
(the running base).  The guarded engine's own tests stop at B = 37, so neither the rank across waves (B > 64) nor the second pass
(B > 256) ever ran.  flope_guard_select_rows launches the kernel exactly as flope_guard_forward does, on a caller's M [n, 9]:

1.  the device's procrustes_gap3x3 on the classes of tests/pose_cases.py (the committed goldens) against a float64 SVD at the
    project's tolerance 8 u |M|_F (tests/test_guard_host.py); the gap-0 rows of `degenerate` are flagged at a positive threshold,
    its rank-2 rows (gap = s2 > 0) are not, non-finite rows are flagged at any;
2.  the list equals nonzero(~(gap >= gap_min)) of the device's own gaps, ascending, at n = 1, 64, 65, 256, 257 and 600, with gap_min
    at the median of those gaps (flagged and unflagged rows mix across waves and passes), at 0 and at 1e9; two runs give equal lists;
3.  one guarded forward at B = 300 with max_repair = 32 and gap_min at the median of a first run's gaps: unflagged rows carry the
    f16 engine's bits, flagged rows the f32m engine's (the assertion of tests/test_gpu_guard.py at 16 crops).
"""
import pytest
import torch

import pose_cases as PC

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _classes():
    """the Procrustes classes of tests/pose_cases.py from the committed goldens: name -> float32 [n, 3, 3]"""
    gold = PC.load_goldens()
    return {c: torch.from_numpy(gold[f"M/{c}"]) for c in PC.PROCRUSTES_CLASSES}


def _gap64(M):
    Md = M.double().reshape(-1, 3, 3)
    s = torch.linalg.svdvals(Md)
    return s[:, 1] + torch.sign(torch.linalg.det(Md)) * s[:, 2], Md.flatten(1).norm(dim=1)


def _select(M, gap_min):
    from flope_amd.engine import guard_select_rows
    gap, sel, count = guard_select_rows(M.cuda(), gap_min)
    sel = sel.cpu()
    assert int(sel[0]) == count, (int(sel[0]), count)
    return gap.cpu(), sel[1:1 + count].tolist(), sel[1 + count:]


def _flagged(gap, gap_min):
    return torch.nonzero(~(gap >= gap_min)).flatten().tolist()


def test_device_gap_on_every_class_and_the_degenerate_rows_are_flagged():
    for name, M in _classes().items():
        gap_min = 0.0 if name == "nonfinite" else 1e-3 * float(M.abs().max())        # positive, in M's own units
        gap, sel, rest = _select(M, gap_min)
        assert bool((rest == -1).all()), f"{name}: entries behind the list were written"
        assert sel == _flagged(gap, gap_min), name
        if name == "nonfinite":
            assert bool(torch.isnan(gap).all()) and sel == list(range(len(M))), "a non-finite M must be flagged at any threshold"
            print(f"{name}: {len(M)} rows, all NaN, all flagged")
            continue
        want, fro = _gap64(M)
        ratio = (gap.double() - want).abs() / (8 * U * fro).clamp_min(1e-300)
        ratio[fro == 0] = gap[fro == 0].double().abs()                      # the zero matrix: gap exactly 0
        print(f"{name}: {len(M)} rows, worst |err| / (8 u |M|_F) = {float(ratio.max()):.4f} at gap / |M|_F = {float((want / fro)[ratio.argmax()]):.3e}, flagged {len(sel)}")
        assert bool(torch.isfinite(gap).all()) and float(ratio.max()) <= 1.0, (name, int(ratio.argmax()))
        if name == "degenerate":
            # rows 0..15 are rank 2 with det = 0 and s2 > 0: gap = s2, well conditioned, not flagged; rank 1, zero and the signed
            # permutations of determinant -1 have gap 0 and are flagged at a positive threshold
            assert sel == list(range(16, len(M))), sel


@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 600])
def test_list_is_the_ascending_nonzero_of_the_devices_own_gaps(n):
    cl = _classes()
    names = [k for k in cl if not k.startswith("gauss_1e") or k == "gauss_1e-20"]       # scales that would all fall on one side are left out
    rows = [cl[k][r] for r in range(64) for k in names if r < len(cl[k])]               # dealt out row by row: the classes share waves
    M = torch.stack((rows * (n // len(rows) + 1))[:n])
    gap0, _, _ = _select(M, 0.0)
    finite = gap0[torch.isfinite(gap0)]
    median = float(finite.sort().values[len(finite) // 2]) if len(finite) else 0.5
    counts = {}
    for gap_min in (median, 0.0, 1e9):
        gap, sel, rest = _select(M, gap_min)
        assert torch.equal(gap.view(torch.int32), gap0.view(torch.int32)), "the gaps depend on the threshold"
        assert sel == _flagged(gap, gap_min), (n, gap_min, len(sel))
        assert sel == sorted(sel) and len(set(sel)) == len(sel)
        assert bool((rest == -1).all()), "entries behind the list were written"
        gap2, sel2, _ = _select(M, gap_min)
        assert sel2 == sel and torch.equal(gap2.view(torch.int32), gap.view(torch.int32)), "two runs differ"
        counts[gap_min] = len(sel)
    nan = int(torch.isnan(gap0).sum())
    print(f"n = {n}: median gap {median:.3g}, flagged {counts[median]} / {counts[0.0]} / {counts[1e9]} at gap_min = median / 0 / 1e9 ({nan} NaN rows)")
    assert counts[1e9] == n and counts[0.0] >= nan
    if n >= 64:
        assert 0.25 * n < counts[median] < 0.75 * n, "the median threshold should mix flagged and unflagged rows"


def test_guarded_forward_of_300_crops_repairs_in_chunks(state_dict):
    from flope_amd.engine import GuardedPoseEngine, PoseEngine, input_format
    B, H, W = 300, 96, 80
    base = torch.rand(8, 3, H, W, generator=torch.Generator().manual_seed(5))
    x = (base[torch.arange(B) % 8] * (0.5 + 0.5 * torch.rand(B, 1, 1, 1, generator=torch.Generator().manual_seed(6)))).contiguous().cuda()
    xyz = torch.rand(B, 3, generator=torch.Generator().manual_seed(2)).cuda()
    fmt = input_format(x)

    def poses(e, x, xyz, **kw):
        n = x.shape[0]
        r9, R, Rt = (torch.zeros(n, c, device="cuda") for c in (9, 9, 16))
        if kw:
            e.forward_poses_into(x, fmt, xyz, True, Rt, R, r9)
        else:                                                     # (PoseEngine.forward_poses_into has no r9 argument)
            e.forward_into(x, fmt, r9, None)
            e.forward_poses_into(x, fmt, xyz, True, Rt, R)
        torch.cuda.synchronize()
        return r9.cpu(), R.cpu(), Rt.cpu()

    g = GuardedPoseEngine(H, W, B, max_repair=32)
    g.load_state_dict(state_dict)
    g.gap_min = 0.0
    poses(g, x, xyz, guard=True)
    gap0 = g.last_gap.cpu()
    assert g.last_repaired == 0 and bool(torch.isfinite(gap0).all())
    g.gap_min = float(gap0.sort().values[B // 2])
    got = poses(g, x, xyz, guard=True)
    sel = g.read_selection()
    flagged = torch.zeros(B, dtype=torch.bool)
    flagged[sel] = True
    assert sel == _flagged(g.last_gap.cpu(), g.gap_min) and g.last_repaired == len(sel)
    assert 64 < len(sel) < B - 64, f"{len(sel)} crops flagged: the threshold should split the batch (several repair chunks of 32)"
    g.close()
    plain = PoseEngine(H, W, B, "f16")
    plain.load_state_dict(state_dict)
    fast = poses(plain, x, xyz)
    plain.close()
    exact_e = PoseEngine(H, W, len(sel), "f32m")
    exact_e.load_state_dict(state_dict)
    exact = poses(exact_e, x[flagged.cuda()].contiguous(), xyz[flagged.cuda()].contiguous())
    exact_e.close()
    print(f"B = {B}: {len(sel)} crops repaired in {(len(sel) + 31) // 32} chunks of <= 32")
    for name, a, f, e in zip(("r9", "R", "Rt"), got, fast, exact):
        assert torch.equal(a[~flagged], f[~flagged]), f"{name}: an unflagged row differs from the plain f16 engine's"
        assert torch.equal(a[flagged], e), f"{name}: a flagged row differs from the f32m engine's forward of those crops alone"
        assert not torch.equal(f[flagged], e), name                # (the comparison above could tell the two apart)
