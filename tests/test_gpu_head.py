"""The head behind layer4.1 (flope_amd/csrc/pool_head.hip) at every kernel variant plan.h: head_plan can choose, judged from the
device's own taps, so the trunk is not under test here.

One engine per case on small crops.  From the tensor the DEVICE fed each step (read_stage("layer4.1" | "feat" | "hidden")):

    feat, hidden, r9   element by element against fp64 within oracle/conv_bound.py's avgpool_reference / linear_reference, with both
                       assertions of tests/test_gpu_conv_elementwise.py (its _judge)
    R                  against R_ref of the device's own r9 (float64 SVD: the weights below keep gap(r9) above 0.1) within the
                       Procrustes bound of tests/pose_bound.py, 2^-24 |R_ref| + C 2^-53 |M|_F / gap, plus 64 2^-53 |M|_F / gap for
                       the float64 SVD's own backward error; and as a rotation within pose_bound's ORTH_BOUND / DET_BOUND
    Rt                 [:3, :3] is R in bits with nullify = 0; with nullify = 1 column 2 is R's in bits, and columns 0, 1 lie within
                       2^-24 |O_ref| + 12 2^-53 (|a| + |b|) + 2^-150 of O_ref = R Rz(a)^T, a = atan2(-R01, R00), of the device's own R
                       (pose_bound's yaw bound with the constant of the float64 reference used here, see K_YAW).  [:3, 3] is xyz
                       in bits (zeros for None), the last row exactly 0 0 0 1; all four pairs of nullify and xyz / None run.
    tails              r9, R and Rt are written into tensors with three rows more than the batch, filled with a sentinel:
                       those rows stay untouched.
    determinism        a second run of each entry point gives equal bits.

Weights for a width bod: the fixture's state dict with base.fc.0.* and fc_rot.* rebuilt by a seeded generator; fc_rot.bias is
2 I, and fc_rot.weight small against it, so that gap(r9) stays above 0.1 (asserted from the device's r9 by a float64 SVD).

Every case asserts which variant it ran through PoseEngine.head_plan() (flope_head_plan: the rule the launchers themselves
use); the last test asserts that every variant was judged.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pose_bound as PB
import pose_cases as PC
from oracle import conv_bound as CB

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_YAW = PB.K_YAW - 1 + 7      # the kernel's 5 (pose_bound.py) and 7 for the float64 reference here: atan2 1, cos / sin of |a| <= pi 4.2, two products and a sum 2
SENTINEL = -7.25e11
TAIL = 3


def _c(bod, B, fc1, fc2, dtype="f16", H=96, W=80, **opts):
    return (bod, B, dtype, H, W, tuple(sorted(opts.items())), fc1, fc2)


CASES = [
    # defaults, and each option at the default width
    _c(2048, 1, "packed", "k4"), _c(2048, 17, "row-major", "k4", fc1_packed=0), _c(2048, 5, "packed", "wave-vector", fc2_k4=0),
    _c(2048, 33, "packed", "k4", "bf16"), _c(2048, 5, "packed", "k4", "f32"), _c(2048, 16, "packed", "k4", "f32m"),
    # k4 with one trip, and with three trips under `unroll 2`
    _c(1024, 16, "packed", "k4"), _c(1024, 5, "packed", "wave-vector", fc2_k4=0), _c(3072, 1, "packed", "k4"), _c(3072, 17, "packed", "k4"),
    # 17 fc.0 tiles: one live wave in the last workgroup; fc_rot vector loop with a 4-lane second step
    _c(272, 33, "packed", "wave-vector"), _c(272, 5, "row-major", "wave-vector", fc1_packed=0),
    # 3 tiles; 12 live lanes
    _c(48, 16, "packed", "wave-vector"), _c(48, 33, "row-major", "wave-vector", fc1_packed=0),
    # fc1_simple_kernel; a partly filled fourth step of the vector loop
    _c(1000, 17, "simple", "wave-vector"), _c(1000, 1, "simple", "wave-vector", "bf16"), _c(1000, 5, "simple", "wave-vector", "f32"),
    _c(1000, 33, "simple", "wave-vector", "f32m"),
    # scalar fc_rot loop; minimal width
    _c(30, 1, "simple", "wave-scalar"), _c(30, 16, "simple", "wave-scalar"), _c(1, 5, "simple", "wave-scalar"), _c(1, 17, "simple", "wave-scalar"),
    # avgpool: 64 pixels (the last of the register path), 70 pixels (the first of the strided path, ragged groups of 4), float32
    _c(2048, 5, "packed", "k4", "f16", 256, 256), _c(2048, 5, "packed", "k4", "bf16", 256, 256),
    _c(2048, 5, "packed", "k4", "f16", 224, 320), _c(2048, 5, "packed", "k4", "bf16", 224, 320), _c(2048, 2, "packed", "k4", "f32", 224, 320),
]

FC1_VARIANTS, FC2_VARIANTS = ("packed", "row-major", "simple"), ("k4", "wave-vector", "wave-scalar")
POOL_VARIANTS = ("avgpool_kernel<=64px", "avgpool_kernel>64px", "avgpool_f32_kernel")
_DONE = {}


def _case_id(c):
    bod, B, dtype, H, W, opts, fc1, fc2 = c
    return f"bod{bod}-B{B}-{dtype}-{H}x{W}" + "".join(f"-{k}{v}" for k, v in opts)


@functools.lru_cache(maxsize=None)
def _head_weights(bod):
    g = torch.Generator().manual_seed(1000 + bod)
    return {"base.fc.0.weight": torch.randn(bod, 512, generator=g) / 512 ** 0.5, "base.fc.0.bias": 0.1 * torch.randn(bod, generator=g),
            "fc_rot.weight": 0.05 * torch.randn(9, bod, generator=g) / bod ** 0.5, "fc_rot.bias": (2.0 * torch.eye(3)).reshape(9) + 0.05 * torch.randn(9, generator=g)}


@functools.lru_cache(maxsize=None)
def _crops(H, W):
    return torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(12))


def _yaw_f64(R):
    """R Rz(a)^T with a = atan2(-R01, R00) in float64 -- the statement of mvg.py, not the kernel's c0 / n form -- on float32 R
    [B, 3, 3] -> O_ref [B, 3, 3], |a| + |b| [B, 3]"""
    R = R.double()
    a = torch.atan2(-R[:, 0, 1], R[:, 0, 0])
    Rz = torch.zeros_like(R)
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = torch.cos(a), -torch.sin(a), torch.sin(a), torch.cos(a), 1.0
    return R @ Rz.transpose(1, 2), R[:, :, 0].abs() + R[:, :, 1].abs()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _walk(sd, case):
    import test_gpu_conv_elementwise as EW
    from flope_amd.engine import PoseEngine, input_format
    bod, B, dtype, H, W, opts, want_fc1, want_fc2 = case
    dev = torch.device("cuda")
    hw = _head_weights(bod)
    sdb = {**sd, **hw}
    e = PoseEngine(H, W, B, dtype, backbone_out_dim=bod)
    for k, v in opts:
        e.set_option(k, v)
    e.load_state_dict(sdb)
    assert e.head_plan() == (want_fc1, want_fc2), (e.head_plan(), case)
    x = _crops(H, W)[torch.arange(B) % 4].contiguous().to(dev)
    fmt = input_format(x)
    xyz = torch.randn(B, 3, generator=torch.Generator().manual_seed(B)).to(dev)
    lines, fails = [f"{_case_id(case)}: fc.0 {want_fc1}, fc_rot {want_fc2}"], []

    def big(cols):
        return torch.full((B + TAIL, cols), SENTINEL, dtype=torch.float32, device=dev)

    # ---- A: r9 and R; the taps of this run ----
    r9, R = big(9), big(9)
    e.forward_into(x, fmt, r9, R)
    torch.cuda.synchronize()
    last, feat, hidden = e.read_stage("layer4.1", B).cpu(), e.read_stage("feat", B).cpu(), e.read_stage("hidden", B).cpu()
    r9c, Rc = r9.cpu(), R.cpu()
    assert bool((r9c[B:] == SENTINEL).all()) and bool((Rc[B:] == SENTINEL).all()), "a row behind the batch was written (r9 / R)"
    r9b, Rb = r9c[:B], Rc[:B].view(B, 3, 3)
    npx = last.shape[2] * last.shape[3]
    pool_variant = "avgpool_f32_kernel" if dtype in ("f32", "f32m") else ("avgpool_kernel<=64px" if npx <= 64 else "avgpool_kernel>64px")
    assert hidden.shape == (B, bod) and feat.shape == (B, 512)
    f32 = torch.float32
    ref, bound = CB.avgpool_reference(last)
    EW._judge(lines, fails, "feat", pool_variant, feat, ref, bound, float((last.mean(dim=(2, 3)).double() - ref).pow(2).sum()), float(ref.pow(2).sum()), f32, B,
              float(CB.statistical_bound(ref, bound, npx, f32).pow(2).sum()))
    ref, bound = CB.linear_reference(feat, hw["base.fc.0.weight"], hw["base.fc.0.bias"], True)
    emu = F.relu(F.linear(feat, hw["base.fc.0.weight"], hw["base.fc.0.bias"]))
    EW._judge(lines, fails, "hidden", "fc.0 " + want_fc1, hidden, ref, bound, float((emu.double() - ref).pow(2).sum()), float(ref.pow(2).sum()), f32, B,
              float(CB.statistical_bound(ref, bound, 512, f32).pow(2).sum()))
    ref, bound = CB.linear_reference(hidden, hw["fc_rot.weight"], hw["fc_rot.bias"], False)
    emu = F.linear(hidden, hw["fc_rot.weight"], hw["fc_rot.bias"])
    EW._judge(lines, fails, "r9", "fc_rot " + want_fc2, r9b, ref, bound, float((emu.double() - ref).pow(2).sum()), float(ref.pow(2).sum()), f32, B,
              float(CB.statistical_bound(ref, bound, bod, f32).pow(2).sum()))

    # ---- R: the special Procrustes rotation of the device's own r9 ----
    M9 = r9b.numpy().reshape(B, 3, 3)
    Rref, gap, fro, _ = PC.procrustes_reference(M9, "f64")
    assert float(gap.min()) > 0.1, f"the test's weights give gap(r9) = {float(gap.min()):.3g}"
    pbound = PB.procrustes_bound(Rref, gap, fro, PB.newton_ab(M9, gap, fro)) + (64 * PB.U64 * fro / gap)[:, None, None]
    perr = float((np.abs(Rb.numpy().astype(np.float64) - Rref) / pbound).max())
    o, d = PB.rotation_defect(Rb.numpy())
    lines.append(f"  R: min gap(r9) {float(gap.min()):.3f}  err / bound {perr:.3f}  |R R^T - I| / bound {o.max():.3f}  |det R - 1| / bound {d.max():.3f}")
    if not (perr <= 1 and o.max() <= 1 and d.max() <= 1):
        fails.append(f"R of the device's own r9: err / bound {perr:.3f}, rotation defect {max(o.max(), d.max()):.3f}")

    # ---- B: poses with xyz and the yaw-null; C: without either ----
    Rt1, R1 = big(16), big(9)
    e.forward_poses_into(x, fmt, xyz, True, Rt1, R1)
    Rt0, Rtx, Rtn = big(16), big(16), big(16)
    e.forward_poses_into(x, fmt, None, False, Rt0)
    e.forward_poses_into(x, fmt, xyz, False, Rtx)                 # the crossed pairs
    e.forward_poses_into(x, fmt, None, True, Rtn)
    torch.cuda.synchronize()
    Rt1c, R1c, Rt0c = Rt1.cpu(), R1.cpu(), Rt0.cpu()
    assert bool((Rt1c[B:] == SENTINEL).all()) and bool((R1c[B:] == SENTINEL).all()) and bool((Rt0c[B:] == SENTINEL).all()), "a row behind the batch was written (Rt / R)"
    assert torch.equal(_bits(R1c), _bits(Rc)), "R of forward_poses differs in bits from R of forward"
    P1, P0 = Rt1c[:B].view(B, 4, 4), Rt0c[:B].view(B, 4, 4)
    last_row = torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 4)
    assert torch.equal(_bits(P1[:, 3]), _bits(last_row)) and torch.equal(_bits(P0[:, 3]), _bits(last_row)), "last row of Rt"
    assert torch.equal(_bits(P1[:, :3, 3]), _bits(xyz.cpu())) and torch.equal(_bits(P0[:, :3, 3]), _bits(torch.zeros(B, 3))), "translation column of Rt"
    assert torch.equal(_bits(P0[:, :3, :3]), _bits(Rb)), "Rt[:3, :3] with nullify = 0 is not R in bits"
    assert torch.equal(_bits(P1[:, :3, 2]), _bits(Rb[:, :, 2])), "the yaw-null changed column 2"
    Rtxc, Rtnc = Rtx.cpu(), Rtn.cpu()
    assert bool((Rtxc[B:] == SENTINEL).all()) and bool((Rtnc[B:] == SENTINEL).all()), "a row behind the batch was written (Rt)"
    Px, Pn = Rtxc[:B].view(B, 4, 4), Rtnc[:B].view(B, 4, 4)
    assert torch.equal(_bits(Px[:, :3, :3]), _bits(Rb)) and torch.equal(_bits(Px[:, :3, 3]), _bits(xyz.cpu())) and torch.equal(_bits(Px[:, 3]), _bits(last_row)), "xyz with nullify = 0"
    assert torch.equal(_bits(Pn[:, :3, :3]), _bits(P1[:, :3, :3])) and torch.equal(_bits(Pn[:, :3, 3]), _bits(torch.zeros(B, 3))) and torch.equal(_bits(Pn[:, 3]), _bits(last_row)), "no xyz with nullify = 1"
    Oref, ab = _yaw_f64(Rb)
    ybound = U * Oref[:, :, :2].abs() + K_YAW * 2.0 ** -53 * ab[:, :, None] + 2.0 ** -150
    yerr = (P1[:, :3, :2].double() - Oref[:, :, :2]).abs()
    lines.append(f"  Rt: yaw-null worst err / bound {float((yerr / ybound).max()):.3f}, |O01| max {float(P1[:, 0, 1].abs().max()):.2e}")
    if not bool((yerr <= ybound).all()):
        fails.append(f"yaw-null of the device's own R: err / bound = {float((yerr / ybound).max()):.3f}")

    # ---- determinism ----
    r9_2, R_2, Rt1_2 = big(9), big(9), big(16)
    e.forward_into(x, fmt, r9_2, R_2)
    e.forward_poses_into(x, fmt, xyz, True, Rt1_2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(r9_2.cpu()), _bits(r9c)) and torch.equal(_bits(R_2.cpu()), _bits(Rc)) and torch.equal(_bits(Rt1_2.cpu()), _bits(Rt1c)), "two runs differ in bits"
    e.close()
    print("\n".join(lines))
    _DONE[case] = (want_fc1, want_fc2, pool_variant)
    return fails


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_head_from_the_devices_own_taps(state_dict, case):
    fails = _walk(state_dict, case)
    assert not fails, "\n".join(fails)


def _variants(case):
    bod, B, dtype, H, W, opts, fc1, fc2 = case
    npx = -(-H // 32) * -(-W // 32)
    return ("fc.0 " + fc1, "fc_rot " + fc2, "avgpool_f32_kernel" if dtype in ("f32", "f32m") else ("avgpool_kernel<=64px" if npx <= 64 else "avgpool_kernel>64px"))


def test_every_head_variant_was_judged(state_dict):
    """Runs last.  Under a -k selection only as many further cases are walked as it takes to reach every variant (nine at most), so
    the assertion stands alone without running the table again."""
    want = ["fc.0 " + v for v in FC1_VARIANTS] + ["fc_rot " + v for v in FC2_VARIANTS] + list(POOL_VARIANTS)
    seen = {}
    for case in list(_DONE) + [c for c in CASES if c not in _DONE]:
        if case not in _DONE:
            if all(seen.get(v) for v in _variants(case)):
                continue
            assert not _walk(state_dict, case)
        fc1, fc2, pool = _DONE[case]
        assert ("fc.0 " + fc1, "fc_rot " + fc2, pool) == _variants(case), case
        for v in _variants(case):
            seen[v] = seen.get(v, 0) + 1
    print("head variants judged (cases):", {v: seen.get(v, 0) for v in want})
    missing = [v for v in want if not seen.get(v)]
    assert not missing, f"head variants no case reached: {missing}"
