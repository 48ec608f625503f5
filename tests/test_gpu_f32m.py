"""The float32 trunk on the exact-fp32 matrix instruction (engine option f32mfma = 1, PoseEngine dtype "f32m").

Tolerances are the project's own: the strict mode's whole-stage figures (tests/test_gpu_parity.py: stage |err| <= 2e-4 max|ref|,
|dr9| < 2e-4, |dR| < 1e-4), the element-wise bound and the order-free statistic of oracle/conv_bound.py (u = 2^-24), the
end-to-end tolerances of test_fast_pose_predictor_end_to_end_vs_oracle and the amplification law of
test_rotation_error_vs_conditioning_of_M.  The helpers of tests/test_gpu_conv_elementwise.py and tests/test_gpu_parity.py are
imported, not copied.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv_bound as CB
from oracle import pipeline_ref as P
from oracle import posenet_ref as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_conv_elementwise as E  # noqa: E402
import test_gpu_parity as G  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_STAGES = G.STAGES + [f"layer{li}.{bi}.mid" for li in range(1, 5) for bi in range(2)] + [f"layer{li}.0.ds" for li in (2, 3, 4)]


def _engine(sd, H, W, B, dtype="f32m", **opts):
    return G._engine(sd, H, W, B, dtype, **opts)


def _conv_labels(e, B):
    """kernel labels of the stem and the 19 trunk convs of the last forward"""
    info = e.launch_info(B)
    return [k for layer, k, _ in info if layer == "stem" or layer.startswith("base.layer")]


# ---- 4. every stage against the fp32 oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B,streams", [(224, 224, 4, None), (96, 80, 3, None), (65, 71, 2, None), (512, 512, 2, None), (96, 80, 37, 2)])
def test_every_stage_against_the_fp32_oracle(state_dict, H, W, B, streams):
    torch.manual_seed(10)
    x = torch.rand(B, 3, H, W)
    ref = O.forward_stages(state_dict, x)
    e = _engine(state_dict, H, W, B, **({} if streams is None else {"streams": streams}))
    r9, R = G._run(e, x)
    labels = _conv_labels(e, B)
    assert len(labels) == 20 and all(k.startswith("conv_f32m_kernel<") for k in labels), labels
    for s in G.STAGES:
        got = e.read_stage(s, B).cpu()
        assert got.shape == ref[s].shape, s
        err, lim = float((got - ref[s]).abs().max()), 2e-4 * float(ref[s].abs().max())
        print(f"  {s:10s} |err| {err:.3e}  allowed {lim:.3e}")
        assert err <= lim, s
    print(f"  |dr9| {float((r9 - ref['r9']).abs().max()):.3e}  |dR| {float((R - O.procrustes_to_rotmat(ref['r9'])).abs().max()):.3e}")
    assert (r9 - ref["r9"]).abs().max() < 2e-4
    assert (R - O.procrustes_to_rotmat(ref["r9"])).abs().max() < 1e-4
    e.close()


# ---- 5. every conv on its own, element-wise against fp64 --------------------------------------------------------------------------------------
def _walk(sd, H, W, B, nb, **opts):
    """The walk of tests/test_gpu_conv_elementwise.py for a float32 engine with f32mfma = 1: each conv from the device's own input,
    every element within `bound`, relL2 within `statistical_bound`; -> (failures, kernel labels judged)."""
    dt, dev = torch.float32, torch.device("cuda")
    xin, xconv = E._inputs(H, W, nb, "f32", dt)
    sel = torch.arange(B) % nb
    e = _engine(sd, H, W, B, **opts)
    e.forward(xin[sel].contiguous().to(dev))
    torch.cuda.synchronize()
    info = e.launch_info(B)
    kern = {layer: k for layer, k, _ in info}
    lines, fails, judged = [f"{H}x{W}-B{B}-f32m{opts}: {e.launches()} launches"], [], []
    specs = E._specs(sd, "f32", frozenset())
    gsel = sel.to(dev)
    # front: stem on its own, the max-pool from the device's stem is exact
    stem, pool = e.read_stage("stem", B), e.read_stage("pool", B)
    assert info[0][1] == "prep_input_kernel" and info[1][0] == "stem" and info[2][1] == "maxpool_kernel", info[:3]
    ref, bound = CB.reference(specs["stem"], xconv, dt)
    emu = CB.emulate(specs["stem"], xconv, dt)
    stat = CB.statistical_bound(ref, bound, specs["stem"].K, dt).pow(2)
    E._judge(lines, fails, "stem", info[1][1], stem, ref.to(dev)[gsel], bound.to(dev)[gsel], float((emu.double() - ref)[sel].pow(2).sum()),
             float(ref[sel].pow(2).sum()), dt, nb, float(stat[sel].sum()))
    judged.append(info[1][1])
    assert torch.equal(pool, F.max_pool2d(stem, 3, 2, 1)), "maxpool_kernel differs from the max of the device's stem tensor"
    # the 16 block convs and the three shortcut convs
    taps = {"pool": pool}
    for name, xn, rn, dsn, on in CB.trunk_io(specs):
        assert dsn is None, name                       # no folded shortcut in float32
        for t in (xn, rn, on):
            if t is not None and t not in taps:
                taps[t] = e.read_stage(t, B)
        ins = [taps[t] for t in (xn, rn) if t is not None]
        reps, gid = E._groups(ins)
        refs, bounds, e2, r2, s2 = [], [], 0.0, 0.0, 0.0
        counts = torch.bincount(gid, minlength=len(reps)).tolist()
        for g, r in enumerate(reps):
            rf, bd, ee, rr, ss = E._reference(specs[name], "f32", [t[r:r + 1].cpu() for t in ins], rn is not None, False, dev)
            refs.append(rf)
            bounds.append(bd)
            e2 += ee * counts[g]
            r2 += rr * counts[g]
            s2 += ss * counts[g]
        k = kern["base." + name.replace(".ds", ".downsample.0")]
        E._judge(lines, fails, name, k, taps[on], torch.stack(refs)[gid], torch.stack(bounds)[gid], e2, r2, dt, len(reps), s2)
        judged.append(k)
    e.close()
    print("\n".join(lines))
    return fails, judged


@pytest.mark.parametrize("H,W,B,nb,opts", [(224, 224, 4, 4, {}), (65, 71, 2, 2, {}), (224, 224, 70, 4, {"streams": 2}), (512, 512, 2, 2, {})],
                         ids=["224x224-B4", "65x71-B2", "224x224-B70-streams2", "512x512-B2"])
def test_every_conv_elementwise_within_the_derived_bound(state_dict, H, W, B, nb, opts):
    fails, judged = _walk(state_dict, H, W, B, nb, **opts)
    assert len(judged) == 20 and all(k.startswith("conv_f32m_kernel<") for k in judged), judged
    assert not fails, "\n".join(fails)


# ---- 6. the ring and the checker survive ---------------------------------------------------------------------------------------------------------
def _all_stages(e, B):
    return {s: e.read_stage(s, B).clone() for s in ALL_STAGES}


def test_option_flips_between_forwards_leave_nothing_behind(state_dict):
    H, W, B = 96, 80, 3
    torch.manual_seed(3)
    x = torch.rand(B, 3, H, W)
    e = _engine(state_dict, H, W, B, "f32")
    assert e.set_option("f32mfma", 1) == 0
    r1 = G._run(e, x)
    s1 = _all_stages(e, B)
    assert all(k.startswith("conv_f32m_kernel<") for k in _conv_labels(e, B))
    assert e.set_option("f32mfma", 0) == 1
    r0 = G._run(e, x)
    s0 = _all_stages(e, B)
    assert all(k == "naive_conv_kernel" for k in _conv_labels(e, B))
    fresh = _engine(state_dict, H, W, B, "f32")
    rf = G._run(fresh, x)
    sf = _all_stages(fresh, B)
    assert all(k == "naive_conv_kernel" for k in _conv_labels(fresh, B))
    for s in ALL_STAGES:
        assert torch.equal(s0[s], sf[s]), f"{s}: the strict mode after an f32mfma forward differs from a fresh strict engine"
    assert torch.equal(r0[0], rf[0]) and torch.equal(r0[1], rf[1])
    e.set_option("f32mfma", 1)
    r2 = G._run(e, x)
    s2 = _all_stages(e, B)
    for s in ALL_STAGES:
        assert torch.equal(s1[s], s2[s]), f"{s}: two f32mfma forwards of one input differ"
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
    # (the zero ring of every padded buffer is read by the strict checker's 3x3 convs, so the equality above holds it too);
    # the two modes differ in summation order only
    assert (r1[0] - r0[0]).abs().max() < 2e-4
    fresh.close()
    e.close()


# ---- 7. batch independence -------------------------------------------------------------------------------------------------------------------------
def test_a_crop_gives_the_same_bits_wherever_it_stands(state_dict):
    B = 5
    torch.manual_seed(4)
    x = torch.rand(B, 3, 224, 224)
    e = _engine(state_dict, 224, 224, B, streams=1)
    base, _ = G._run(e, x)
    perm = torch.tensor([3, 0, 4, 1, 2])
    got, _ = G._run(e, x[perm].contiguous())
    assert torch.equal(got, base[perm])
    # other neighbours, another batch size: the tiling moves, the order of every sum does not
    y = torch.rand(B, 3, 224, 224)
    y[2] = x[0]
    got, _ = G._run(e, y)
    assert torch.equal(got[2], base[0])
    got, _ = G._run(e, x[:2].contiguous())
    assert torch.equal(got, base[:2])
    e.close()


# ---- 8. public interface ---------------------------------------------------------------------------------------------------------------------------
def test_posenet_module_in_f32m(state_dict, golden_cfg1):
    from sunflower.models.posenet import PoseResNet
    from sunflower.utils.conversion import procrustes_to_rotmat
    torch.manual_seed(0)
    x = torch.rand(16, 3, 224, 224).cuda()
    net = PoseResNet(compute_dtype="f32m", max_batch=16).to("cuda")
    net.load_state_dict(state_dict)
    r9 = net(x)
    R = procrustes_to_rotmat(r9).cpu()
    Rg = torch.from_numpy(golden_cfg1["R"])
    print(f"cfg1 f32m: |R - golden|max = {float((R - Rg).abs().max()):.3e}")
    assert (R - Rg).abs().max() <= 1e-4
    assert net.extract_features(x).shape == (16, 2048)
    e = net.engine_for("cuda", (224, 224), 16)
    info = e.launch_info(16)
    assert info[1][0] == "stem" and info[1][1].startswith("conv_f32m_kernel<")
    assert sum(k.startswith("conv_f32m_kernel<") for _, k, _ in info) == 20 and not any(k == "naive_conv_kernel" for _, k, _ in info)


def test_option_is_a_no_op_on_a_16_bit_engine(state_dict):
    torch.manual_seed(1)
    x = torch.rand(3, 3, 96, 80)
    e = _engine(state_dict, 96, 80, 3, "f16")
    before = G._run(e, x)
    info = e.launch_info(3)
    plan = e.describe_plan()
    assert e.set_option("f32mfma", 1) == 0 and e.set_option("f32mfma", 5) == 1 and e.set_option("f32mfma", 1) == 1
    after = G._run(e, x)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert e.launch_info(3) == info and e.describe_plan() == plan
    e.close()


def test_fast_pose_predictor_frame_with_an_f32m_posenet(state_dict, tmp_path, monkeypatch):
    """One 480 x 640 frame, detections given, as test_fast_pose_predictor_end_to_end_vs_oracle sets it up; FLOPE_DTYPE selects the
    network's mode, and the predictor's input-format lookup falls through to float32 NCHW crops."""
    import yaml
    from sunflower.predictor.fast_pose_predictor import FastPosePredictor
    monkeypatch.setenv("FLOPE_DTYPE", "f32m")
    rgb, mask, depth, boxes = G._scene(22)
    ckpt, intr = tmp_path / "posenet.pth", tmp_path / "intrinsics.yaml"
    torch.save(state_dict, ckpt)
    intr.write_text(yaml.safe_dump(dict(fx=600.0, fy=600.0, cx=320.0, cy=240.0, h=480, w=640)))
    pred = FastPosePredictor("cuda", lambda img: (boxes, mask), str(ckpt), str(intr))
    assert pred.posenet.compute_dtype == "f32m"
    Rt = pred.get_flower_poses(rgb, depth)
    K = np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]])
    ref = P.get_flower_poses(lambda b: O.forward(state_dict, b), O.procrustes_to_rotmat, rgb, depth, boxes, mask, K)
    assert Rt.dtype == np.float64 and Rt.shape == ref.shape and Rt.shape[0] >= 3
    print(f"f32m frame: rot err {np.abs(Rt[:, :3, :3] - ref[:, :3, :3]).max():.3e}")
    assert np.abs(Rt[:, :3, :3] - ref[:, :3, :3]).max() <= 1e-3                 # rot err
    assert np.linalg.norm(Rt[:, :3, 3] - ref[:, :3, 3], axis=1).max() <= 1e-5   # trans err (m)
    np.testing.assert_array_equal(Rt[:, 3], np.tile([0, 0, 0, 1.0], (Rt.shape[0], 1)))
    e = pred.posenet.engine_for("cuda", (512, 512))
    assert sum(k.startswith("conv_f32m_kernel<") for _, k, _ in e.launch_info(1)) == 20


# ---- 9. the reason the mode exists -------------------------------------------------------------------------------------------------------------------
def test_rotation_error_vs_conditioning_of_M_in_f32m(state_dict):
    """The sweep of tests/test_gpu_parity.py::test_rotation_error_vs_conditioning_of_M (re-biased head, M_i = a R0 + (W h_i - mean W h),
    (s2 + s3) from ~2 down to ~0.01) with the float32 MFMA trunk: the amplification law |dR| (s2 + s3) <= 3 |dM| at every point.
    The measured table is printed (pytest -s) and quoted in DESIGN.md beside f16's."""
    torch.manual_seed(0)
    x = torch.rand(16, 3, 224, 224)
    rows = []
    e = _engine(state_dict, 224, 224, 16)
    sd0 = dict(state_dict)
    sd0["fc_rot.bias"] = torch.zeros(9)
    mean_wh = O.forward(sd0, x).mean(0)
    for a in (1.0, 0.3, 0.1, 0.03, 0.01):
        sd = dict(state_dict)
        sd["fc_rot.bias"] = state_dict["fc_rot.bias"] * a - mean_wh
        e.load_state_dict(sd)
        r9, R = G._run(e, x)
        ref9 = O.forward(sd, x)
        Rref = O.procrustes_to_rotmat(ref9)
        sv = torch.linalg.svdvals(ref9.double().view(-1, 3, 3))
        gap = (sv[:, 1] + sv[:, 2])
        dR = (R - Rref).abs().amax(dim=(1, 2)).double()
        dM = (r9 - ref9).abs().amax(dim=1).double()
        rows.append((a, float(gap.min()), float(gap.median()), float(dM.max()), float(dR.max()), float((dR * gap).max())))
    assert all(k.startswith("conv_f32m_kernel<") for k in _conv_labels(e, 16))
    e.close()
    print("\nf32m: bias scale a | min(s2+s3) | median | max|dM| | max|dR| | max |dR|*(s2+s3)")
    for r in rows:
        print("   %.2f | %.4f | %.4f | %.2e | %.2e | %.2e" % r)
    assert rows[0][1] > 1.5 and rows[-1][1] < 0.05               # the sweep really spans two decades of conditioning
    for a, gmin, gmed, dM, dR, k in rows:
        assert k <= 3.0 * dM + 1e-6, (a, k, dM)
