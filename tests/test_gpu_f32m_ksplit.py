"""Split-K of the float32 MFMA trunk on the device (engine option f32m_ksplit, PoseEngine dtype "f32mk", GuardedPoseEngine
exact_dtype "f32mk", compute_dtype "guardk"; conv_f32m.hip).

Shapes: 65x71 (layer 4 is a 3x3 map: 9 pixels per crop, one ragged 16-pixel tile, 288 steps), 96x80, and 224^2 at B = 1, the shape
the feature exists for.  Tolerances are tests/test_gpu_f32m.py's own (stage 2e-4 max|ref|, |dr9| < 2e-4, |dR| < 1e-4; the
element-wise bound and the order-free statistic of oracle/conv_bound.py, u = 2^-24 -- both hold for any summation order, so they
are the same at every share count).  Every test that claims to exercise the split asserts that launch_info shows a "[split-K x"
entry.  The helpers of tests/test_gpu_f32m.py, test_gpu_parity.py, test_gpu_conv_elementwise.py and test_gpu_guard.py are
imported, not copied.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import conv_bound as CB
from oracle import posenet_ref as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_f32m_ksplit_host as HK  # noqa: E402
import test_gpu_f32m as M  # noqa: E402
import test_gpu_guard as GD  # noqa: E402
import test_gpu_parity as G  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = torch.float32
both_kinds = GD.both_kinds                                  # the fixture of tests/test_gpu_guard.py: eight well-, eight ill-conditioned crops


def _split_layers(e, B):
    """{layer: S} of the trunk convs the last forward ran as split launches"""
    out = {}
    for layer, k, _ in e.launch_info(B):
        if "[split-K x" in layer:
            assert k.startswith("conv_f32m_kernel<"), (layer, k)
            out[layer.split("[")[0]] = int(layer.split("[split-K x")[1].rstrip("]"))
    return out


# ---- 1. every stage against the fp32 oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H_,W,B,v", [(65, 71, 1, 1), (96, 80, 3, 1), (224, 224, 1, 1), (224, 224, 4, 1), (65, 71, 2, 32)])
def test_every_stage_against_the_fp32_oracle(state_dict, H_, W, B, v):
    torch.manual_seed(10)
    x = torch.rand(B, 3, H_, W)
    ref = O.forward_stages(state_dict, x)
    e = M._engine(state_dict, H_, W, B, f32m_ksplit=v)
    r9, R = G._run(e, x)
    labels = M._conv_labels(e, B)
    assert len(labels) == 20 and all(k.startswith("conv_f32m_kernel<") for k in labels), labels
    split = _split_layers(e, B)
    print(f"  split: {split}")
    assert split, "no launch of this forward was split"
    assert e.launches() == 3 + 19 + 3                                      # a split conv counts once
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


# ---- 2. every conv on its own, element-wise against fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H_,W,B,nb,v", [(65, 71, 2, 2, 2), (65, 71, 2, 2, 8), (65, 71, 2, 2, 32), (65, 71, 2, 2, 1), (96, 80, 3, 3, 4), (224, 224, 1, 1, 1)])
def test_every_conv_elementwise_within_the_derived_bound(state_dict, monkeypatch, H_, W, B, nb, v):
    """tests/test_gpu_f32m.py::_walk with the option forwarded.  That walk looks a conv's kernel up by its bare layer name, and a
    split launch is listed as "layer[split-K xS]": the engine it builds here answers launch_info with the bracket taken off (and
    remembers the full names, which is how the test knows a split ran)."""
    seen = []

    def engine(sd, h, w, b, dtype="f32m", **opts):
        e = G._engine(sd, h, w, b, dtype, **opts)
        full = e.launch_info

        def bare(batch):
            info = full(batch)
            seen.extend(layer for layer, _, _ in info)
            return [(layer.split("[")[0], k, f) for layer, k, f in info]
        e.launch_info = bare
        return e

    monkeypatch.setattr(M, "_engine", engine)
    fails, judged = M._walk(state_dict, H_, W, B, nb, f32m_ksplit=v)
    assert any("[split-K x" in layer for layer in seen), seen
    assert len(judged) == 20 and all(k.startswith("conv_f32m_kernel<") for k in judged), judged
    assert not fails, "\n".join(fails)


# ---- 3. bits --------------------------------------------------------------------------------------------------------------------------------
def test_bits_depend_on_the_batch_size_only(state_dict):
    B = 5
    torch.manual_seed(4)
    x = torch.rand(B, 3, 224, 224)
    e = M._engine(state_dict, 224, 224, B, streams=1, f32m_ksplit=1)
    base, R0 = G._run(e, x)
    assert _split_layers(e, B)
    again, R1 = G._run(e, x)
    assert torch.equal(base, again) and torch.equal(R0, R1)                # two forwards of one input
    perm = torch.tensor([3, 0, 4, 1, 2])
    got, _ = G._run(e, x[perm].contiguous())
    assert torch.equal(got, base[perm])                                    # position
    y = torch.rand(B, 3, 224, 224)
    y[2] = x[0]
    got, _ = G._run(e, y)
    assert torch.equal(got[2], base[0])                                    # neighbours, at the same batch size
    e.close()


def _stages_equal(a, b, B, stages):
    return [s for s in stages if not torch.equal(a.read_stage(s, B), b.read_stage(s, B))]


def test_where_nothing_splits_every_bit_is_option_zeros(state_dict):
    """B = 64 x 224^2 runs in two slices: no launch may split, and r9 / R and every stage equal option 0's."""
    H_, W, B = 224, 224, 64
    torch.manual_seed(12)
    x = torch.rand(B, 3, H_, W)
    on, off = M._engine(state_dict, H_, W, B, f32m_ksplit=1), M._engine(state_dict, H_, W, B)
    a, b = G._run(on, x), G._run(off, x)
    assert not _split_layers(on, B) and on.launch_info(B) == off.launch_info(B)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert _stages_equal(on, off, B, M.ALL_STAGES) == []
    on.close()
    off.close()


def test_unsplit_launches_of_a_partly_split_forward_keep_their_bits(state_dict):
    """B = 37 x 96x80 with streams = 2 is ONE slice (37 / 2 < 32 crops per slice), and layers 3 and 4 are 72 and 48 workgroups there:
    the cost model splits them (so r9 is not option 0's -- another summation order), while layers 1 and 2 (139 and 140
    workgroups: tiles x 2 > 256) must not split.  Everything in front of the first split launch equals option 0's bit for bit, and
    the launches that did not split are listed exactly as option 0 lists them."""
    H_, W, B = 96, 80, 37
    torch.manual_seed(13)
    x = torch.rand(B, 3, H_, W)
    on, off = M._engine(state_dict, H_, W, B, streams=2, f32m_ksplit=1), M._engine(state_dict, H_, W, B, streams=2)
    a, b = G._run(on, x), G._run(off, x)
    split = _split_layers(on, B)
    print(f"  split: {split}")
    assert split and not any(l.startswith(("base.layer1", "base.layer2")) for l in split), split
    assert [(l, k) for l, k, _ in on.launch_info(B) if "[" not in l] == [(l, k) for l, k, _ in off.launch_info(B) if l not in split]
    front = ["stem", "pool"] + [s for s in M.ALL_STAGES if s.startswith(("layer1", "layer2"))]
    assert _stages_equal(on, off, B, front) == []
    assert (a[0] - b[0]).abs().max() < 2e-4
    on.close()
    off.close()


# ---- 4. nothing left behind ----------------------------------------------------------------------------------------------------------------
def test_option_flips_between_forwards_leave_nothing_behind(state_dict):
    H_, W, B = 96, 80, 3
    torch.manual_seed(3)
    x = torch.rand(B, 3, H_, W)
    e = M._engine(state_dict, H_, W, B, "f32")
    assert e.set_option("f32mfma", 1) == 0 and e.set_option("f32m_ksplit", 32) == 0
    G._run(e, x)
    assert _split_layers(e, B)
    assert e.set_option("f32m_ksplit", 0) == 32
    r1 = G._run(e, x)
    s1 = M._all_stages(e, B)
    assert not _split_layers(e, B) and all(k.startswith("conv_f32m_kernel<") for k in M._conv_labels(e, B))
    assert e.set_option("f32mfma", 0) == 1
    r0 = G._run(e, x)
    s0 = M._all_stages(e, B)
    assert all(k == "naive_conv_kernel" for k in M._conv_labels(e, B))
    for dtype, r, s in (("f32m", r1, s1), ("f32", r0, s0)):
        fresh = M._engine(state_dict, H_, W, B, dtype)
        rf = G._run(fresh, x)
        sf = M._all_stages(fresh, B)
        for st in M.ALL_STAGES:
            assert torch.equal(s[st], sf[st]), f"{st}: the {dtype} forward after a split forward differs from a fresh {dtype} engine's"
        assert torch.equal(r[0], rf[0]) and torch.equal(r[1], rf[1]), dtype
        fresh.close()
    e.close()


# ---- 5. the device against the host walk ------------------------------------------------------------------------------------------------------
def test_device_against_the_host_walk_layer4_1_conv1(state_dict):
    """layer4.1.conv1 at 65x71, B = 1, 32 shares of 9 steps, from the device's own input tap: every element within the fma-chain bound
    of oracle/conv_bound.py, and every element equal, bit for bit, to the host walk (std::fmaf chains per share from +0 in the kernel's
    operand order, the ordered adds of finalize).  Measured on an MI355X before the equality was asserted: 0 of 4608 elements differ."""
    H_, W, B = 65, 71, 1
    ksp = HK._load("libflope_host_f32m_ksplit.so", ("f32m_image_floats", "f32m_stem_image_floats", "f32m_ksplit_ws_bytes"))
    torch.manual_seed(21)
    x = torch.rand(B, 3, H_, W)
    e = M._engine(state_dict, H_, W, B, f32m_ksplit=32)
    G._run(e, x)
    assert _split_layers(e, B).get("base.layer4.1.conv1") == 32
    xin, got = e.read_stage("layer4.0", B).cpu(), e.read_stage("layer4.1.mid", B).cpu()
    e.close()
    assert xin.shape == (1, 512, 3, 3) and got.shape == (1, 512, 3, 3)
    spec = CB.trunk_specs(state_dict, F32)["layer4.1.conv1"]
    ref, bound = CB.reference(spec, xin, F32)
    rep = CB.check("layer4.1.conv1", got, ref, bound)
    print(f"  device: max err/bound {rep.max_ratio:.4f}, {rep.count} of {rep.total} over")
    assert rep.count == 0, rep
    host = HK._run_split(ksp, spec, xin, None, 1, 32)
    diff = got != host
    ulps = (got.view(torch.int32).long() - host.view(torch.int32).long()).abs()
    print(f"  device vs host walk: {int(diff.sum())} of {diff.numel()} elements differ, max {int(ulps.max())} ulp")
    assert CB.check("layer4.1.conv1 (host walk)", host, ref, bound).count == 0
    assert torch.equal(got, host)


# ---- 6. guard -----------------------------------------------------------------------------------------------------------------------------------
def test_guard_over_the_split_trunk(both_kinds):
    sd, x, _, Rref = both_kinds
    xyz = torch.rand(16, 3, generator=torch.Generator().manual_seed(2))
    g = GD._guard(sd, 224, 224, 16, exact_dtype="f32mk")
    got = GD._poses(g, x, xyz, guard=True)
    assert g.last_repaired == 8 and g.read_selection() == GD.B_ROWS
    assert _split_layers(g.exact, 8), "the repair of eight crops split nothing"
    dR = (got[1].view(-1, 3, 3) - Rref).abs().amax(dim=(1, 2))
    print(f"  guardk: max|dR| A {float(dR[:8].max()):.3e}  B {float(dR[8:].max()):.3e}; repair split {_split_layers(g.exact, 8)}")
    assert dR.max() <= 1e-3
    plain = G._engine(sd, 224, 224, 16, "f16")
    fast = GD._poses(plain, x, xyz)
    exact_e = G._engine(sd, 224, 224, 8, "f32mk")
    exact = GD._poses(exact_e, x[8:], xyz[8:])                              # the same chunk: all eight in one forward (max_repair 32)
    assert _split_layers(exact_e, 8) == _split_layers(g.exact, 8)
    for name, a, f, ex in zip(("r9", "R", "Rt"), got, fast, exact):
        assert torch.equal(a[:8], f[:8]), f"{name}: a row of group A differs from the plain f16 engine's"
        assert torch.equal(a[8:], ex), f"{name}: a row of group B differs from the f32mk engine's forward of those crops alone"
    for e_ in (g, plain, exact_e):
        e_.close()
    with pytest.raises(ValueError, match="exact_dtype"):
        GD._guard(sd, 224, 224, 16, exact_dtype="f16")


def test_guarded_frame_handle_over_guardk(state_dict):
    """flope_frame_* over the guard PoseResNet(compute_dtype="guardk") builds, everything flagged, against the same handle over an
    f32mk engine -- the set-up of test_guarded_frame_handle_with_more_boxes_than_the_engine_holds, with a guard that holds all seven
    in-frame crops so that both sides run them in one forward of seven (the share counts depend on the batch)."""
    from flope_amd.engine import PoseEngine
    from flope_amd.frame import FramePoses
    from sunflower.models.posenet import PoseResNet
    from sunflower.predictor.fast_pose_predictor import upload_depth
    rgb, mask, depth, boxes = G._scene(22)
    K = np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]])
    dev = torch.device("cuda")
    det = torch.zeros((16, 8), dtype=torch.float32)
    det[:len(boxes), :4] = torch.from_numpy(boxes.astype(np.float32))
    det, count = det.to(dev), torch.tensor([len(boxes)], dtype=torch.int32, device=dev)
    frame_d, mask_d, depth_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(mask).to(dev), upload_depth(depth, dev)
    e = PoseEngine(96, 96, 8, "f32mk")
    e.load_state_dict(state_dict)
    ctx = FramePoses(e, 480, 640, 16, 1)
    want = ctx.to_poses(det, count, frame_d, mask_d, depth_d, K)
    assert _split_layers(e, 7)
    ctx.close()
    e.close()
    net = PoseResNet(compute_dtype="guardk", max_batch=8).to("cuda")
    net.load_state_dict(state_dict)
    g = net.engine_for("cuda", (96, 96), 8)
    assert g.guard_handle and g.max_repair == 8
    g.gap_min = 1e9
    ctx = FramePoses(g, 480, 640, 16, 1)
    got = ctx.to_poses(det, count, frame_d, mask_d, depth_d, K)
    assert g.read_selection(0) == list(range(7)) and _split_layers(g.exact, 7)
    assert want.shape[0] == 6 and np.array_equal(got, want)
    ctx.close()
    g.close()


# ---- 7. public surface -------------------------------------------------------------------------------------------------------------------------
def test_posenet_module_in_f32mk(state_dict, golden_cfg1, monkeypatch):
    from sunflower.models.posenet import PoseResNet
    from sunflower.utils.conversion import procrustes_to_rotmat
    torch.manual_seed(0)
    x = torch.rand(16, 3, 224, 224).cuda()
    net = PoseResNet(compute_dtype="f32mk", max_batch=16).to("cuda")
    net.load_state_dict(state_dict)
    R = procrustes_to_rotmat(net(x)).cpu()
    Rg = torch.from_numpy(golden_cfg1["R"])
    print(f"cfg1 f32mk: |R - golden|max = {float((R - Rg).abs().max()):.3e}")
    assert (R - Rg).abs().max() <= 1e-4
    e = net.engine_for("cuda", (224, 224), 16)
    assert e.set_option("f32mfma", 1) == 1 and e.set_option("f32m_ksplit", 1) == 1
    assert _split_layers(e, 16) and sum(k.startswith("conv_f32m_kernel<") for _, k, _ in e.launch_info(16)) == 20
    monkeypatch.setenv("FLOPE_DTYPE", "f32mk")
    env = PoseResNet(max_batch=16).to("cuda")
    assert env.compute_dtype == "f32mk"
    env.load_state_dict(state_dict)
    assert torch.equal(env(x), net(x))
    e2 = env.engine_for("cuda", (224, 224), 16)
    assert e2.set_option("f32m_ksplit", 1) == 1 and e2.launch_info(16) == e.launch_info(16)


def test_option_is_a_no_op_on_a_16_bit_engine(state_dict):
    torch.manual_seed(1)
    x = torch.rand(3, 3, 96, 80)
    e = M._engine(state_dict, 96, 80, 3, "f16")
    before = G._run(e, x)
    info = e.launch_info(3)
    plan = e.describe_plan()
    assert e.set_option("f32m_ksplit", 1) == 0 and e.set_option("f32m_ksplit", 99) == 1 and e.set_option("f32m_ksplit", 7) == 32
    assert e.set_option("f32m_ksplit", 7) == 7
    after = G._run(e, x)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert e.launch_info(3) == info and e.describe_plan() == plan
    e.close()
