"""Step schedule options of the pose engine: `inline0` (slice 0 on the caller's stream) and `inplace` (block outputs
over their residual input) change where work is queued and which buffer a launch names -- never a launch, never a bit.  Every
comparison here is torch.equal against an engine that runs with both options off."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
OFF = {"inline0": 0, "inplace": 0}


def _engine(state_dict, H, W, B, dtype, **opts):
    from flope_amd.engine import PoseEngine
    e = PoseEngine(H, W, B, dtype)
    for k, v in opts.items():
        e.set_option(k, v)
    e.load_state_dict(state_dict)
    return e


def _crops(H, W, B, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype.startswith("f32"):
        return torch.rand(B, 3, H, W, generator=g).cuda()
    return torch.rand(B, H, W, 3, generator=g).to(TDT[dtype]).cuda()


def _fmt(x):
    from flope_amd.engine import input_format
    return input_format(x)


def _outputs(e, x, xyz):
    """r9, R (flope_forward) and Rt (flope_forward_poses, yaw nullified) of one batch"""
    r9, R = e.forward(x)
    Rt = torch.empty(x.shape[0], 16, device="cuda")
    e.forward_poses_into(x, _fmt(x), xyz, True, Rt)
    torch.cuda.synchronize()
    return r9.cpu(), R.cpu(), Rt.cpu()


def _same(a, b, what):
    for name, u, v in zip(("r9", "R", "Rt"), a, b):
        assert torch.equal(u, v), (what, name, float((u - v).abs().max()))


# ---- 1. no bit moves ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("B", [64, 71, 19])      # two even slices (the smallest batch that runs two), two uneven ones, one slice
def test_options_move_no_bit(state_dict, dtype, B):
    x = _crops(224, 224, B, dtype, 100 + B)
    xyz = torch.rand(B, 3, generator=torch.Generator().manual_seed(B)).cuda()
    ref_e = _engine(state_dict, 224, 224, B, dtype, **OFF)
    ref = _outputs(ref_e, x, xyz)
    ref_e.close()
    e = _engine(state_dict, 224, 224, B, dtype)
    for inline0 in (0, 1):
        for inplace in (0, 1):
            e.set_option("inline0", inline0)
            e.set_option("inplace", inplace)
            _same(_outputs(e, x, xyz), ref, dict(inline0=inline0, inplace=inplace))
    e.close()


def _conv2(info):
    return [(layer, kern) for layer, kern, _ in info if "conv2" in layer]


INPLACE_CASES = [
    # H, W, B, dtype, options, what must have run a conv2 (a conv with a residual)
    (224, 224, 4, "f16", {"ksplit": 2}, lambda i: any("[split-K" in l and "conv_stag_kernel<256x128>" in k for l, k in _conv2(i))),
    (224, 224, 19, "f16", {"dsfuse": 0}, lambda i: any("downsample" in l for l, _, _ in i) and not any("+shortcut" in l for l, _, _ in i)),
    # 65 x 71 by default: conv_mfma runs the stride-2 convs, every conv2 a ragged conv_stag tile (17 x 18 .. 3 x 3 maps) or its
    # split-K finalize; with stag = 0 every conv2 is a conv_mfma launch with a residual (added here, beyond the default plan)
    (65, 71, 2, "f16", {}, lambda i: any("conv_mfma_kernel" in k for _, k, _ in i) and any("conv_stag_kernel<512x64>" in k for _, k in _conv2(i))),
    (65, 71, 2, "f16", {"stag": 0}, lambda i: all("conv_mfma_kernel" in k for _, k in _conv2(i))),
    (200, 136, 7, "bf16", {}, lambda i: len(_conv2(i)) == 8),
    (512, 512, 2, "f16", {}, lambda i: any("conv_stag_kernel<8rows x64>" in k for _, k in _conv2(i))),
    (224, 224, 4, "f32", {}, lambda i: all(k == "naive_conv_kernel" for _, k in _conv2(i))),
    (224, 224, 2, "f32m", {}, lambda i: all(k.startswith("conv_f32m_kernel") for _, k in _conv2(i))),
]


@pytest.mark.parametrize("H,W,B,dtype,opts,reached", INPLACE_CASES, ids=[f"{c[0]}x{c[1]}-B{c[2]}-{c[3]}-{'-'.join(c[4]) or 'default'}" for c in INPLACE_CASES])
def test_inplace_moves_no_bit_in_any_family_with_a_residual(state_dict, H, W, B, dtype, opts, reached):
    x = _crops(H, W, B, dtype, 7 * H + B)
    xyz = torch.rand(B, 3, generator=torch.Generator().manual_seed(B)).cuda()
    ref_e = _engine(state_dict, H, W, B, dtype, **OFF, **opts)
    ref = _outputs(ref_e, x, xyz)
    ref_e.close()
    e = _engine(state_dict, H, W, B, dtype, inplace=1, **opts)
    got = _outputs(e, x, xyz)
    info = e.launch_info(B)
    assert reached(info), info
    _same(got, ref, (H, W, B, dtype, opts))
    e.close()


def test_inplace_layer1_runs_conv_r4_and_the_strided_layers_their_own_kernels(state_dict):
    """the shapes above reach split-K, conv_mfma, the column segments, naive and conv_f32m; the bench's own families (conv_r4,
    conv_s1r, conv_w4 with the residual by LDS-DMA) are the ones test_options_move_no_bit runs at B = 64 / 71: said here"""
    e = _engine(state_dict, 224, 224, 64, "f16", inplace=1)
    kernels = {k.split("<")[0] for _, k in _conv2(e.launch_info(64))}
    assert {"conv_r4_kernel", "conv_s1r_kernel", "conv_w4_kernel"} <= kernels, kernels
    e.close()


# ---- 2. stages ----------------------------------------------------------------------------------------------------------------------
SERVED = {"stem", "feat", "hidden"} | {f"layer{li}.1" for li in range(1, 5)} | {f"layer{li}.1.mid" for li in range(1, 5)}


@pytest.mark.parametrize("opts", [{}, {"dsfuse": 0, "fuse_stem": 0}], ids=["default", "shortcut-and-stem-materialised"])
def test_inplace_serves_the_stages_its_buffers_still_hold(state_dict, opts):
    from flope_amd.engine import STAGES
    B = 5
    x = _crops(224, 224, B, "f16", 21)
    ref_e = _engine(state_dict, 224, 224, B, "f16", **OFF, **opts)
    ref_e.forward(x)
    e = _engine(state_dict, 224, 224, B, "f16", inplace=1, **opts)
    e.forward(x)
    n_served = n_refused = 0
    for name in STAGES:
        try:
            want = ref_e.read_stage(name, B).cpu()
        except RuntimeError as err:                  # not materialised in this configuration (fused stem, folded shortcut): either way
            assert "not materialised" in str(err), (name, err)
            with pytest.raises(RuntimeError, match="flope_amd error -3"):
                e.read_stage(name, B)
            continue
        if name in SERVED:
            assert torch.equal(e.read_stage(name, B).cpu(), want), name
            n_served += 1
        else:
            with pytest.raises(RuntimeError, match=r"flope_amd error -3: .*option inplace"):
                e.read_stage(name, B)
            n_refused += 1
    assert n_served >= 10 and n_refused >= 9, (n_served, n_refused)      # 4 + 4 + feat + hidden; pool + 4 block outputs + 4 conv1 outputs
    # the option off again: the next forward serves every stage the default serves
    e.set_option("inplace", 0)
    with pytest.raises(RuntimeError, match="option inplace"):          # ... but not before it: the map of the LAST forward counts
        e.read_stage("pool", B)
    e.forward(x)
    for name in STAGES:
        try:
            want = ref_e.read_stage(name, B).cpu()
        except RuntimeError:
            continue
        assert torch.equal(e.read_stage(name, B).cpu(), want), name
    e.close()
    ref_e.close()


# ---- 3. rings and toggling ------------------------------------------------------------------------------------------------------------
def test_toggling_inplace_leaves_rings_and_shared_buffers_intact(state_dict):
    B = 6
    xs = [_crops(224, 224, B, "f16", 40 + i) for i in range(4)]
    xyz = torch.zeros(B, 3).cuda()
    e = _engine(state_dict, 224, 224, B, "f16")
    for i, x in enumerate(xs):
        inplace = 1 - i % 2                          # 1 -> 0 -> 1 -> 0
        e.set_option("inplace", inplace)
        got = _outputs(e, x, xyz)
        if not inplace:
            fresh = _engine(state_dict, 224, 224, B, "f16", **OFF)
            _same(got, _outputs(fresh, x, xyz), f"forward {i}")
            for name in ("pool", "layer1.0", "layer1.0.mid", "layer2.0", "layer4.1"):      # buffers the forward before wrote other maps into
                assert torch.equal(e.read_stage(name, B), fresh.read_stage(name, B)), (i, name)
            fresh.close()
    e.close()


# ---- 4. stream order ------------------------------------------------------------------------------------------------------------------
def test_inline0_keeps_the_callers_stream_order(state_dict):
    """x is written on a non-default stream right before each call and the outputs are cloned on it right after, two calls back to
    back through ONE input buffer, no host synchronisation in between: the second copy must wait for both slices of the first
    call, the clones for both slices of theirs."""
    B = 64
    xa, xb = _crops(224, 224, B, "f16", 61), _crops(224, 224, B, "f16", 62)
    ref_e = _engine(state_dict, 224, 224, B, "f16", **OFF)
    want = []
    for x in (xa, xb):
        r9, R = ref_e.forward(x)
        torch.cuda.synchronize()
        want.append((r9.cpu(), R.cpu()))
    ref_e.close()
    assert not torch.equal(want[0][0], want[1][0])
    e = _engine(state_dict, 224, 224, B, "f16", inline0=1)
    xbuf = torch.empty_like(xa)
    outs = [(torch.empty(B, 9, device="cuda"), torch.empty(B, 9, device="cuda")) for _ in range(2)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    got = []
    with torch.cuda.stream(s):
        for x, (r9, R) in zip((xa, xb), outs):
            xbuf.copy_(x, non_blocking=True)
            e.forward_into(xbuf, 2, r9, R)
            got.append((r9.clone(), R.clone()))
    s.synchronize()
    for i in range(2):
        assert torch.equal(got[i][0].cpu(), want[i][0]), i
        assert torch.equal(got[i][1].cpu().view(B, 3, 3), want[i][1]), i
    e.close()


# ---- 5. time line ---------------------------------------------------------------------------------------------------------------------
def test_timeline_and_profile_keep_their_meaning_under_inline0(state_dict):
    B = 64
    x = _crops(224, 224, B, "f16", 71)
    R = torch.empty(B, 9, device="cuda")
    e = _engine(state_dict, 224, 224, B, "f16", inline0=1)
    n_launch = e.launches()
    e.set_option("profile", 2)
    for _ in range(2):
        e.forward_into(x, 2, None, R)
    ms, sl = (C.c_float * 256)(), (C.c_int * 256)()
    n = e.lib.flope_profile_timeline(e.handle, ms, sl, 256)
    assert n == 1 + 2 * (n_launch + 1), n             # the fork + per slice: one mark in front of every launch, one behind the last
    assert ms[0] == 0.0 and sl[0] == 0                # event 0 = the fork
    for s in (0, 1):
        t = [ms[i] for i in range(1, n) if sl[i] == s]
        assert len(t) == n_launch + 1, (s, len(t))
        assert all(0.0 <= a <= b for a, b in zip(t, t[1:])), (s, t)
    e.set_option("profile", 1)
    e.forward_into(x, 2, None, R)
    per_launch = e.profile_read()
    assert len(per_launch) == n_launch and all(v > 0.0 for v in per_launch)
    e.close()
