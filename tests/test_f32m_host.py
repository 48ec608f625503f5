"""The float32 MFMA trunk (engine option f32mfma, flope_amd/csrc/conv_f32m.hip) as far as a CPU can see it.

1.  The planner (plan.h through the existing host harness): the option, and what a float32 engine launches under it.
2.  The weight packer of host_pack.h and the kernel's operand feed, through tests/host_harness/harness_f32m.cpp: a scalar walk
    that reads the packed image and a zero-bordered NHWC input exactly as lane (row / pixel, kq) and MFMA s of every 16-deep K
    step do, accumulating in float in that order, judged against the fp64 oracle of oracle/conv_bound.py: every element within
    `bound`, relL2 within `statistical_bound` (u = 2^-24) -- the same two assertions the GPU walk makes of the real kernel
    (tests/test_gpu_f32m.py).  One missing tap or one swapped row of the permutation is orders of magnitude outside both.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import conv_bound as CB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_F16, DT_F32 = 1, 2
F32 = torch.float32
SHAPES = [(224, 224, 4), (65, 71, 2), (512, 512, 2), (224, 224, 256)]


@pytest.fixture(scope="module")
def f32m():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_f32m.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_f32m.so"])
    lib = C.CDLL(path)
    lib.f32m_image_floats.restype = C.c_long
    lib.f32m_stem_image_floats.restype = C.c_long
    return lib


# ---- 1. planner ---------------------------------------------------------------------------------------------------------------------
def _dump(harness, H, W, B, dtype, opts=""):
    buf = C.create_string_buffer(1 << 16)
    n = harness.flope_host_plan_dump(H, W, B, dtype, 256, opts.encode(), B, buf, len(buf))
    assert n > 0, (H, W, B, dtype, opts, n)
    text = buf.value.decode()
    plan, rest = text.split("slices|")
    sl, rest = rest.split("\nlaunches=")
    lines = rest.split("\n")
    assert int(lines[0]) == len(lines[1:-1])
    slices = [tuple(int(v) for v in s.split(":")) for s in sl.split("|")[2].split()]
    return text, plan, slices, [ln.split("|") for ln in lines[1:-1]]


def test_option_defaults_to_off_and_stores_like_a_bool(harness):
    v = C.c_int(-7)
    assert harness.flope_host_option_default(b"f32mfma", C.byref(v)) == 0 and v.value == 0
    probes = [0, 1, 2, -1, 7, 0, 1]
    stored = (C.c_int * len(probes))()
    calls = ",".join(f"f32mfma={p}" for p in probes).encode()
    assert harness.flope_host_set_options(calls, stored, len(probes)) == len(probes)
    assert list(stored) == [int(p != 0) for p in probes]


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_float32_engine_plans_every_conv_on_the_new_kernel(harness, H, W, B):
    _, _, sl, on = _dump(harness, H, W, B, DT_F32, "f32mfma=1")
    _, _, sl0, off = _dump(harness, H, W, B, DT_F32)
    assert len(on) == len(off) == 3 + 19 + 3 and sl == sl0
    assert [l[0] for l in on] == [l[0] for l in off]                      # same layers in the same order
    assert on[0][:2] == ["prep_input", "prep_input_kernel"] and on[2][:2] == ["maxpool", "maxpool_kernel"]
    assert on[1][0] == "stem" and on[1][1].startswith("conv_f32m_kernel<") and off[1][1] == "naive_conv_kernel"
    convs = [l for l in on if len(l) == 12]
    assert len(convs) == 19
    assert not any("naive_conv_kernel" in "|".join(l) for l in on)
    for l in convs:
        label, grid, lds, mtiles, ntiles, ksplit, total = l[1], int(l[3]), int(l[4]), int(l[5]), int(l[6]), int(l[7]), int(l[11])
        assert label.startswith("conv_f32m_kernel<"), l
        assert grid >= 1 and grid <= total * max(1, ksplit) and lds <= 160 * 1024, l
        assert total == mtiles * ntiles and grid % ntiles == 0, l
    assert all(l[1] == "naive_conv_kernel" for l in off if len(l) == 12)
    # the slices tile the batch
    assert sl[0][0] == 0 and sum(c for _, c in sl) == B and all(a[0] + a[1] == b[0] for a, b in zip(sl, sl[1:]))


def test_launches_reserve_more_than_half_a_cu_of_lds(harness):
    """One workgroup per CU: every conv_f32m launch asks for 84 KiB (more than half of 160 KiB) that the kernel never touches."""
    _, _, _, launches = _dump(harness, 224, 224, 4, DT_F32, "f32mfma=1")
    assert [int(l[4]) for l in launches if len(l) == 12] == [84 * 1024] * 19


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_sixteen_bit_engines_ignore_the_option(harness, H, W, B):
    assert _dump(harness, H, W, B, DT_F16, "f32mfma=1")[0] == _dump(harness, H, W, B, DT_F16)[0]


def test_tile_height_minimises_whole_rounds_of_the_chip(f32m):
    """plan.h f32m_mp: one workgroup per CU, so a launch takes whole rounds of 256 workgroups; the cheapest of 4 / 2 / 1 pixel
    tiles per wave by rounds x (4 mp + 1), ties to the larger tile."""
    def cost(M, cout, mp):
        return -(-(-(-M // (64 * mp)) * (cout // 64)) // 256) * (4 * mp + 1)
    assert f32m.f32m_plan_mp(256 * 56 * 56, 64, 256) == 4          # many rounds: the large tile
    assert f32m.f32m_plan_mp(16 * 32 * 32, 256, 256) == 4          # 64 x 4 workgroups: one round exactly
    assert f32m.f32m_plan_mp(16 * 16 * 16, 512, 256) == 2          # 32 x 8 = one round at 128 pixels, half a round at 256
    assert f32m.f32m_plan_mp(4 * 7 * 7, 512, 256) == 1             # a small batch: as many workgroups as there are
    for M, cout in ((3136, 64), (3136, 512), (50176, 128), (12544, 256), (196, 512), (1, 64)):
        mp = f32m.f32m_plan_mp(M, cout, 256)
        assert mp in (1, 2, 4) and all(cost(M, cout, mp) <= cost(M, cout, o) for o in (1, 2, 4)), (M, cout, mp)


# ---- 2. packer and feed order -----------------------------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _padded_nhwc(t, border=1, hip=None, wip=None, cstored=None):
    """[B,C,h,w] -> zero-bordered NHWC float32 numpy array [B,hip,wip,cstored]."""
    B, Cc, h, w = t.shape
    hip, wip, cstored = hip or h + 2 * border, wip or w + 2 * border, cstored or Cc
    a = np.zeros((B, hip, wip, cstored), dtype=np.float32)
    a[:, border:border + h, border:border + w, :Cc] = t.permute(0, 2, 3, 1).numpy()
    return a


def _run(f32m, spec, x, r, mp, stem=False):
    """The scalar walk of one conv -> [B,Cout,ho,wo] float32 and the whole padded output buffer."""
    w = spec.w.contiguous().numpy()
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    B, _, h, wd = x.shape
    if stem:
        img = np.zeros(f32m.f32m_stem_image_floats(), dtype=np.float32)
        f32m.f32m_pack_stem(_ptr(w), _ptr(img))
        xin = _padded_nhwc(x, 3, h + 6, (wd + 8 + 1) & ~1, 4)
        in_off, cstored = 0, 4
    else:
        img = np.zeros(f32m.f32m_image_floats(cout, cin, k), dtype=np.float32)
        f32m.f32m_pack(_ptr(w), cout, cin, k, _ptr(img))
        xin = _padded_nhwc(x)
        in_off, cstored = (0 if k == 3 else 1), cin
    ho = (h + 2 * spec.padding - k) // spec.stride + 1
    wo = (wd + 2 * spec.padding - k) // spec.stride + 1
    res = _padded_nhwc(r) if r is not None else None
    out = np.full((B, ho + 2, wo + 2, cout), 7.0, dtype=np.float32)          # the ring must come back untouched
    bias = spec.b.contiguous().numpy()
    rc = f32m.f32m_walk(_ptr(xin), _ptr(img), _ptr(bias), _ptr(res) if res is not None else None, _ptr(out), B, xin.shape[1], xin.shape[2],
                        cstored, cin, ho, wo, cout, k, spec.stride, in_off, int(spec.relu), int(stem), mp)
    assert rc == 0, f"the walk left a buffer (code {rc})"
    ring = out.copy()
    ring[:, 1:-1, 1:-1, :] = 7.0
    assert (ring == 7.0).all(), "a store outside the interior"
    return torch.from_numpy(out[:, 1:-1, 1:-1, :]).permute(0, 3, 1, 2).contiguous()


FEED_CASES = [
    # name, spec, input [B, Cin, h, w], residual, pixel tiles per wave
    ("3x3 s1 64->64 + residual", "layer1.0.conv2", (2, 64, 9, 11), True, 2),
    ("3x3 s2 64->128", "layer2.0.conv1", (2, 64, 11, 13), False, 1),
    ("1x1 s2 128->256", "layer3.0.ds", (2, 128, 9, 10), False, 4),
    ("3x3 s1 512->512 on 3x5 (ragged pixel tile)", "layer4.1.conv1", (1, 512, 3, 5), False, 1),
    ("stem on a 23x29 crop", "stem", (1, 3, 23, 29), False, 2),
]


@pytest.mark.parametrize("case", FEED_CASES, ids=[c[0] for c in FEED_CASES])
def test_packed_image_and_feed_order_against_fp64(f32m, state_dict, case):
    title, name, shape, with_res, mp = case
    spec = CB.trunk_specs(state_dict, F32)[name]
    g = torch.Generator().manual_seed(5)
    x = torch.rand(shape, generator=g)
    ref0, _ = CB.reference(spec, x, F32)
    r = torch.rand(ref0.shape, generator=g) if with_res else None
    ref, bound = CB.reference(spec, x, F32, r)
    got = _run(f32m, spec, x, r, mp, stem=name == "stem")
    rep = CB.check(name, got, ref, bound)
    stat = CB.statistical_bound(ref, bound, spec.K, F32)
    stat_rel = float(stat.norm() / ref.norm())
    print(f"{title}: max err/bound {rep.max_ratio:.4f}  relL2 {rep.rel_l2:.3e}  statistic allows {stat_rel:.3e}")
    fails = CB.verdict(rep, 0.0, F32, "f32m feed order (CPU)", stat_rel)
    assert not fails, "\n".join(fails)


def test_tile_height_does_not_change_a_bit(f32m, state_dict):
    """Every output is summed in one order whatever the tiling: 1, 2 and 4 pixel tiles per wave give the same floats."""
    spec = CB.trunk_specs(state_dict, F32)["layer2.0.conv1"]
    x = torch.rand((2, 64, 11, 13), generator=torch.Generator().manual_seed(6))
    a, b, c = (_run(f32m, spec, x, None, mp) for mp in (1, 2, 4))
    assert torch.equal(a, b) and torch.equal(a, c)


def test_packer_is_a_permutation_of_the_weights(f32m, state_dict):
    """Every folded weight appears exactly once in the image; the stem's image holds them plus zeros only."""
    specs = CB.trunk_specs(state_dict, F32)
    for name in ("layer2.0.conv1", "layer3.0.ds"):
        w = specs[name].w.contiguous().numpy()
        img = np.zeros(f32m.f32m_image_floats(*w.shape[:3]), dtype=np.float32)
        f32m.f32m_pack(_ptr(w), w.shape[0], w.shape[1], w.shape[2], _ptr(img))
        assert img.size == w.size and np.array_equal(np.sort(img), np.sort(w.ravel()))
    w = specs["stem"].w.contiguous().numpy()
    img = np.zeros(f32m.f32m_stem_image_floats(), dtype=np.float32)
    f32m.f32m_pack_stem(_ptr(w), _ptr(img))
    nz = img[img != 0]
    assert np.array_equal(np.sort(nz), np.sort(w.ravel()[w.ravel() != 0]))
