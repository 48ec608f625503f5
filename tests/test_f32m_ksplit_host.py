"""Split-K of the float32 MFMA trunk (engine option f32m_ksplit, flope_amd/csrc/conv_f32m.hip, plan.h f32m_ksplit) as far as a CPU
can see it.

1.  The option and the planner (plan.h through the existing host harness): off = today's plan text, ignored where it does not
    apply, and for every split launch the invariants the kernel's bounds rest on.
2.  The arithmetic: a scalar walk of the split launch + the finalize launch over the packed image (tests/host_harness/
    harness_f32m_ksplit.cpp) against the fp64 oracle of oracle/conv_bound.py with the two assertions of tests/test_f32m_host.py
    (every element within `bound`, relL2 within `statistical_bound`, u = 2^-24).  The bound is order-free -- it holds for any
    order of the K products and any association of the partial sums -- so it is the same bound at every S.
The helpers of tests/test_f32m_host.py are imported, not copied.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import conv_bound as CB

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_f32m_host as H  # noqa: E402

ROOT = H.ROOT
DT_F16, DT_F32, F32 = H.DT_F16, H.DT_F32, H.F32
CUS = 256
CANDIDATES = (2, 4, 8, 16, 32)


@pytest.fixture(scope="module")
def f32m():
    return _load("libflope_host_f32m.so", ("f32m_image_floats", "f32m_stem_image_floats"))


def _load(name, longs=()):
    path = os.path.join(ROOT, "tests", "host_harness", name)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/" + name])
    lib = C.CDLL(path)
    for fn in longs:
        getattr(lib, fn).restype = C.c_long
    return lib


@pytest.fixture(scope="module")
def ksp():
    return _load("libflope_host_f32m_ksplit.so", ("f32m_image_floats", "f32m_stem_image_floats", "f32m_ksplit_ws_bytes"))


# ---- 1. option ----------------------------------------------------------------------------------------------------------------------
def test_option_defaults_to_off_and_stores_clamped(harness):
    v = C.c_int(-7)
    assert harness.flope_host_option_default(b"f32m_ksplit", C.byref(v)) == 0 and v.value == 0
    probes = [-3, 0, 1, 2, 7, 32, 99]
    stored = (C.c_int * len(probes))()
    calls = ",".join(f"f32m_ksplit={p}" for p in probes).encode()
    assert harness.flope_host_set_options(calls, stored, len(probes)) == len(probes)
    assert list(stored) == [0, 0, 1, 2, 7, 32, 32]
    assert harness.flope_host_set_options(b"f32m_ksplt=1", stored, len(probes)) == -1          # an unknown name is still refused
    assert harness.flope_host_option_default(b"f32m_ksplt", C.byref(v)) == -1


@pytest.mark.parametrize("Hh,W,B", H.SHAPES)
def test_option_off_is_todays_plan_text(harness, Hh, W, B):
    assert H._dump(harness, Hh, W, B, DT_F32, "f32mfma=1,f32m_ksplit=0")[0] == H._dump(harness, Hh, W, B, DT_F32, "f32mfma=1")[0]


@pytest.mark.parametrize("Hh,W,B", H.SHAPES)
@pytest.mark.parametrize("v", [1, 32])
def test_ignored_where_it_does_not_apply(harness, Hh, W, B, v):
    assert H._dump(harness, Hh, W, B, DT_F16, f"f32m_ksplit={v}")[0] == H._dump(harness, Hh, W, B, DT_F16)[0]
    assert H._dump(harness, Hh, W, B, DT_F32, f"f32m_ksplit={v}")[0] == H._dump(harness, Hh, W, B, DT_F32)[0]          # strict float32
    assert H._dump(harness, Hh, W, B, DT_F32, f"f32mfma=0,f32m_ksplit={v}")[0] == H._dump(harness, Hh, W, B, DT_F32)[0]


# ---- planner invariants ------------------------------------------------------------------------------------------------------------------
_SHAPE_RE = re.compile(r"^(\S+): (\d)x\d s(\d) (\d+)->(\d+) out (\d+)x(\d+)", re.M)


def _convs(harness, Hh, W, B, opts):
    """-> (text, plan_slices, [dict per trunk conv launch of the last slice])"""
    text, plan, sl, launches = H._dump(harness, Hh, W, B, DT_F32, opts)
    plan_slices = int(text.split("slices|")[1].split("|")[1])
    shape = {m.group(1): tuple(int(g) for g in m.groups()[1:]) for m in _SHAPE_RE.finditer(plan)}
    out = []
    for l in launches:
        if len(l) != 12:
            continue
        k, stride, cin, cout, ho, wo = shape[l[0]]
        out.append(dict(layer=l[0], label=l[1], detail=l[2], grid=int(l[3]), lds=int(l[4]), mtiles=int(l[5]), ntiles=int(l[6]), ksplit=int(l[7]),
                        mp=int(l[8]), total=int(l[11]), k=k, cin=cin, cout=cout, nsteps=k * k * cin // 16, M=sl[-1][1] * ho * wo))
    assert len(out) == 19
    return text, plan_slices, out


MATRIX_HW = [(65, 71), (96, 80), (224, 224), (512, 512)]
MATRIX_B = [1, 2, 3, 4, 8, 16, 31, 37, 64, 256]
MATRIX_V = [1, 2, 8, 32]


@pytest.mark.parametrize("Hh,W", MATRIX_HW)
def test_planner_invariants_of_every_split_launch(harness, ksp, Hh, W):
    min_share, ws_bytes = ksp.f32m_ksplit_min_share_steps(), ksp.f32m_ksplit_ws_bytes(CUS)
    assert min_share == 4 and ws_bytes == CUS * 256 * 64 * 4
    n_split = 0
    for B in MATRIX_B:
        off_text, _, off = _convs(harness, Hh, W, B, "f32mfma=1")
        for v in MATRIX_V:
            text, plan_slices, convs = _convs(harness, Hh, W, B, f"f32mfma=1,f32m_ksplit={v}")
            stem = [l for l in H._dump(harness, Hh, W, B, DT_F32, f"f32mfma=1,f32m_ksplit={v}")[3] if l[0] == "stem"]
            assert stem == [["stem", "conv_f32m_kernel<7x7,4ch>"]]                      # the stem: its own launch, no split detail
            for c, c0 in zip(convs, off):
                S = c["ksplit"]
                # the option changes the share count and the grid only
                assert {k: c[k] for k in c if k not in ("ksplit", "grid", "detail")} == {k: c0[k] for k in c0 if k not in ("ksplit", "grid", "detail")}
                assert c["label"].startswith("conv_f32m_kernel<") and c["total"] == c["mtiles"] * c["ntiles"]
                assert c["grid"] == c["total"] * S and c["detail"] == (f"[split-K x{S}]" if S > 1 else "")
                assert S == ksp.f32m_ksplit_plan(v, c["total"], c["mp"], c["nsteps"], plan_slices, CUS)
                if plan_slices > 1 or c["nsteps"] == 4:
                    assert S == 1, c                                                    # one workspace per engine; the 4-step shortcut
                if v >= 2 and S > 1:
                    assert S <= v and S == max(s for s in CANDIDATES if s <= v and c["total"] * s <= CUS and c["nsteps"] // s >= min_share)
                if S == 1:
                    continue
                n_split += 1
                assert S in CANDIDATES and c["grid"] <= CUS, c
                begins = [ksp.f32m_ksplit_share_begin(c["nsteps"], S, s) for s in range(S + 1)]
                assert begins[0] == 0 and begins[-1] == c["nsteps"]                    # the shares tile [0, nsteps) exactly ...
                assert all(b - a >= min_share for a, b in zip(begins, begins[1:])), (c, begins)   # ... and none is shorter than the minimum
                assert S * c["M"] * c["cout"] * 4 <= ws_bytes, c
            if B in (64, 256) and (Hh, W) == (224, 224):
                assert plan_slices == 2                                                 # the batches the mode was measured at: two slices
            if plan_slices > 1:
                assert text == off_text                                                 # ... where the dump equals option 0's
    assert n_split > 0


def test_one_crop_at_224_splits_every_3x3_conv_of_layers_3_and_4(harness):
    """16 and 8 workgroups for 144 - 288 serial steps: no sensible constants decide otherwise."""
    _, _, convs = _convs(harness, 224, 224, 1, "f32mfma=1,f32m_ksplit=1")
    deep = [c for c in convs if c["k"] == 3 and ("layer3" in c["layer"] or "layer4" in c["layer"])]
    assert len(deep) == 8 and all(c["ksplit"] > 1 for c in deep), [(c["layer"], c["ksplit"]) for c in deep]
    print([(c["layer"], c["total"], c["nsteps"], c["ksplit"]) for c in convs])


def test_cost_model_minimises_its_own_figure(ksp):
    """value 1: the S in {1, 2, .., 32} allowed by the three rules with the smallest ceil(n / S) 655 mp + (S > 1) (4300 + 720 S) cycles,
    ties to the smaller S (plan.h kF32mStepCycles / kF32mFinalizeCycles / kF32mFinalizeShareCycles as fitted to the per-launch table
    of DESIGN.md 17)."""
    for tiles in (1, 8, 16, 32, 49, 100, 128, 129, 256):
        for mp in (1, 2, 4):
            for n in (4, 8, 16, 36, 72, 144, 288):
                def cost(S):
                    return -(-n // S) * 655 * mp + (4300 + 720 * S if S > 1 else 0)
                ok = [1] + [S for S in CANDIDATES if tiles * S <= CUS and n // S >= 4]
                want = min(ok, key=lambda S: (cost(S), S))
                assert ksp.f32m_ksplit_plan(1, tiles, mp, n, 1, CUS) == want, (tiles, mp, n)
                assert ksp.f32m_ksplit_plan(1, tiles, mp, n, 2, CUS) == 1 and ksp.f32m_ksplit_plan(0, tiles, mp, n, 1, CUS) == 1


# ---- 2. feed order -----------------------------------------------------------------------------------------------------------------------
def _run_split(ksp, spec, x, r, mp, S, expect_rc=0):
    """The scalar walk of one conv as a split launch of S shares + finalize -> [B,Cout,ho,wo] float32 (S = 1: the unsplit kernel)."""
    w = spec.w.contiguous().numpy()
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    B, _, h, wd = x.shape
    img = np.zeros(ksp.f32m_image_floats(cout, cin, k), dtype=np.float32)
    ksp.f32m_pack(H._ptr(w), cout, cin, k, H._ptr(img))
    xin = H._padded_nhwc(x)
    ho = (h + 2 * spec.padding - k) // spec.stride + 1
    wo = (wd + 2 * spec.padding - k) // spec.stride + 1
    res = H._padded_nhwc(r) if r is not None else None
    out = np.full((B, ho + 2, wo + 2, cout), 7.0, dtype=np.float32)              # the ring must come back untouched
    ws = np.full(max(S, 1) * B * ho * wo * cout, np.nan, dtype=np.float32)       # exactly S * M * Cout floats: one past is code 3 / 4
    bias = spec.b.contiguous().numpy()
    rc = ksp.f32m_ksplit_walk(H._ptr(xin), H._ptr(img), H._ptr(bias), H._ptr(res) if res is not None else None, H._ptr(out), H._ptr(ws),
                              C.c_long(ws.size), B, xin.shape[1], xin.shape[2], cin, ho, wo, cout, k, spec.stride, 0 if k == 3 else 1,
                              int(spec.relu), mp, S)
    if expect_rc:
        assert rc == expect_rc, rc
        return None
    assert rc == 0, f"the walk left a buffer or met an empty share (code {rc})"
    if S > 1:
        assert not np.isnan(ws).any(), "a workspace element no share wrote"
    ring = out.copy()
    ring[:, 1:-1, 1:-1, :] = 7.0
    assert (ring == 7.0).all(), "a store outside the interior"
    return torch.from_numpy(out[:, 1:-1, 1:-1, :]).permute(0, 3, 1, 2).contiguous()


SPLIT_CASES = [c for c in H.FEED_CASES if c[1] != "stem"]                         # the 3x3 and 1x1 cases (the stem is never split)


def _case_io(state_dict, case):
    title, name, shape, with_res, mp = case
    spec = CB.trunk_specs(state_dict, F32)[name]
    g = torch.Generator().manual_seed(5)
    x = torch.rand(shape, generator=g)
    ref0, _ = CB.reference(spec, x, F32)
    r = torch.rand(ref0.shape, generator=g) if with_res else None
    return spec, x, r


@pytest.mark.parametrize("S", [2, 8, 32])
@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_walk_and_finalize_against_fp64(ksp, state_dict, case, S):
    title, name, shape, with_res, mp = case
    spec, x, r = _case_io(state_dict, case)
    if spec.K // 16 < S:
        # 8 K steps cannot feed 32 shares: a share without a step does not exist in the kernel (its first load is unconditional), the
        # launch guard of conv_f32m.hip refuses nsteps / S < 1 and the planner keeps >= 4 steps per share -- the walk reports it
        assert name == "layer3.0.ds" and S == 32
        _run_split(ksp, spec, x, r, mp, S, expect_rc=5)
        return
    ref, bound = CB.reference(spec, x, F32, r)
    got = _run_split(ksp, spec, x, r, mp, S)
    rep = CB.check(name, got, ref, bound)
    stat = CB.statistical_bound(ref, bound, spec.K, F32)
    stat_rel = float(stat.norm() / ref.norm())
    print(f"{title} S={S}: max err/bound {rep.max_ratio:.4f}  relL2 {rep.rel_l2:.3e}  statistic allows {stat_rel:.3e}")
    fails = CB.verdict(rep, 0.0, F32, f"f32m split-K x{S} feed order (CPU)", stat_rel)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_one_share_is_the_unsplit_walk_bit_for_bit(f32m, ksp, state_dict, case):
    title, name, shape, with_res, mp = case
    spec, x, r = _case_io(state_dict, case)
    assert torch.equal(_run_split(ksp, spec, x, r, mp, 1), H._run(f32m, spec, x, r, mp))


@pytest.mark.parametrize("S", [2, 8])
def test_tile_height_does_not_change_a_bit_at_a_fixed_share_count(ksp, state_dict, S):
    spec = CB.trunk_specs(state_dict, F32)["layer2.0.conv1"]
    x = torch.rand((2, 64, 11, 13), generator=torch.Generator().manual_seed(6))
    a, b, c = (_run_split(ksp, spec, x, None, mp, S) for mp in (1, 2, 4))
    assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(a, _run_split(ksp, spec, x, None, 1, 1))             # (and the share count does: another summation order)
