"""flope_depth_lift (flope_amd/csrc/prep.hip: depth_box_kernel / depth_box_final_kernel) at box, strip and frame edges against an
fp64 reference that exposes the count (oracle.pipeline_ref.depth_stats64).  Cases and checker: tests/depth_cases.py; what the cases
promise and which kernel defects they catch: tests/test_depth_cases.py (CPU).

Per case and row:  reliable == (count >= 50);  |depth_val - mean64| <= 2^-23 mean64 and exactly 0 where count == 0;
|xyz - get_points3d(mean64)| <= 2^-23 |component| on every row, unreliable ones included, zeros where count == 0.
The bound: the kernel sums at most 2^21 float32 millimetre values in float64 and divides twice in float64 (< 2^-31 relative), then
rounds once to float32 (2^-24); 2^-23 is twice that.  Run with -s for the worst |err| / bound of every case.
"""
import numpy as np
import pytest
import torch

import depth_cases as DC
from oracle import pipeline_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    return DC.load_plan()


def _upload(c, storage=None):
    d = c.depth
    if d.dtype == np.uint16:
        t = torch.from_numpy(d.view(np.int16).copy())
        if storage == "uint16":
            t = t.view(torch.uint16)
        return t.cuda()
    return torch.from_numpy(d.copy()).cuda()


def _lift(c, storage=None):
    from flope_amd import engine as E
    dv, rel, xyz = E.depth_lift(_upload(c, storage), torch.from_numpy(c.mask.copy()).cuda(), torch.from_numpy(c.boxes.copy()).cuda(),
                                c.K4, c.depth_div, c.near, c.far)
    torch.cuda.synchronize()
    assert dv.dtype == torch.float32 and rel.dtype == torch.bool and xyz.dtype == torch.float32
    return dv.cpu().numpy(), rel.cpu().numpy(), xyz.cpu().numpy()


def _judge(c, out, what):
    fails, r_dv, r_xyz = DC.check(c, *out)
    count, mean = DC.reference(c)
    dv32, _ = P.get_depth_value(c.boxes.tolist(), DC.metres(c), c.mask, near_plane=c.near, far_plane=c.far)
    own = float((np.abs(dv32 - mean)[count > 0] / (DC.U23 * mean[count > 0])).max())
    print(f"{what}: {len(count)} boxes, counts {int(count.min())}..{int(count.max())}, worst |err| / bound: depth_val {r_dv:.3f}, "
          f"xyz {r_xyz:.3f}   (for the record: the reference's own float32 np.mean is {own:.3f} bounds from fp64)")
    assert not fails, fails[:8]
    assert r_dv <= 1.0 and r_xyz <= 1.0


@pytest.mark.parametrize("name", DC.NAMES)
def test_depth_lift_case_vs_fp64(plan, name):
    c = DC.case(plan, name)
    out = _lift(c)
    _judge(c, out, name)
    again = _lift(c)                                    # strip partials are combined in strip order: no dependence on timing
    for a, b in zip(out, again):
        assert a.tobytes() == b.tobytes()


def test_uint16_storage_of_the_high_half(plan):
    """raw values >= 32768 as torch.uint16 and as the int16 view of the same bits: the same result, held to the same reference"""
    c = DC.case(plan, "high16")
    a = _lift(c, None)
    _judge(c, a, "high16 as the int16 view")
    if hasattr(torch, "uint16"):
        b = _lift(c, "uint16")
        _judge(c, b, "high16 as torch.uint16")
        for p, q in zip(a, b):
            assert p.tobytes() == q.tobytes()


def test_no_boxes(plan):
    from flope_amd import engine as E
    c = DC.case(plan, "odd")
    dv, rel, xyz = E.depth_lift(_upload(c), torch.from_numpy(c.mask.copy()).cuda(), torch.zeros((0, 4), dtype=torch.int32).cuda(),
                                c.K4, c.depth_div, c.near, c.far)
    assert dv.shape == (0,) and rel.shape == (0,) and xyz.shape == (0, 3)
    assert dv.dtype == torch.float32 and rel.dtype == torch.bool and xyz.dtype == torch.float32
