"""flope_crop_resize_mask (flope_amd/csrc/prep.hip: crop_resize_mask_tiled_kernel) at box, tile and path edges, bit for bit against
oracle.pipeline_ref.crop_batch.  Cases and checker: tests/crop_cases.py; what the cases promise and which kernel defects they
notice: tests/test_crop_cases.py (CPU).

Per case and output format (float32 NCHW, bfloat16 NHWC, float16 NHWC) the kernel writes into a buffer this test allocates: the N
crops and one more crop's worth behind them, all pre-filled with a sentinel.  Every element of a live crop must have the
reference's bits, every element of a degenerate crop (cw <= 0 or ch <= 0) must be zero, the tail must still be the sentinel, and a
second call must give the same bytes.  No tolerance anywhere.  Run with -s for the number of tiles on each path.
"""
import numpy as np
import pytest
import torch

import crop_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plan():
    return CC.load_plan()


def _call(c, fmt, n=None):
    """one call into a sentinel-filled buffer -> (return code, the buffer as element bits)"""
    from flope_amd import _lib, engine as E
    assert (_lib.IN_F32_NCHW, _lib.IN_BF16_NHWC, _lib.IN_F16_NHWC) == tuple(CC.FMT_CODE[f] for f in CC.FORMATS)
    H, W = c.mask.shape
    frame = torch.from_numpy(c.rgb.copy()).cuda()
    mask = torch.from_numpy(c.mask.copy()).cuda()
    boxes = torch.from_numpy(c.boxes.copy()).cuda()
    assert frame.is_contiguous() and mask.is_contiguous() and boxes.is_contiguous() and boxes.dtype == torch.int32
    out = torch.full((CC.new_buffer(c, fmt).nbytes,), CC.SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    with torch.cuda.device(out.device):
        rc = _lib.load().flope_crop_resize_mask(frame.data_ptr(), mask.data_ptr(), H, W, boxes.data_ptr(),
                                                len(c.boxes) if n is None else n, c.S, CC.FMT_CODE[fmt], out.data_ptr(),
                                                E._stream_ptr(out.device))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().view(CC.BITS_DTYPE[fmt])


@pytest.mark.parametrize("name", CC.NAMES)
def test_crop_case_bit_for_bit(plan, name):
    c = CC.case(plan, name)
    sep, direct, mixed = CC.path_counts(plan, c)
    print(f"{name}: {len(c.boxes)} boxes at S = {c.S}: {sep} tiles on the separable path, {direct} on the direct path, "
          f"{mixed} crops with both")
    for fmt in CC.FORMATS:
        rc, buf = _call(c, fmt)
        assert rc == 0
        fails = CC.check(plan, c, fmt, buf)
        assert not fails, fails[:8]
        rc, again = _call(c, fmt)
        assert rc == 0 and buf.tobytes() == again.tobytes()


@pytest.mark.parametrize("fmt", CC.FORMATS)
def test_no_boxes_touches_nothing(plan, fmt):
    c = CC.case(plan, "degenerate")
    rc, buf = _call(c, fmt, n=0)
    assert rc == 0 and (buf == CC.SENTINEL[fmt]).all()
