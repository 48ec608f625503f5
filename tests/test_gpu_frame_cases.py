"""The frame handle on the device (flope_frame_select / enqueue / finish / to_poses, flope_amd/csrc/frame.hip, FramePoses): box
selection integer for integer, capacity, several different frames in flight, the host path, failed calls, call order.  Cases and
checker: tests/frame_cases.py; what the cases promise and which defects of the selection kernel they notice:
tests/test_frame_cases.py (CPU).

Every comparison of poses is bit for bit: a frame through any slot, in any order, on a plain or a guarded handle, equals
`to_poses` of that frame alone on a fresh one-slot handle over the same engine (the forwards are the same chunks of 4, so no
tolerance is involved).  The frames differ in rgb, mask, depth and boxes, so a buffer taken from another slot changes the answer.
The failed calls of test 5 are argument refusals made before any launch.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import frame_cases as FC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_guard as TG  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- engines, inputs, references ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(state_dict):
    """kind -> engine: one f16 PoseEngine of 4 crops of 64 x 64 and one guard over the same geometry, shared by the module"""
    from flope_amd.engine import PoseEngine
    eng = PoseEngine(FC.CROP, FC.CROP, FC.ENGINE_BATCH, "f16")
    eng.load_state_dict(state_dict)
    g = TG._guard(state_dict, FC.CROP, FC.CROP, FC.ENGINE_BATCH)
    yield {"plain": eng, "guard": g}
    _ALONE.clear()
    g.close()
    eng.close()


_INPUTS, _ALONE = {}, {}


def _inputs(name):
    """(det, count, frame, mask, depth) of a frame on the device, uploaded once"""
    if name not in _INPUTS:
        from sunflower.predictor.fast_pose_predictor import upload_depth
        fr = FC.frame(name)
        dev = torch.device("cuda")
        _INPUTS[name] = (torch.from_numpy(fr.det.copy()).to(dev), torch.tensor([fr.count], dtype=torch.int32, device=dev),
                         torch.from_numpy(fr.rgb.copy()).to(dev), torch.from_numpy(fr.mask.copy()).to(dev), upload_depth(fr.depth.copy(), dev))
    return _INPUTS[name]


def _handle(engine, slots=FC.SLOTS):
    from flope_amd.frame import FramePoses
    return FramePoses(engine, FC.FH, FC.FW, FC.MAX_BOXES, slots)


def _alone(engine, name):
    """to_poses of the frame alone on a fresh one-slot handle over `engine` (at the guard's current threshold), computed once"""
    key = (id(engine), getattr(engine, "gap_min", None), name)
    if key not in _ALONE:
        ctx = _handle(engine, 1)
        _ALONE[key] = ctx.to_poses(*_inputs(name), FC.K, depth_div=FC.DEPTH_DIV, near=FC.NEAR, far=FC.FAR)
        ctx.close()
    return _ALONE[key]


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype
                                         and a.tobytes() == b.tobytes())


def _select(ctx, slot, name):
    det, count = _inputs(name)[:2]
    ctx.select(slot, det, count)


def _enqueue(ctx, slot, name, **kw):
    return ctx.enqueue(slot, *_inputs(name)[2:], FC.K, **{"depth_div": FC.DEPTH_DIV, "near": FC.NEAR, "far": FC.FAR, **kw})


def _run(ctx, slot, name):
    _select(ctx, slot, name)
    n = _enqueue(ctx, slot, name)
    return n, ctx.finish(slot)


def _rows(name):
    """(boxes in frame, rows with reliable depth) the oracle promises for the frame"""
    good, _, cnt, _ = FC.frame_reference(FC.frame(name))
    return len(good), int((cnt >= FC.MIN_COUNT).sum())


def test_the_references_are_what_the_cases_promise(engines):
    """the fresh-handle poses every other test compares with: row counts from the oracle, `None` where it says so, F0 and F1
    different in every row, and the guard's two thresholds giving different bits (so that the comparisons can tell them apart)"""
    g = engines["guard"]
    for kind, gap_min in (("plain", None), ("guard", 1e9), ("guard", -1.0)):
        if gap_min is not None:
            g.gap_min = gap_min
        want = {n: _alone(engines[kind], n) for n in FC.FRAME_NAMES if n != "F4"}
        for n, w in want.items():
            rel = _rows(n)[1]
            assert (w is None) == (rel == 0) and (w is None or (w.shape == (rel, 4, 4) and w.dtype == np.float64 and np.isfinite(w).all())), n
        assert all(want[n] is None for n in ("F2", "F3", "F5", "F6")) and want["F0"].shape[0] == 4 and want["F1"].shape[0] == 5
        for a in want["F0"]:
            for b in want["F1"]:
                assert not np.array_equal(a[:3, :3], b[:3, :3]) and not np.array_equal(a[:3, 3], b[:3, 3])
    g.gap_min = 1e9
    exact = _alone(g, "F0")
    g.gap_min = -1.0
    assert _same(_alone(g, "F0"), _alone(engines["plain"], "F0")) and not _same(exact, _alone(g, "F0"))


# ---- 1. selection ------------------------------------------------------------------------------------------------------------------------------
def test_selection_integer_for_integer(engines):
    """every selection row through select + read_boxes at counts 0, 1, 63, 64, 65, 130, a count above the table, a negative count, a
    handle of 12 boxes under 65 rows, and the 32767-wide frame on a handle of its own"""
    from flope_amd.frame import FramePoses
    eng = engines["plain"]
    handles = {}
    for name in FC.SEL_NAMES:
        c = FC.selection_case(name)
        key = (c.H, c.W, c.cap)
        if key not in handles:
            handles[key] = FramePoses(eng, c.H, c.W, c.cap, 2)
        ctx = handles[key]
        mem = torch.from_numpy(c.det.copy()).cuda()                       # the table and the rows the test owns behind it
        det = mem[:c.max_det]
        assert det.data_ptr() == mem.data_ptr() and det.is_contiguous()
        count = torch.tensor([c.count], dtype=torch.int32, device="cuda")
        for slot in (1, 0):
            ctx.select(slot, det, count)
        for slot in (0, 1):
            good, sq = ctx.read_boxes(slot)
            fails = FC.check_selection(c, good, sq)
            assert not fails, fails[:8]
        total, good_ref, _ = FC.selection_reference(c)
        print(f"{name}: {total} in frame, {len(good_ref)} kept")
    assert len(handles) == 3
    for ctx in handles.values():
        ctx.close()


# ---- 2. capacity -------------------------------------------------------------------------------------------------------------------------------
def test_one_box_more_than_the_handle_holds(engines):
    eng = engines["plain"]
    ctx = _handle(eng)
    good_ref, sq_ref, _, _ = FC.frame_reference(FC.frame("F4"))
    assert len(good_ref) == FC.MAX_BOXES + 1
    _select(ctx, 1, "F4")
    good, sq = ctx.read_boxes(1)
    assert np.array_equal(good, good_ref[:FC.MAX_BOXES]) and np.array_equal(sq, sq_ref[:FC.MAX_BOXES])      # the first 12, in detection order
    with pytest.raises(RuntimeError, match=r"more in-frame boxes than max_boxes \(13\)"):
        _enqueue(ctx, 1, "F4")
    with pytest.raises(RuntimeError, match="nothing enqueued"):
        ctx.finish(1)
    n, got = _run(ctx, 1, "F0")
    assert n == 5 and _same(got, _alone(eng, "F0"))
    with pytest.raises(RuntimeError, match=r"\(13\)"):                       # the same through the one-call form, on slot 0
        ctx.to_poses(*_inputs("F4"), FC.K)
    assert _same(ctx.to_poses(*_inputs("F0"), FC.K), _alone(eng, "F0"))
    ctx.close()


# ---- 3. slots ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,gap_min", [("plain", None), ("guard", 1e9), ("guard", -1.0)], ids=["plain", "guard_all", "guard_none"])
def test_three_different_frames_in_flight(engines, kind, gap_min):
    engine = engines[kind]
    if gap_min is not None:
        engine.gap_min = gap_min
    names = ["F0", "F1", "F3"]
    want = {n: _alone(engine, n) for n in names}
    assert want["F0"] is not None and want["F1"] is not None and want["F3"] is None
    ctx = _handle(engine)
    for turn in range(2):                                                    # the second walk: every frame one slot on
        in_slot = {(s + turn) % 3: names[s] for s in range(3)}
        for s in (0, 1, 2):
            _select(ctx, s, in_slot[s])
        for s in (2, 0, 1):
            assert _enqueue(ctx, s, in_slot[s]) == _rows(in_slot[s])[0]
        for s in (1, 2, 0):
            got = ctx.finish(s)
            assert _same(got, want[in_slot[s]]), (kind, gap_min, turn, s, in_slot[s])
        if kind == "guard":                                                  # F1's last forward held three crops, F0's one
            s1 = [s for s in in_slot if in_slot[s] == "F1"][0]
            assert len(ctx.read_gaps(s1)) == 7 and engine.read_selection(s1) == (list(range(3)) if gap_min > 0 else [])
    ctx.close()


# ---- 4. the host path --------------------------------------------------------------------------------------------------------------------------
class _EngineNet:
    """just enough of a PoseResNet for poses_from_detections to run its crops through the handle's own engine, in the handle's own
    chunks (sunflower.models.posenet.PoseResNet would build an engine of its own batch size: another summation order)"""
    compute_dtype = "f16"

    def __init__(self, eng):
        self.eng = eng

    def predict_rotations(self, crops):
        R = [self.eng.forward(crops[o:o + self.eng.max_batch], want_r9=False, want_R=True)[1] for o in range(0, crops.shape[0], self.eng.max_batch)]
        return None, torch.cat(R)


def test_to_poses_is_the_host_path_bit_for_bit(engines):
    """the contract of test_frame_to_poses_is_the_host_path_bit_for_bit on frames with an inverted and a zero-area box (kept by the
    selection, empty in the depth lift, an all-zero or a real crop, dropped for unreliable depth), with nothing in frame, with nothing
    reliable and with no detection at all"""
    from sunflower.predictor.fast_pose_predictor import poses_from_detections
    eng = engines["plain"]
    ctx = _handle(eng, 1)
    for name in ("F0", "F1", "F2", "F3", "F5"):
        fr = FC.frame(name)
        got = ctx.to_poses(*_inputs(name), FC.K, depth_div=FC.DEPTH_DIV, near=FC.NEAR, far=FC.FAR)
        ref = poses_from_detections(_EngineNet(eng), fr.rgb.copy(), fr.depth.copy(), FC.frame_boxes_int16(fr), fr.mask.copy(), FC.K, depth_div=FC.DEPTH_DIV,
                                    crop_size=FC.CROP, near=FC.NEAR, far=FC.FAR, device="cuda")
        assert (got is None) == (ref is None) == (_rows(name)[1] == 0), name
        assert _same(got, ref), name
        assert _same(got, _alone(eng, name)), name
    ctx.close()


# ---- 5. failed calls leave the slot idle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "guard"])
def test_a_refused_enqueue_leaves_the_slot_idle(engines, kind):
    """Against the parent of the commit that added this test, the plain handle's finish() after the refused enqueue did not raise:
    it returned rows of the frame the slot had finished before."""
    from flope_amd.engine import _stream_ptr
    engine = engines[kind]
    if kind == "guard":
        engine.gap_min = 1e9
    want0, want1 = _alone(engine, "F0"), _alone(engine, "F1")
    ctx = _handle(engine)
    lib = ctx.lib

    def refused_by_ctypes():
        frame_d, mask_d, depth_d = _inputs("F1")[2:]
        k4 = (C.c_float * 4)(float(FC.K[0][0]), float(FC.K[1][1]), float(FC.K[0][2]), float(FC.K[1][2]))
        rc = lib.flope_frame_enqueue(ctx.handle, 0, frame_d.data_ptr(), mask_d.data_ptr(), depth_d.data_ptr(), 7, FC.DEPTH_DIV, k4, FC.NEAR, FC.FAR,
                                     _stream_ptr(ctx.device))
        assert rc < 0 and b"depth" in lib.flope_frame_last_error(ctx.handle), rc

    def refused_by_python():
        with pytest.raises(RuntimeError, match="depth"):
            _enqueue(ctx, 0, "F1", depth_div=0.0)

    for refuse in (refused_by_python, refused_by_ctypes):
        n, got = _run(ctx, 0, "F0")
        assert n == 5 and _same(got, want0)
        _select(ctx, 0, "F1")
        refuse()
        with pytest.raises(RuntimeError, match="nothing enqueued"):         # the call-order error: no rows of any frame
            ctx.finish(0)
        if kind == "guard":                                                  # the guard slot is not armed either
            assert lib.flope_guard_repair(engine.guard_handle, 0, None) == -3
        with pytest.raises(RuntimeError, match="select"):
            _enqueue(ctx, 0, "F1")
        n, got = _run(ctx, 0, "F1")                                          # select is accepted, and the frame is F1's own bits
        assert n == 7 and _same(got, want1)
    # the same refusal through the one-call form
    with pytest.raises(RuntimeError, match="depth"):
        ctx.to_poses(*_inputs("F1"), FC.K, depth_div=-1.0)
    with pytest.raises(RuntimeError, match="nothing enqueued"):
        ctx.finish(0)
    assert _same(ctx.to_poses(*_inputs("F0"), FC.K), want0)
    ctx.close()


# ---- 6. other order and buffer errors --------------------------------------------------------------------------------------------------------------
def test_call_order_and_small_buffers(engines):
    eng = engines["plain"]
    ctx = _handle(eng)
    lib = ctx.lib
    with pytest.raises(RuntimeError, match="nothing selected"):
        ctx.read_boxes(0)
    with pytest.raises(RuntimeError, match="select"):                        # on a fresh handle
        _enqueue(ctx, 0, "F0")
    with pytest.raises(RuntimeError, match="nothing enqueued"):
        ctx.finish(0)
    # selecting twice keeps the second selection
    _select(ctx, 0, "F0")
    _select(ctx, 0, "F1")
    good, sq = ctx.read_boxes(0)
    good_ref, sq_ref, _, _ = FC.frame_reference(FC.frame("F1"))
    assert np.array_equal(good, good_ref) and np.array_equal(sq, sq_ref)
    assert _enqueue(ctx, 0, "F1") == 7
    with pytest.raises(RuntimeError, match="unfinished frame"):              # and a slot that holds a frame refuses the next select
        _select(ctx, 0, "F0")
    assert _same(ctx.finish(0), _alone(eng, "F1"))
    with pytest.raises(RuntimeError, match="select"):                        # after a finished frame as well
        _enqueue(ctx, 0, "F1")
    # a result buffer smaller than the reliable rows: FLOPE_EINVAL, and the slot is idle and usable afterwards
    _select(ctx, 0, "F0")
    assert _enqueue(ctx, 0, "F0") == 5
    out = np.full((FC.MAX_BOXES, 4, 4), -1.0)
    assert lib.flope_frame_finish(ctx.handle, 0, out.ctypes.data, 2) == -1 and b"poses_out too small" in lib.flope_frame_last_error(ctx.handle)
    assert (out[2:] == -1.0).all()
    with pytest.raises(RuntimeError, match="nothing enqueued"):
        ctx.finish(0)
    n, got = _run(ctx, 0, "F0")
    assert n == 5 and _same(got, _alone(eng, "F0"))
    for bad in (-1, FC.SLOTS):
        with pytest.raises(RuntimeError, match="bad slot"):
            ctx.finish(bad)
    ctx.close()
