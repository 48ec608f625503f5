"""The CPU half of the frame handle's tests (GPU half: tests/test_gpu_frame_cases.py; cases and checker: tests/frame_cases.py).

1.  The arithmetic (flope_amd/csrc/frame_plan.h through tests/host_harness/harness_frame.cpp): frame_box equals the hand-written
    answers and both Python statements of the reference's loop on every selection row and on all (w, h) in 0..40 x 0..40 at the four
    corners of the frame; the count clamp.
2.  The builder's promises, from the oracle alone (P.select_boxes, depth_stats64): kept counts, reliable counts, the forwards each
    frame runs, F0 and F1 different in every output row, no two frames sharing a buffer.
3.  A numpy emulation of frame_select_kernel (64-row passes, ballot rank = base + popcount below the lane, store under rank < cap
    into one flat [2 * cap][4] buffer, nsel = (min(base, cap), base)) passes every selection case; copies of it broken the way this
    kernel could break each fail on at least one case.  A break that no case catches means a case is missing.
"""
import numpy as np
import pytest

import frame_cases as FC


@pytest.fixture(scope="module")
def plan():
    return FC.load_plan()


# ---- 1. the arithmetic -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,W,H", [(FC.ROWS, FC.SW, FC.SH), (FC.WIDE_ROWS, FC.WW, FC.WH)], ids=["640x480", "32767x16"])
def test_frame_box_equals_the_hand_written_answers_and_both_python_statements(plan, rows, W, H):
    from sunflower.utils.mvg import bb_in_frame, squarify_bb
    from oracle import pipeline_ref as P
    assert plan.frame_det_row() == 8
    det = np.array([r[0] for r in rows], np.float32)
    keep, good, sq = FC.plan_boxes(plan, det, W, H)
    bb16 = det.astype(np.int16)                                           # fast_pose_predictor.py:55-56
    assert np.array_equal(good, bb16.astype(np.int32))
    for i, (row, sq_hand, keep_hand) in enumerate(rows):
        assert sq[i].tolist() == list(sq_hand) and bool(keep[i]) == keep_hand, (row, sq[i].tolist(), bool(keep[i]))
        s_m, s_o = squarify_bb(bb16[i]), P.squarify_bb(bb16[i].astype(np.int64))
        assert list(s_m) == list(s_o) == list(sq_hand), row
        assert bb_in_frame(s_m, (H, W, 3)) == P.bb_in_frame(s_o, (H, W, 3)) == keep_hand, row
    good_ref, sq_ref = FC.host_loop(bb16, H, W)                           # the loops themselves, on the int16 rows
    assert np.array_equal(good[keep], good_ref) and np.array_equal(sq[keep], sq_ref)
    assert keep.any() and not keep.all()


def test_selection_rows_hold_what_they_are_listed_for():
    bb = np.array([r[0] for r in FC.ROWS], np.float32).astype(np.int16).astype(int)
    kept = np.array([r[2] for r in FC.ROWS])
    w, h = bb[:, 2] - bb[:, 0], bb[:, 3] - bb[:, 1]
    sq = np.array([r[1] for r in FC.ROWS])
    assert ((w < 0) & (h > 0) & kept).any() and ((h < 0) & (w > 0) & kept).any() and ((w < 0) & (h < 0) & kept).any()
    assert ((w < 0) & ~kept).any() and ((bb[:, 0] > FC.SW) & kept).any()
    zero = (w == 0) & (h == 0) & kept
    assert (zero & (bb[:, 0] < FC.SW)).any() and (zero & (bb[:, 0] == FC.SW) & (bb[:, 1] < FC.SH)).any() and (zero & (bb[:, 0] == FC.SW) & (bb[:, 1] == FC.SH)).any()
    for wide_first in (True, False):                                      # d odd and even on both axes
        d = np.where((w > h) == wide_first, np.abs(w - h), 0)
        assert ((d > 0) & (d % 2 == 1) & kept & (w > 0) & (h > 0)).any() and ((d > 0) & (d % 2 == 0) & kept & (w > 0) & (h > 0)).any()
    moved = (sq != bb).any(axis=1)
    for col, lim in ((2, FC.SW), (3, FC.SH)):                             # the square touches the far edge exactly / overshoots by one
        assert (moved & (sq[:, col] == lim) & kept).any() and (moved & (sq[:, col] == lim + 1) & ~kept).any()
    for col in (0, 1):
        assert (moved & (sq[:, col] == 0) & kept).any() and (moved & (sq[:, col] == -1) & ~kept).any()
    assert ((w == 1) & (h == 1) & kept).sum() >= 3
    raw = np.array([r[0] for r in FC.ROWS], np.float64)
    assert (raw == -0.5).any() and (raw == -0.999).any() and ((raw == -1.0).any(axis=1) & ~kept).sum() >= 2
    assert np.abs(raw).max() <= 32767 and max(abs(v) for r in FC.WIDE_ROWS for v in r[0]) == 32767
    assert any(r[0][2] == 32767 and r[2] for r in FC.WIDE_ROWS)


@pytest.mark.parametrize("W,H", [(640, 480), (128, 96), (41, 41)])
def test_frame_box_over_all_small_sizes_at_the_four_corners(plan, W, H):
    rows = []
    for cx, cy in ((0, 0), (W, 0), (0, H), (W, H)):                       # the box hangs into the frame from each corner
        for w in range(41):
            for h in range(41):
                x0, y0 = (0 if cx == 0 else W - w), (0 if cy == 0 else H - h)
                rows.append((x0, y0, x0 + w, y0 + h))
    det = np.array(rows, np.float32)
    keep, good, sq = FC.plan_boxes(plan, det, W, H)
    good_ref, sq_ref = FC.host_loop(det.astype(np.int16), H, W)
    assert np.array_equal(good[keep], good_ref) and np.array_equal(sq[keep], sq_ref)
    assert 0 < keep.sum() < len(rows)


def test_count_clamp(plan):
    for count, max_det, want in ((0, 16, 0), (1, 16, 1), (16, 16, 16), (17, 16, 16), (-1, 16, 0), (-3, 16, 0), (2 ** 31 - 1, 300, 300),
                                 (-2 ** 31, 300, 0), (5, 1, 1)):
        assert plan.frame_count_rows(count, max_det) == want


# ---- 2. the builder's promises ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.FRAME_NAMES)
def test_frames_keep_and_lift_what_they_promise(name):
    fr = FC.frame(name)
    good, sq, cnt, mean = FC.frame_reference(fr)
    in_frame, reliable = FC.PROMISED[name]
    rel = cnt[:FC.MAX_BOXES] >= FC.MIN_COUNT
    print(f"{name}: {len(good)} in frame, eroded-valid pixels {cnt.tolist()}")
    assert len(good) == in_frame and int(rel.sum()) == reliable
    assert fr.rgb.shape == (FC.FH, FC.FW, 3) and fr.mask.shape == fr.depth.shape == (FC.FH, FC.FW) and fr.depth.dtype == np.uint16
    assert fr.det.shape == (FC.MAX_DET, 8) and fr.det.dtype == np.float32
    assert ((fr.det[:max(fr.count, 0), :4] % 1) != 0).any() or fr.count <= 0      # fractional coordinates: the cast truncates
    # rows behind the count would be kept if they were read
    extra, _ = FC.host_loop(fr.det[:, :4].astype(np.int16), FC.FH, FC.FW)
    assert len(extra) > in_frame
    # reliable by a margin, unreliable by a margin: not at the threshold of 50
    assert all(c >= 2 * FC.MIN_COUNT or c == 0 for c in cnt.tolist())


def test_frame_shapes_of_the_walk():
    f0, f1, f3, f4 = (FC.frame_reference(FC.frame(n)) for n in ("F0", "F1", "F3", "F4"))
    assert FC.forwards(len(f0[0])) == [4, 1] and FC.forwards(len(f1[0])) == [4, 3] and FC.forwards(len(f3[0])) == [2]
    assert len(f4[0]) == FC.MAX_BOXES + 1
    # F0: the unreliable box is the last one; F1: the inverted and the zero-area box are kept and select nothing in the depth lift
    assert (f0[2] >= FC.MIN_COUNT).tolist() == [True, True, True, True, False]
    good, sq, cnt, _ = f1
    w, h = good[:, 2] - good[:, 0], good[:, 3] - good[:, 1]
    assert (w < 0).sum() == 1 and ((w == 0) & (h == 0)).sum() == 1
    inv = int(np.nonzero(w < 0)[0][0])
    assert sq[inv].tolist() == [45, 10, 55, 20] and cnt[inv] == 0 and cnt[(w == 0) & (h == 0)].tolist() == [0]
    assert (cnt >= FC.MIN_COUNT).tolist() == [True, False, True, False, True, True, True]
    # F2, F5, F6: nothing in frame, for three different reasons
    assert [FC.frame(n).count for n in ("F2", "F5", "F6")] == [3, 0, -3]


def test_no_two_frames_share_a_buffer_and_f0_f1_differ_in_every_output_row():
    frames = [FC.frame(n) for n in FC.FRAME_NAMES]
    for i, a in enumerate(frames):
        for b in frames[i + 1:]:
            assert (a.rgb != b.rgb).mean() > 0.9 and (a.mask != b.mask).mean() > 0.3 and (a.depth != b.depth).mean() > 0.9
            assert a.count != b.count or not np.array_equal(a.det, b.det)
    # an output row is a rotation from the crop and a translation from (box centre, mean depth): no row of F0 shares its square (the
    # crop's source), its box or its depth with a row of F1, and every reliable box of F1 lies deeper than every one of F0
    g0, s0, c0, m0 = FC.frame_reference(frames[0])
    g1, s1, c1, m1 = FC.frame_reference(frames[1])
    r0, r1 = c0 >= FC.MIN_COUNT, c1 >= FC.MIN_COUNT
    for i in np.nonzero(r0)[0]:
        for j in np.nonzero(r1)[0]:
            assert s0[i].tolist() != s1[j].tolist() and g0[i].tolist() != g1[j].tolist() and m0[i] != m1[j]
    assert m0[r0].max() < m1[r1].min()
    for a, b in ((frames[0], frames[1]), (frames[1], frames[3]), (frames[0], frames[3])):
        assert a.depth.max() < b.depth.min() or (a.depth != b.depth).all()


# ---- 3. the emulation and its broken copies ----------------------------------------------------------------------------------------------------
def _box(row, W, H, brk):
    """frame_plan.h's frame_box in Python, with one deliberate defect"""
    v = np.rint(row[:4]) if brk == "round" else np.trunc(row[:4])
    x0, y0, x1, y1 = (int(np.int16(int(t))) for t in v)
    w, h = x1 - x0, y1 - y0
    d = abs(w - h)
    lo, hi = (d + 1) // 2, d // 2
    if brk == "lo_hi":
        lo, hi = hi, lo
    s = [x0, y0, x1, y1]
    if w > h:
        s[1] -= lo; s[3] += hi
    elif h > w:
        s[0] -= lo; s[2] += hi
    out_x = s[2] >= W if brk == "ge_W" else s[2] > W
    out_y = s[3] >= H if brk == "ge_H" else s[3] > H
    return not (s[0] < 0 or s[1] < 0 or out_x or out_y), [x0, y0, x1, y1], s


def emulate(c, brk=None):
    """frame_select_kernel on case c -> (box memory int32 [2 * cap * 4], nsel [2]); `brk` names one deliberate defect"""
    cap = c.cap
    mem = np.full(2 * cap * 4 + 8, FC.SENTINEL, np.int64)                # 8 more: a store one row too far stays inside the array
    n = c.count
    if brk == "neg_count":                                               # the count read as unsigned: a negative one reads the table
        n = n + 2 ** 32 if n < 0 else n
    elif n < 0:
        n = 0
    if brk != "no_max_det":
        n = min(n, c.max_det)
    n = min(n, len(c.det))                                               # (what the test owns behind the table)
    store_cap = cap + 1 if brk == "cap_plus_1" else cap
    base = 0
    for i0 in range(0, n, 64):
        rows = range(i0, min(i0 + 64, n))
        res = [_box(c.det[i], c.W, c.H, brk) for i in rows]
        below = 0
        for keep, good, sq in res:                                       # lanes in order: popcount of the ballot below the lane
            if keep:
                rank = (0 if brk == "no_carry" else base) + below
                if rank < store_cap:
                    mem[rank * 4:rank * 4 + 4] = good
                    at = rank * 4 if brk == "sq_first_table" else cap * 4 + rank * 4
                    mem[at:at + 4] = sq
                below += 1
        base += below
    return mem, (min(base, store_cap), base)


def judge(c, mem, nsel):
    """what flope_frame_read_boxes would return from this memory, through the shared checker; and nothing stored elsewhere"""
    cap = c.cap
    k = nsel[0]
    fails = FC.check_selection(c, mem[:k * 4].reshape(-1, 4), mem[cap * 4:cap * 4 + k * 4].reshape(-1, 4), in_frame=nsel[1])
    k = min(k, cap)
    rest = np.concatenate([mem[k * 4:cap * 4], mem[cap * 4 + k * 4:]])
    if (rest != FC.SENTINEL).any():
        fails.append(f"{c.name}: stores outside the first {k} rows of the two tables")
    return fails


@pytest.mark.parametrize("name", FC.SEL_NAMES)
def test_unbroken_emulation_passes(plan, name):
    c = FC.selection_case(name)
    mem, nsel = emulate(c)
    assert not judge(c, mem, nsel)
    # its arithmetic is the header's
    n = min(max(c.count, 0), c.max_det)
    keep, good, sq = FC.plan_boxes(plan, c.det[:n], c.W, c.H)
    assert [(_box(c.det[i], c.W, c.H, None)) for i in range(n)] == [(bool(keep[i]), good[i].tolist(), sq[i].tolist()) for i in range(n)]
    assert nsel[1] == int(keep.sum())


def test_selection_cases_reach_what_they_are_built_for():
    total = {n: FC.selection_reference(FC.selection_case(n))[0] for n in FC.SEL_NAMES}
    assert total["rows_0"] == 0 and total["count_negative"] == 0
    assert total["rows_64"] < total["rows_65"] or total["rows_65"] < total["rows_130"]      # boxes kept in the second and third pass
    assert total["rows_130"] > total["rows_64"] > 0
    assert total["count_above_table"] == total["rows_130"]                                 # and the rows behind the table are in frame
    c = FC.selection_case("count_above_table")
    assert len(c.det) == c.max_det + FC.SEL_BEHIND and len(FC.host_loop(c.det[c.max_det:, :4].astype(np.int16), c.H, c.W)[0]) == FC.SEL_BEHIND
    assert total["cap_12"] > 12 == FC.selection_case("cap_12").cap
    assert FC.selection_case("wide").W == 32767 and total["wide"] >= 5


BREAKS = ["no_carry", "ge_W", "ge_H", "lo_hi", "round", "cap_plus_1", "no_max_det", "neg_count", "sq_first_table"]


@pytest.mark.parametrize("brk", BREAKS)
def test_broken_emulation_is_caught(brk):
    """neg_count: merely dropping `count < 0 ? 0` changes nothing the kernel does (its loops run `while i0 < n` and store under
    `i < n`, which a negative n never passes), so the break that stands for it is the count read as unsigned."""
    caught = {}
    for name in FC.SEL_NAMES:
        c = FC.selection_case(name)
        fails = judge(c, *emulate(c, brk))
        if fails:
            caught[name] = len(fails)
    print(f"{brk}: caught by {caught}")
    assert caught, f"no case notices the break {brk!r}: a case is missing"


def test_what_each_break_needs():
    """the cases are not interchangeable"""
    for brk, name in (("no_carry", "rows_65"), ("no_carry", "rows_130"), ("cap_plus_1", "cap_12"), ("no_max_det", "count_above_table"),
                      ("neg_count", "count_negative"), ("ge_W", "wide"), ("ge_H", "wide"), ("ge_W", "rows_63"), ("ge_H", "rows_63"),
                      ("lo_hi", "rows_63"), ("round", "rows_63"), ("sq_first_table", "rows_1")):
        c = FC.selection_case(name)
        assert judge(c, *emulate(c, brk)), (brk, name)
    for brk in ("no_carry", "cap_plus_1", "no_max_det", "neg_count"):      # one pass, nothing dropped, the count inside the table
        c = FC.selection_case("rows_63")
        assert not judge(c, *emulate(c, brk)), brk
