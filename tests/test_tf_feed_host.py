"""The feed rule of a device-positioned encoder stream without a device (flope_amd/csrc/tf_stream_feed.h, which
tf_stream_feed_kernel calls per thread, through tests/host_harness/harness_tf_feed.cpp).  Cases and the brute-force
statement of the rule: tests/track_stream_cases.py.

  1. the codes of include/flope_amd.h, the track an association entry names;
  2. the host compile against the brute-force rule: the hand cases, the scenario, random associations -- in ascending and in
     descending row order, which must agree (the rule needs no order);
  3. copies broken the way the kernel can break are noticed by the hand cases and by the scenario;
  4. the scenario keeps what it promises: every decision 1 mm from its threshold, the oracle's association, the events it contains;
  5. the token row and track_measure through the harness;
  6. the rule once more as a stand-alone program under -fsanitize=address,undefined (nothing is loaded into Python under a sanitizer);
  7. the new entry points are declared, bound and exported; the Python surface that needs no device.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import track_cases as TC
import track_stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    return SC.load_harness()


# ---- 1. codes and encoding ---------------------------------------------------------------------------------------------------------------
def test_codes_are_distinct_negative_and_the_headers(H):
    codes = np.zeros(5, dtype=np.int32)
    assert H.tf_feed_codes(codes.ctypes.data) == 0                  # (0: the header's skipped value and dimension are track_math.h's)
    assert codes.tolist() == [SC.SKIPPED, SC.OVERFLOW, SC.RANGE, SC.DUPLICATE, SC.FULL]
    assert len(set(codes.tolist())) == 5 and (codes < 0).all()
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    for name, v in zip(("SKIPPED", "OVERFLOW", "RANGE", "DUPLICATE", "FULL"), codes.tolist()):
        assert re.search(rf"#define FLOPE_TF_FEED_{name}\s+\({v}\)", header), name
    from flope_amd import _lib
    assert (_lib.TF_FEED_SKIPPED, _lib.TF_FEED_OVERFLOW, _lib.TF_FEED_RANGE, _lib.TF_FEED_DUPLICATE, _lib.TF_FEED_FULL) == tuple(codes.tolist())


def test_the_track_an_entry_names(H):
    for a, t in ((0, 0), (5, 5), (-1, 0), (-2, 1), (-7, 6), (SC.INT_MAX, SC.INT_MAX), (-SC.INT_MAX, SC.INT_MAX - 1)):
        assert H.tf_feed_h_track(a) == t == SC.track_of(a)


# ---- 2. the host compile against brute force ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(H, case):
    name, assoc, overflow, tracks, pos = case
    want = SC.feed_rule(assoc, overflow, tracks, pos)
    for descending in (0, 1):
        assert SC.same(SC.host_walk(H, assoc, overflow, tracks, pos, descending), want), (name, descending)


def test_what_the_hand_cases_promise():
    got = {c[0]: SC.feed_rule(*c[1:]) for c in SC.hand_cases()}
    who, where, after = got["duplicate_rows_0_1"]
    assert who.tolist() == [2, SC.DUPLICATE, 1] and where.tolist() == [7, 0, 0] and after == [3, 1, 8, 1]
    who, where, after = got["duplicate_rows_0_255"]
    assert who[0] == 5 and who[255] == SC.DUPLICATE and (who[1:255] == SC.SKIPPED).all() and after[5] == 10
    assert got["opened_then_matched"][0].tolist() == [3, SC.DUPLICATE, 0] and got["matched_then_opened"][0].tolist() == [3, SC.DUPLICATE]
    assert got["opened_track_1_is_not_track_2"][0].tolist() == [1, 2, SC.DUPLICATE]
    who, where, after = got["track_at_and_above_tracks"]
    assert who.tolist() == [3] + [SC.RANGE] * 5 and where.tolist() == [2, 0, 0, 0, 0, 0] and after == [0, 0, 0, 3]
    assert got["skipped_row"][0].tolist() == [SC.SKIPPED, 0, SC.SKIPPED, 1]
    who, where, after = got["overflow_flag"]
    assert who.tolist() == [SC.OVERFLOW] * 4 and where.tolist() == [0] * 4 and after == [1, 2, 3, 4]
    who, where, after = got["position_int_max_minus_1"]
    assert who.tolist() == [0, 1] and where.tolist() == [SC.INT_MAX - 1, 0] and after == [SC.INT_MAX, 1]
    who, where, after = got["position_int_max"]
    assert who.tolist() == [SC.FULL, 1, SC.DUPLICATE] and where.tolist() == [0, SC.INT_MAX - 1, 0] and after == [SC.INT_MAX, SC.INT_MAX]


def test_random_associations(H):
    rng = np.random.default_rng(4601)
    seen = set()
    for _ in range(400):
        assoc, overflow, tracks, pos = SC.random_case(rng)
        want = SC.feed_rule(assoc, overflow, tracks, pos)
        seen |= set(int(c) for c in want[0] if c < 0)
        for descending in (0, 1):
            assert SC.same(SC.host_walk(H, assoc, overflow, tracks, pos, descending), want)
        for m in range(len(assoc)):                                   # one row's decision reads nothing it may not
            a, p = np.array(assoc, dtype=np.int32), np.array(pos, dtype=np.int32)
            assert H.tf_feed_h_decide(a.ctypes.data, m, overflow, tracks, p.ctypes.data) == want[0][m]
    assert seen == {SC.SKIPPED, SC.OVERFLOW, SC.RANGE, SC.DUPLICATE, SC.FULL}


def test_the_scenario_through_the_host_compile(H):
    pos = [0] * SC.STREAM_TRACKS
    for a in SC.scenario_assoc():
        want = SC.feed_rule(a, 0, SC.STREAM_TRACKS, pos)
        for descending in (0, 1):
            assert SC.same(SC.host_walk(H, a, 0, SC.STREAM_TRACKS, pos, descending), want)
        pos = want[2]
    assert pos == SC.scenario_feed()[1]


# ---- 3. broken copies --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("broken,names", [("last_wins", ("duplicate_rows_0_1", "duplicate_rows_0_255", "opened_then_matched")),
                                          ("dup_advances", ("duplicate_rows_0_1", "duplicate_rows_0_255", "matched_then_opened")),
                                          ("opened_neg", ("opened_then_matched", "opened_track_1_is_not_track_2", "skipped_row")),
                                          ("full_fed", ("position_int_max",))])
def test_broken_copies_are_noticed(H, broken, names):
    """the last duplicate wins; a duplicate still advances the position; the opened encoding read as -a; a full track still fed"""
    cases = {c[0]: c[1:] for c in SC.hand_cases()}
    for name in names:
        assoc, overflow, tracks, pos = cases[name]
        assert not SC.same(SC.host_walk(H, assoc, overflow, tracks, pos, 0, SC.BROKEN[broken]), SC.feed_rule(assoc, overflow, tracks, pos)), (broken, name)
    if broken == "full_fed":
        return
    pos, noticed = [0] * SC.STREAM_TRACKS, 0                          # the scenario notices the other three too
    for a in SC.scenario_assoc():
        want = SC.feed_rule(a, 0, SC.STREAM_TRACKS, pos)
        noticed += not SC.same(SC.host_walk(H, a, 0, SC.STREAM_TRACKS, pos, 0, SC.BROKEN[broken]), want)
        pos = want[2]
    assert noticed >= 1, broken


# ---- 4. the scenario -----------------------------------------------------------------------------------------------------------------------
def test_scenario_margins_and_oracle():
    case = SC.scenario()
    T = TC.load_harness()
    gate, gap = TC.margins(T, case)
    print(f"gate margin {gate * 1e3:.2f} mm, gap {gap * 1e3:.2f} mm")
    assert gate >= 1e-3 - 1e-12 and gap >= 1e-3 - 1e-12, (gate, gap)
    assert len(case.frames) == 8 and max(len(f.poses) for f in case.frames) == 6
    trace = TC.run_case(case, TC.HostWalk(T, case.max_tracks, case.max_meas, lanes=64))
    fails = TC.check_case(case, trace)
    assert not fails, fails[:4]
    # what the rows were built to be: row -> track as SC.ROWS says, a track's first appearance opens it
    opened = set()
    for rows, a in zip(SC.ROWS, SC.scenario_assoc()):
        start = set(opened)
        for t, v in zip(rows, a):
            if t is None:
                assert v == SC.SKIPPED_ASSOC
            else:
                assert v == (t if t in start else -1 - t)
                opened.add(t)
    assert len(opened) == SC.MAX_TRACKS


def test_scenario_contains_what_the_gpu_test_needs():
    feed, pos = SC.scenario_feed()
    codes = [set(int(c) for c in who if c < 0) for who, _ in feed]
    assert SC.SKIPPED in codes[3] and SC.DUPLICATE in codes[2] and SC.DUPLICATE in codes[7] and SC.RANGE in codes[5] and SC.RANGE in codes[6]
    first = {}
    for fi, (who, _) in enumerate(feed):
        for t in who[who >= 0]:
            first.setdefault(int(t), fi)
    assert len(set(first.values())) >= 3                              # tracks opened in different frames
    held = [[fi for fi, (who, _) in enumerate(feed) if t in who.tolist()] for t in range(SC.STREAM_TRACKS)]
    assert any(b - a == 4 for a, b in zip(held[2], held[2][1:]))      # track 2 is absent for three frames
    assert len(set(pos)) >= 3 and pos == [len(h) for h in held]       # positions diverge
    # the ring wraps and comes round at more than one phase: tokens behind the first lap land on more than one row of a ring of 4 and of 6
    for cap in SC.CAPACITIES:
        assert max(pos) > cap
        slots = {int(p) % cap for who, where in feed for t, p in zip(who, where) if t >= 0 and p >= cap}
        assert len(slots) >= 2, (cap, slots)
    assert max(pos) >= SC.WINDOW + 2                                  # the window slides: a token no longer sees the track's first


# ---- 5. tokens ---------------------------------------------------------------------------------------------------------------------------
def test_token_rows_and_track_measure(H):
    T = TC.load_harness()
    fr = SC.scenario().frames[0]
    z = SC.measurement(H, fr.poses[1], fr.cam)
    assert z.tobytes() == TC.measure(T, fr.poses[1], fr.cam).tobytes()          # the harness exposes track_math.h's own function
    assert abs(np.linalg.norm(z[3:]) - 1) < 1e-15
    for dim in (7, 9, 12):
        row = SC.token(H, z, dim)
        assert row[:7].tobytes() == z.astype(np.float32).tobytes() and (row[7:] == 0).all() and row.shape == (dim,)
        assert (SC.token(H, None, dim) == 0).all()
    want = SC.expected_tokens(H, fr, np.array([0, SC.DUPLICATE, 2]), 9)
    assert want[0, :7].tobytes() == SC.measurement(H, fr.poses[0], fr.cam).astype(np.float32).tobytes() and (want[1] == 0).all() and (want[:, 7:] == 0).all()


# ---- 6. the same under AddressSanitizer + UBSan, as a program of its own ------------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """the rule once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "tf_feed_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTF_FEED_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_harness", "harness_tf_feed.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and " frames, 0 failures" in r.stdout


# ---- 7. the surface ----------------------------------------------------------------------------------------------------------------------
NEW = ("flope_tf_stream_open_device", "flope_tf_stream_step_assoc", "flope_tf_stream_step_tracker", "flope_tf_stream_reset_device",
       "flope_tf_stream_read_positions", "flope_tf_stream_read_feed", "flope_tf_stream_read_tokens", "flope_track_device_view")


def test_new_entry_points_are_declared_bound_and_exported():
    from flope_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "flope_amd.h")).read()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    import ctypes as C
    assert C.sizeof(_lib.TrackView) == 5 * 8 + 4 * 4 + 8


def test_python_surface_without_a_device():
    import inspect
    from flope_amd.tf_encoder import TransformerEncoder, TransformerEncoderStream
    from flope_amd.track import DeviceTracker
    from sunflower.predictor.flower_model import FlowerModel
    sig = inspect.signature(TransformerEncoder.open_stream).parameters
    assert sig["positions"].default == "host" and sig["max_rows"].default is None
    for name in ("step_assoc", "step_tracker", "last_feed", "last_tokens"):
        assert callable(getattr(TransformerEncoderStream, name))
    assert isinstance(DeviceTracker.last_n, property)
    with pytest.raises(ValueError, match="tracker='device'"):
        FlowerModel(track_stream=object())
    fm = FlowerModel()
    assert fm.track_stream is None and fm.track_rows is None and fm.track_feed is None
