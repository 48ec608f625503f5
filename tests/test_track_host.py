"""The device tracker's arithmetic and order without a device (flope_amd/csrc/track_math.h, which track.hip's kernels call, and a
scalar walk of a whole update in tests/host_harness/harness_track.cpp).  Cases, oracle and checker:
tests/track_cases.py; the bound and the exact evaluation: tests/track_bound.py.

  1. the quaternion rule against scipy over 20 000 random rotations, float64-orthogonal and rounded through float32 -- the second
     figure is the tolerance tests/test_gpu_track.py uses against the host FlowerModel;
  2. measurement and filter update against mpmath within the derived bound;
  3. every case through the walk at 1 and 64 lanes: integers equal to oracle/fusion_ref.py's, means within the bound, sentinel words
     untouched, every decision 1 mm from its threshold;
  4. copies broken the way the kernels can break fall outside the bound or change the association;
  5. float32 rows against the same rows widened give equal bits; overflow; the walk's refusals;
  6. the walk once more as a stand-alone program under -fsanitize=address,undefined (nothing is loaded into Python under a sanitizer);
  7. FlowerModel's tracker= argument.
"""
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as Rot

import track_bound as TB
import track_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    return TC.load_harness()


# ---- 1. the quaternion rule against scipy ----------------------------------------------------------------------------------------------
def _quats(H, mats):
    out = np.empty((len(mats), 4))
    p = np.zeros((4, 4))
    p[3, 3] = 1
    for i, m in enumerate(mats):
        p[:3, :3] = m
        out[i] = TC.measure(H, p, TC.IDENTITY_CAM)[3:]
    return out


def test_quaternion_rule_against_scipy(H):
    """signs included: the rule and scipy pick the same of q and -q.  float64-orthogonal rotations agree to a few ulp; rounded through
    float32 they differ by what scipy's move onto a rotation changes: SCIPY_F32_DIFF, the measured figure of DESIGN.md 45"""
    R64 = Rot.random(TC.SCIPY_ROTATIONS, random_state=2045).as_matrix()
    d64 = np.abs(_quats(H, R64) - Rot.from_matrix(R64).as_quat()).max()
    R32 = R64.astype(np.float32).astype(np.float64)
    d32 = np.abs(_quats(H, R32) - Rot.from_matrix(R32).as_quat()).max()
    print(f"track_measure vs scipy over {TC.SCIPY_ROTATIONS} rotations: float64 {d64:.3g}, through float32 {d32:.3g}")
    assert d64 <= 2 * TB.E_Q                      # each side within the derived bound of the exact quaternion
    assert d32 <= TC.SCIPY_F32_DIFF
    assert d32 >= 1e-9                            # (the float32 figure is a real difference of method, not rounding noise)


def test_candidate_order_and_match_test(H):
    """track_better is np.argmin's order on (distance, index) pairs, whatever order they are met in; a NaN never wins; the match test
    is d < th, and no anchor is no match"""
    inf, nan = float("inf"), float("nan")
    assert H.track_dim() == 7 and H.track_skipped() == TC.SKIPPED
    assert H.track_h_better(0.25, 9, 0.5, 1) and not H.track_h_better(0.5, 1, 0.25, 9)
    assert H.track_h_better(0.25, 3, 0.25, 67) and not H.track_h_better(0.25, 67, 0.25, 3) and not H.track_h_better(0.25, 3, 0.25, 3)
    assert H.track_h_better(0.25, 0, inf, -1) and not H.track_h_better(nan, 0, inf, -1) and not H.track_h_better(nan, 0, 0.25, 5)
    rng = np.random.default_rng(3)
    for _ in range(200):
        d = rng.integers(0, 4, 40) * 0.125                       # many exact ties
        order = rng.permutation(40)
        bd, bi = inf, -1
        for i in order:
            if H.track_h_better(d[i], int(i), bd, bi):
                bd, bi = d[i], int(i)
        assert bi == int(np.argmin(d))
    assert H.track_h_match(0.049, 0, 0.05) and not H.track_h_match(0.05, 0, 0.05) and not H.track_h_match(0.051, 0, 0.05)
    assert not H.track_h_match(inf, -1, 0.05) and not H.track_h_match(0.0, -1, 0.05) and not H.track_h_match(nan, 0, 0.05)


# ---- 2. one measurement, one update ----------------------------------------------------------------------------------------------------
def test_measurement_and_update_within_the_bound_of_mpmath(H):
    rng = np.random.default_rng(7)
    worst_t = worst_q = worst_x = 0.0
    for _ in range(200):
        cam = np.concatenate([rng.uniform(-2, 2, 3), Rot.random(random_state=int(rng.integers(1 << 30))).as_quat()])
        p = TC.pose(rng.uniform(-2, 2, 3), Rot.random(random_state=int(rng.integers(1 << 30))).as_rotvec())
        cm = TC.cam_matrix(cam)
        z = TC.measure(H, p, cam)
        zm, margin = TB.mp_measure(p, cm)
        if margin < 1e-9:
            continue
        S = float(np.linalg.norm(p[:3, 3]) + np.abs(cm[:3, 3]).max())
        e_t, e_q = TB.measurement_bound(S)
        err = np.array([abs(float(zm[c] - float(z[c]))) for c in range(7)])
        worst_t, worst_q = max(worst_t, err[:3].max() / e_t), max(worst_q, err[3:].max() / e_q)
        # one update of a track opened on z by a second measurement nearby
        p2 = p.copy()
        p2[:3, 3] += rng.uniform(-0.02, 0.02, 3)
        p2[:3, :3] = p[:3, :3] @ Rot.from_rotvec(rng.normal(0, 0.05, 3)).as_matrix()
        z2, (zm2, _) = TC.measure(H, p2, cam), TB.mp_measure(p2, cm)
        x, pv = z.copy(), np.array([TC.P0])
        H.track_h_update(x.ctypes.data, pv.ctypes.data, z2.ctypes.data, TC.Q, TC.R)
        xm, pm, nu = TB.mp_track([zm, zm2], TC.Q, TC.R, TC.P0)
        bt, bq, brho = TB.track_bound(1, S, TC.TH, TC.Q, TC.R, TC.P0, nu)
        errx = np.array([abs(float(xm[c] - float(x[c]))) for c in range(7)])
        worst_x = max(worst_x, errx[:3].max() / bt[1], errx[3:].max() / bq[1])
        assert abs(float((pm - float(pv[0])) / pm)) <= brho[1]
    print(f"error / bound: translation {worst_t:.3f}, quaternion {worst_q:.3f}, after one update {worst_x:.3f}")
    assert worst_t <= 1 and worst_q <= 1 and worst_x <= 1


def test_the_walk_equals_the_oracles_scalar_track_on_its_own_measurements(H):
    """same order of operations as oracle/fusion_ref.py's scalar_track: fed with the walk's own measurements the means agree to the
    last bit, which pins the order of track_filter_update"""
    from oracle import fusion_ref as F
    case = TC.cases()["long_200"]
    w = TC.HostWalk(H, case.max_tracks, case.max_meas)
    trace = TC.run_case(case, w, case.frames[:40])
    zs = [list(TC.measure(H, fr.poses[0], fr.cam)) for fr in case.frames[:40]]
    x, p = F.scalar_track(zs, TC.Q, TC.R, TC.P0)
    assert trace.means[0].tolist() == x and float(trace.p[0]) == p


# ---- 3. every case ---------------------------------------------------------------------------------------------------------------------
def test_every_case_is_named():
    assert tuple(TC.cases()) == TC.CASE_NAMES


@pytest.mark.parametrize("name", TC.CASE_NAMES)
def test_case_on_the_host_walk(H, name):
    case = TC.cases()[name]
    gate, gap = TC.margins(H, case)
    assert gate >= 1e-3 - 1e-12 and gap >= 1e-3 - 1e-12, (gate, gap)
    traces = []
    for lanes in (1, 64):
        w = TC.HostWalk(H, case.max_tracks, case.max_meas, lanes=lanes)
        traces.append(TC.run_case(case, w))
        fails = TC.check_case(case, traces[-1])
        assert not fails, fails[:6]
        assert w.sentinels_changed() == 0 and not w.overflowed
    ratio, err, ratio_p = TC.worst_ratio(case, traces[0])
    print(f"{name}: error / bound {ratio:.3f} (error {err:.3g}), p {ratio_p:.3f}; gate margin {gate * 1e3:.2f} mm, gap {gap * 1e3:.2f} mm")
    a, b = traces
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])) and all(np.array_equal(x, y) for x, y in zip(a.assoc, b.assoc))


def test_what_the_cases_promise(H):
    c = TC.cases()
    one = TC.run_case(c["first_frame"], TC.HostWalk(H, 8, 8))
    assert [a.tolist() for a in one.assoc] == [[-1, -2, -3, -4, -5]]
    # under an identity camera pose the anchors' translations equal the input bit for bit
    assert one.anchors[:, :3].tobytes() == np.ascontiguousarray(c["first_frame"].frames[0].poses[:, :3, 3]).tobytes()
    assert TC.run_case(c["gate_49_51"], TC.HostWalk(H, 8, 8)).assoc[1].tolist() == [0, -2]
    assert TC.run_case(c["two_on_one"], TC.HostWalk(H, 8, 8)).assoc[1].tolist() == [0, 1, 0]
    assert [a.tolist() for a in TC.run_case(c["two_new_close"], TC.HostWalk(H, 8, 8)).assoc[1:]] == [[-2, -3], [2, 1]]
    assert TC.run_case(c["tie_lower_index"], TC.HostWalk(H, 80, 72, lanes=64)).assoc[1].tolist() == [0, 3, 5]
    assert [a.tolist() for a in TC.run_case(c["rel_skipped"], TC.HostWalk(H, 8, 8)).assoc[1:]] == [[0, TC.SKIPPED, -3, TC.SKIPPED, 1], [TC.SKIPPED]]
    nz = TC.run_case(c["n_zero"], TC.HostWalk(H, 8, 8))
    assert [a.tolist() for a in nz.assoc] == [[], [-1, -2], [], [0]] and nz.hits.tolist() == [2, 1]
    long = TC.run_case(c["long_200"], TC.HostWalk(H, 4, 4))
    assert long.hits.tolist() == [201]
    assert TC.run_case(c["drifted_mean"], TC.HostWalk(H, 4, 4)).hits.tolist() == [8]
    for T, n in TC.ARGMIN_SHAPES:
        tr = TC.run_case(c[f"argmin_T{T}_n{n}"], TC.HostWalk(H, T + n, max(T, n), lanes=64))
        got = tr.assoc[1]
        assert {0, T - 1, 63 % T, 64 % T} <= set(got[got >= 0].tolist()) and (got < 0).sum() == n // 7


# ---- 4. broken copies ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("broken,name", [("reverse", "two_on_one"), ("means", "drifted_mean"), ("visible", "two_new_close"), ("tie_high", "tie_lower_index")])
def test_broken_copies_are_noticed(H, broken, name):
    """updates of one track in reverse measurement order; distances to the filtered means; a new track visible to the rest of its
    frame; the highest index winning a tie"""
    case = TC.cases()[name]
    w = TC.HostWalk(H, case.max_tracks, case.max_meas, lanes=64, broken=TC.BROKEN[broken])
    fails = TC.check_case(case, TC.run_case(case, w))
    print(fails[:3])
    assert fails
    if broken == "reverse":                      # the integers are right; the means leave the bound, and by far more than the bound
        good = TC.run_case(case, TC.HostWalk(H, case.max_tracks, case.max_meas))
        bad = TC.run_case(case, TC.HostWalk(H, case.max_tracks, case.max_meas, broken=1))
        exp = TC.expected(case)
        assert not TC.check_integers(case, bad)
        assert np.abs(good.means[0] - bad.means[0]).max() > 1e6 * max(exp.bound_t[0], exp.bound_q[0])
    else:
        assert TC.check_integers(case, TC.run_case(case, TC.HostWalk(H, case.max_tracks, case.max_meas, broken=TC.BROKEN[broken])))   # at one lane too


# ---- 5. float32 rows, overflow, refusals -----------------------------------------------------------------------------------------------
def test_float32_rows_equal_the_same_rows_widened(H):
    f32, f64 = TC.f32_frames()
    case = TC.cases()["camera_pose"]
    a = TC.run_case(case, TC.HostWalk(H, 8, 8), f32)
    b = TC.run_case(case, TC.HostWalk(H, 8, 8), f64)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])) and len(a.hits) == 4 and a.hits.sum() == 11


def test_overflow_applies_nothing_and_sticks_until_reset(H):
    three, two_more, one_more = TC.overflow_frames()
    w = TC.HostWalk(H, 4, 4)
    assert w.update(*three) == 0 and w.read()[3].tolist() == [1, 1, 1]
    before = [a.copy() for a in (w.anchors, w.means, w.p, w.hits, w.assoc_buf)]
    assert w.update(*two_more) == 0 and w.overflowed and int(w.cnt[0]) == 3
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (w.anchors, w.means, w.p, w.hits, w.assoc_buf))) and w.sentinels_changed() == 0
    assert w.update(*one_more) == 0 and int(w.cnt[0]) == 3           # sticky: nothing is applied
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (w.anchors, w.means, w.p, w.hits, w.assoc_buf)))
    w.reset()
    assert w.update(*three) == 0 and w.update(*one_more) == 0 and not w.overflowed
    assert w.last_association().tolist() == [-4, 1] and w.read()[3].tolist() == [1, 2, 1, 1] and w.sentinels_changed() == 0


def test_the_walk_refuses_what_the_handle_refuses(H):
    w = TC.HostWalk(H, 4, 2)
    three = TC.overflow_frames()[0]
    assert w.update(*three) < 0 and int(w.cnt[0]) == 0 and w.sentinels_changed() == 0      # n = 3 > max_meas = 2


# ---- 6. the same under AddressSanitizer + UBSan, as a program of its own ----------------------------------------------------------------
def test_stand_alone_program_under_sanitizers(tmp_path):
    """the walk once in a stand-alone program of its own (host code only, nothing loaded into python)"""
    exe = str(tmp_path / "track_selfcheck")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DTRACK_MAIN", "-std=c++17",
                           "-I" + os.path.join(ROOT, "flope_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host_harness", "harness_track.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and " updates, 0 failures" in r.stdout


# ---- 7. FlowerModel(tracker=) ------------------------------------------------------------------------------------------------------------
def test_flower_model_tracker_argument():
    from sunflower.predictor.flower_model import FlowerModel
    fm = FlowerModel()
    assert fm.tracker == "host" and fm.state is None and fm.scores is None and fm.kfs == [] and fm.device_tracker is None
    with pytest.raises(ValueError, match="'host' or 'device'"):
        FlowerModel(tracker="gpu")
    with pytest.raises(AttributeError):
        fm.no_such_attribute
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device"):       # there is no quiet fall-back to the host tracker
            FlowerModel(tracker="device")
    else:
        dm = FlowerModel(tracker="device")
        assert dm.state is None and dm.scores is None and dm.filtered_state().shape == (0, 7)
        with pytest.raises(AttributeError, match="tracker='host'"):
            dm.kfs
        dm.device_tracker.close()
