"""Cases of the device tracker (flope_amd/csrc/track.hip, flope_amd/track.py) and the checker both halves of its tests share:
tests/test_track_host.py (CPU: flope_amd/csrc/track_math.h and a scalar walk of an update through
tests/host_harness/harness_track.cpp, its broken copies) and tests/test_gpu_track.py (the kernels behind flope_track_update).

A case is a name, the capacity of the state and a list of frames (poses [n,4,4] in the camera frame, the reference's camera
7-vector, rel int32 [n] or None).  A backend -- the host walk here, a DeviceTracker in the GPU test -- takes the frames one by one;
`run_case` records the association after every frame and the state at the end, `check_case` compares them with the oracle:

  integers   oracle.fusion_ref.associate on the host's own poses_to_measurements(pose_cam_to_world(...)) of the reliable rows:
             association, track count and hit counts integer for integer.  Every case keeps each decision at least 1 mm from the
             50 mm gate and 1 mm between the two nearest anchors (`margins` measures it), except the deliberate exact ties, which are
             built from coordinates that are exact in binary.
  means      an mpmath evaluation of the same recursion on the oracle's track membership, within tests/track_bound.py's bound.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import track_bound as TB
from oracle import fusion_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH_MM, Q, R, P0 = 50, 1e-3, 0.1, 1.0
TH = TH_MM / 1000
SKIPPED = -2 ** 31
IDENTITY_CAM = np.array([0, 0, 0, 0, 0, 0, 1.0])
BROKEN = dict(reverse=1, means=2, visible=4, tie_high=8)
# the largest component difference between scipy's Rotation.from_matrix(...).as_quat() and track_measure's quaternion over
# SCIPY_ROTATIONS random rotations rounded through float32 (scipy first moves such a matrix onto a rotation, the rule only
# normalises); tests/test_track_host.py measures it and asserts this figure, DESIGN.md 45 records it.  The host FlowerModel and the
# device tracker may differ by SCIPY_MARGIN times as much on frames of float32 poses: a sample maximum is not a supremum.
SCIPY_ROTATIONS, SCIPY_F32_DIFF, SCIPY_MARGIN = 20000, 2.4e-8, 4

Case = collections.namedtuple("Case", "name max_tracks max_meas frames ties")
Frame = collections.namedtuple("Frame", "poses cam rel")


def load_harness():
    path = os.path.join(ROOT, "tests", "host_harness", "libflope_host_track.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "tests/host_harness/libflope_host_track.so"])
    lib = C.CDLL(path)
    lib.track_h_dist.restype = C.c_double
    lib.track_h_dist.argtypes = [C.c_void_p, C.c_void_p]
    lib.track_h_better.argtypes = [C.c_double, C.c_int, C.c_double, C.c_int]
    lib.track_h_match.argtypes = [C.c_double, C.c_int, C.c_double]
    lib.track_h_measure.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.track_h_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double]
    lib.track_walk.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_double] * 4 + [C.c_int, C.c_int]
    return lib


def cam_matrix(cam):
    from sunflower.predictor.flower_model import cam_pose_to_matrix
    cam = np.asarray(cam, dtype=np.float64)
    return cam if cam.shape == (4, 4) else cam_pose_to_matrix(cam)


def measure(lib, pose, cam):
    """track_measure through the harness: pose float32 or float64 [4,4], cam a 7-vector or a matrix -> float64 [7]"""
    pose = np.ascontiguousarray(pose)
    assert pose.dtype in (np.float32, np.float64)
    cm, z = np.ascontiguousarray(cam_matrix(cam)), np.empty(7)
    lib.track_h_measure(pose.ctypes.data, int(pose.dtype == np.float64), cm.ctypes.data, z.ctypes.data)
    return z


# ---- the host backend: a scalar walk over arrays with sentinel words behind them ---------------------------------------------------------
GUARD = 8


class HostWalk:
    def __init__(self, lib, max_tracks, max_meas, lanes=1, broken=0, th=TH, q=Q, r=R, p0=P0):
        self.lib, self.T, self.M, self.lanes, self.broken, self.par = lib, max_tracks, max_meas, lanes, broken, (th, q, r, p0)
        self.anchors, self.means = self._arr(max_tracks * 7, np.float64), self._arr(max_tracks * 7, np.float64)
        self.p, self.hits = self._arr(max_tracks, np.float64), self._arr(max_tracks, np.int32)
        self.cnt, self.assoc_buf = self._arr(2, np.int32), self._arr(max_meas, np.int32)
        self.last_n = -1

    @staticmethod
    def _arr(n, dtype):
        a = np.zeros(n + GUARD, dtype=dtype)
        a[n:] = 77
        return a

    def sentinels_changed(self):
        return sum(int((a[n:] != 77).sum()) for a, n in ((self.anchors, self.T * 7), (self.means, self.T * 7), (self.p, self.T), (self.hits, self.T),
                                                         (self.cnt, 2), (self.assoc_buf, self.M)))

    def update(self, poses, cam, rel=None):
        poses = np.ascontiguousarray(poses)
        assert poses.dtype in (np.float32, np.float64)
        n = poses.size // 16
        cm = np.ascontiguousarray(cam_matrix(cam))
        relp = None
        if rel is not None:
            rel = np.ascontiguousarray(rel, dtype=np.int32)
            relp = rel.ctypes.data
        rc = self.lib.track_walk(poses.ctypes.data, int(poses.dtype == np.float64), relp, n, cm.ctypes.data, self.anchors.ctypes.data,
                                 self.means.ctypes.data, self.p.ctypes.data, self.hits.ctypes.data, self.cnt.ctypes.data, self.assoc_buf.ctypes.data,
                                 self.T, self.M, *self.par, self.lanes, self.broken)
        if rc == 0 and n > 0:
            self.last_n = n
        return rc

    @property
    def overflowed(self):
        return bool(self.cnt[1])

    def read(self):
        T = int(self.cnt[0])
        return (self.anchors[:T * 7].reshape(T, 7).copy(), self.means[:T * 7].reshape(T, 7).copy(), self.p[:T].copy(), self.hits[:T].copy())

    def last_association(self):
        return self.assoc_buf[:self.last_n].copy()

    def reset(self):
        self.cnt[:2] = 0
        self.last_n = -1


# ---- builders ------------------------------------------------------------------------------------------------------------------------------
def pose(t, rotvec=(0.0, 0.0, 0.0)):
    """float64 [4,4]: a rotation orthogonal to float64 precision and a translation"""
    m = np.eye(4)
    m[:3, :3] = Rot.from_rotvec(np.asarray(rotvec, dtype=np.float64)).as_matrix()
    m[:3, 3] = t
    return m


def _poses(rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 4, 4)


def _grid(n, pitch=0.25, origin=(-1.0, -0.75, 0.5)):
    """n points on a lattice of `pitch` metres (exact in binary), 8 x 8 x ..."""
    i = np.arange(n)
    return np.stack([origin[0] + pitch * (i % 8), origin[1] + pitch * ((i // 8) % 8), origin[2] + pitch * (i // 64)], axis=1)


def _argmin_case(T, n, seed):
    """n measurements against T anchors: most near an anchor (the first, the last and those at lane and wave boundaries among them),
    every seventh far from all"""
    rng = np.random.default_rng(seed)
    anchors = _grid(T)
    f0 = _poses([pose(a, rng.normal(0, 0.4, 3)) for a in anchors])
    wanted = [0, T - 1, 62 % T, 63 % T, 64 % T, (T - 2) % T, 256 % T, 1024 % T]
    rows = []
    for m in range(n):
        if m % 7 == 6:
            rows.append(pose(np.array([3.0 + 0.25 * m, 0.1, 0.2]), rng.normal(0, 0.4, 3)))
            continue
        t = wanted[m] if m < len(wanted) else int(rng.integers(0, T))
        d = rng.normal(0, 1, 3)
        rows.append(pose(anchors[t] + d / np.linalg.norm(d) * rng.uniform(0.002, 0.03), rng.normal(0, 0.4, 3)))
    cam = np.concatenate([[0.125, -0.25, 0.0625], Rot.from_rotvec([0.1, -0.2, 0.3]).as_quat()])
    return Case(f"argmin_T{T}_n{n}", T + n, max(T, n), [Frame(f0, cam, None), Frame(_poses(rows), cam, None)], ())


ARGMIN_SHAPES = [(T, n) for T in (63, 64, 65, 257, 1025) for n in (65, 70)]


def _build():
    rng = np.random.default_rng(45)
    A = np.array([0.125, 0.25, 0.5])
    cases = []
    # 1. the first frame opens one track per measurement
    f = _poses([pose(A + [0.25 * i, 0, 0], rng.normal(0, 0.5, 3)) for i in range(5)])
    cases.append(Case("first_frame", 8, 8, [Frame(f, IDENTITY_CAM, None)], ()))
    # 2. a match at 49 mm, a new track at 51 mm
    cases.append(Case("gate_49_51", 8, 8, [Frame(_poses([pose(A, [0.1, 0.2, 0.3])]), IDENTITY_CAM, None),
                                           Frame(_poses([pose(A + [0.049, 0, 0], [0.1, 0.25, 0.3]), pose(A + [0, 0.051, 0], [0.3, 0.2, 0.1])]), IDENTITY_CAM, None)], ()))
    # 3. two measurements update one track in one frame
    cases.append(Case("two_on_one", 8, 8, [Frame(_poses([pose(A, [0.1, 0.2, 0.3]), pose(A + [1, 0, 0], [0, 0, 1.0])]), IDENTITY_CAM, None),
                                           Frame(_poses([pose(A + [0.010, 0, 0], [0.12, 0.2, 0.3]), pose(A + [1.004, 0, 0], [0, 0.01, 1.0]),
                                                         pose(A + [-0.012, 0.005, 0], [0.1, 0.17, 0.33])]), IDENTITY_CAM, None)], ()))
    # 4. two mutually close measurements far from every anchor: two new tracks, in measurement order; the next frame tells them apart
    cases.append(Case("two_new_close", 8, 8, [Frame(_poses([pose(A)]), IDENTITY_CAM, None),
                                              Frame(_poses([pose(A + [0.5, 0, 0], [0.2, 0, 0]), pose(A + [0.5, 0.010, 0], [0, 0.2, 0])]), IDENTITY_CAM, None),
                                              Frame(_poses([pose(A + [0.5, 0.008, 0], [0, 0.21, 0]), pose(A + [0.5, 0.001, 0], [0.21, 0, 0])]), IDENTITY_CAM, None)], ()))
    # 5. exact ties go to the lower index: anchors 0 / 1 around x = 0 (neighbouring lanes), 3 / 67 (one lane, two strides), 5 / 70
    pts = _grid(72, origin=(1.0, 1.0, 1.0))
    pts[0], pts[1] = [-0.03125, 0, 0], [0.03125, 0, 0]
    pts[3], pts[67] = [4 - 0.03125, 2, 0], [4 + 0.03125, 2, 0]
    pts[70], pts[5] = [8, 0.5 - 0.03125, 0], [8, 0.5 + 0.03125, 0]
    tie = _poses([pose([0, 0, 0], [0.3, 0, 0]), pose([4, 2, 0], [0, 0.3, 0]), pose([8, 0.5, 0], [0, 0, 0.3])])
    cases.append(Case("tie_lower_index", 80, 72, [Frame(_poses([pose(t) for t in pts]), IDENTITY_CAM, None), Frame(tie, IDENTITY_CAM, None)], ((1, 0), (1, 1), (1, 2))))
    # 6. rel = 0 rows are skipped (they hold no pose at all)
    f0 = _poses([pose(A), pose(A + [0.5, 0, 0])])
    f1 = _poses([pose(A + [0.01, 0, 0], [0.1, 0, 0]), np.full((4, 4), np.nan), pose(A + [0, 0.5, 0]), np.full((4, 4), np.nan), pose(A + [0.51, 0, 0])])
    cases.append(Case("rel_skipped", 8, 8, [Frame(f0, IDENTITY_CAM, None), Frame(f1, IDENTITY_CAM, np.array([1, 0, 1, 0, 1], np.int32)),
                                            Frame(_poses([np.full((4, 4), np.nan)]), IDENTITY_CAM, np.array([0], np.int32))], ()))
    # 7. n = 0 is a no-op
    cases.append(Case("n_zero", 8, 8, [Frame(np.zeros((0, 4, 4)), IDENTITY_CAM, None), Frame(f0, IDENTITY_CAM, None), Frame(np.zeros((0, 4, 4)), IDENTITY_CAM, None),
                                       Frame(_poses([pose(A + [0.02, 0, 0], [0, 0.1, 0])]), IDENTITY_CAM, None)], ()))
    # 8. lane, wave and workgroup boundaries of the argmin
    cases += [_argmin_case(T, n, 800 + T + n) for T, n in ARGMIN_SHAPES]
    # 9. one track updated 200 times
    base = np.array([0.1, 0.2, 0.3])
    long_frames = [Frame(_poses([pose(A, base)]), IDENTITY_CAM, None)]
    long_frames += [Frame(_poses([pose(A + rng.uniform(-0.01, 0.01, 3), base + rng.normal(0, 0.02, 3))]), IDENTITY_CAM, None) for _ in range(200)]
    cases.append(Case("long_200", 4, 4, long_frames, ()))
    # 10. a camera that moves and turns
    frames = []
    world = [pose(A + [0.3 * i, 0.1 * i, 0], [0.2 * i, 0.1, -0.3]) for i in range(4)]
    for k in range(4):
        cam7 = np.concatenate([[0.5 - 0.125 * k, 0.25 * k, -0.375], Rot.from_rotvec([0.3 * k, -0.7, 0.2 + 0.4 * k]).as_quat()])
        inv = np.linalg.inv(cam_matrix(cam7))
        rows = []
        for w in world[:2 + k // 2 + (k == 3)]:
            seen = w.copy()                                     # the flower as this frame sees it: turned a little, a few mm off
            seen[:3, :3] = w[:3, :3] @ Rot.from_rotvec(rng.normal(0, 0.02, 3)).as_matrix()
            seen[:3, 3] += rng.uniform(-0.004, 0.004, 3)
            cp = inv @ seen
            u, _, vt = np.linalg.svd(cp[:3, :3])               # back onto a rotation to float64 precision
            cp[:3, :3] = u @ vt
            rows.append(cp)
        frames.append(Frame(_poses(rows), cam7, None))
    cases.append(Case("camera_pose", 8, 8, frames, ()))
    # 11. a mean that has drifted 40 mm from its anchor: the measurement on the other side still matches, because distances go to the anchor
    drift = [Frame(_poses([pose(A, base)]), IDENTITY_CAM, None)] + [Frame(_poses([pose(A + [0.040, 0, 0], base)]), IDENTITY_CAM, None) for _ in range(6)]
    drift.append(Frame(_poses([pose(A + [-0.030, 0, 0], base)]), IDENTITY_CAM, None))
    cases.append(Case("drifted_mean", 4, 4, drift, ()))
    for c in cases:
        for fr in c.frames:
            fr.poses.setflags(write=False)
    return cases


def overflow_frames():
    """for a state of max_tracks = 4: a frame that opens 3, one that matches one of them and needs 2 more, one that needs 1"""
    A = np.array([0.125, 0.25, 0.5])
    three = Frame(_poses([pose(A + [0.5 * i, 0, 0], [0.1 * i, 0.2, 0]) for i in range(3)]), IDENTITY_CAM, None)
    two_more = Frame(_poses([pose(A + [0.01, 0, 0], [0, 0.2, 0.1]), pose(A + [0, 1.0, 0]), pose(A + [0, 2.0, 0])]), IDENTITY_CAM, None)
    one_more = Frame(_poses([pose(A + [0, 1.0, 0]), pose(A + [0.51, 0, 0], [0.1, 0.2, 0.05])]), IDENTITY_CAM, None)
    return three, two_more, one_more


def f32_frames():
    """the frames of case camera_pose rounded to float32 -> (as float32, the same rows widened to float64)"""
    fr = cases()["camera_pose"].frames
    f32 = [Frame(np.ascontiguousarray(f.poses, dtype=np.float32), f.cam, f.rel) for f in fr]
    return f32, [Frame(f.poses.astype(np.float64), f.cam, f.rel) for f in f32]


_CASES = {}


def cases():
    if not _CASES:
        _CASES.update({c.name: c for c in _build()})
    return _CASES


CASE_NAMES = ("first_frame", "gate_49_51", "two_on_one", "two_new_close", "tie_lower_index", "rel_skipped", "n_zero") + \
    tuple(f"argmin_T{T}_n{n}" for T, n in ARGMIN_SHAPES) + ("long_200", "camera_pose", "drifted_mean")


# ---- the oracle's answer -------------------------------------------------------------------------------------------------------------------
Expected = collections.namedtuple("Expected", "assoc tracks mp_means mp_p bound_t bound_q S nu_min")
_EXPECTED = {}


def _reliable(fr):
    n = len(fr.poses)
    return [i for i in range(n) if fr.rel is None or fr.rel[i] != 0]


def expected(case, mp_limit=300):
    """computed once per case and left unchanged.  mp_means / mp_p / bound_t / bound_q: per track, None where the exact evaluation was
    skipped (tracks that were never updated, beyond the first mp_limit, in the large cases)"""
    if case.name in _EXPECTED:
        return _EXPECTED[case.name]
    from sunflower.predictor.flower_model import poses_to_measurements
    from sunflower.utils.mvg import pose_cam_to_world
    meas, src = [], []                                   # the oracle's input, and where each of its rows came from
    for fi, fr in enumerate(case.frames):
        keep = _reliable(fr)
        rows = [list(z) for z in poses_to_measurements(pose_cam_to_world(fr.poses[keep], cam_matrix(fr.cam)))] if keep else []
        meas.append(rows)
        src.append(keep)
    live = [m for m in meas if m]                        # (an empty frame is no frame to the host: add_poses returns before the tracker)
    tracks = F.associate(live, th=TH) if live else []
    where = {id(z): (ti, k) for ti, t in enumerate(tracks) for k, z in enumerate(t)}
    assoc = []
    for fi, fr in enumerate(case.frames):
        a = np.full(len(fr.poses), SKIPPED, dtype=np.int64)
        for z, i in zip(meas[fi], src[fi]):
            ti, k = where[id(z)]
            a[i] = -1 - ti if k == 0 else ti
        assoc.append(a)
    # exact means on the oracle's membership
    origin = {id(z): (fi, i) for fi in range(len(meas)) for z, i in zip(meas[fi], src[fi])}
    S = max([float(np.linalg.norm(fr.poses[i][:3, 3]) + np.abs(cam_matrix(fr.cam)[:3, 3]).max()) for fr in case.frames for i in _reliable(fr)] + [0.0])
    mp_means, mp_p, bt, bq, nus = [], [], [], [], []
    for ti, t in enumerate(tracks):
        if ti >= mp_limit and len(t) == 1:
            mp_means.append(None); mp_p.append(None); bt.append(None); bq.append(None)
            continue
        zs = []
        for z in t:
            fi, i = origin[id(z)]
            zm, margin = TB.mp_measure(case.frames[fi].poses[i], cam_matrix(case.frames[fi].cam))
            assert margin > 1e-9, f"{case.name}: a measurement sits on a branch of the quaternion rule"
            zs.append(zm)
        x, p, nu = TB.mp_track(zs, Q, R, P0)
        b_t, b_q, _ = TB.track_bound(len(t) - 1, S, TH, Q, R, P0, nu)
        mp_means.append(x); mp_p.append(p); bt.append(float(b_t[-1])); bq.append(float(b_q[-1])); nus.append(nu)
    _EXPECTED[case.name] = Expected(assoc, tracks, mp_means, mp_p, bt, bq, S, min(nus + [1.0]))
    return _EXPECTED[case.name]


def margins(lib, case):
    """-> (gate, gap): the smallest |d - th| over every decision and the smallest d2 - d1 over every match but the declared ties,
    from the oracle's membership and track_math.h's own distances"""
    exp = expected(case)
    anchors, gate, gap = [], np.inf, np.inf
    for fi, fr in enumerate(case.frames):
        start = len(anchors)
        for i in _reliable(fr):
            z = measure(lib, fr.poses[i], fr.cam)
            d = np.sort([lib.track_h_dist(z.ctypes.data, a.ctypes.data) for a in anchors[:start]])
            if len(d):
                gate = min(gate, abs(d[0] - TH))
            if len(d) > 1 and d[0] < TH and (fi, i) not in case.ties:
                gap = min(gap, d[1] - d[0])
            if exp.assoc[fi][i] < 0:
                anchors.append(z)
    return gate, gap


# ---- running and checking ------------------------------------------------------------------------------------------------------------------
Trace = collections.namedtuple("Trace", "assoc anchors means p hits")


def run_case(case, backend, frames=None):
    """every frame through backend.update; -> Trace (the association after each frame with n > 0, the state at the end)"""
    assoc = []
    for fr in (case.frames if frames is None else frames):
        rc = backend.update(fr.poses, fr.cam, fr.rel)
        assert rc in (0, None), rc
        assoc.append(backend.last_association() if len(fr.poses) else np.zeros(0, np.int32))
    return Trace(assoc, *backend.read())


def check_integers(case, trace):
    exp = expected(case)
    fails = []
    for fi, (got, want) in enumerate(zip(trace.assoc, exp.assoc)):
        if len(got) != len(want) or (np.asarray(got, dtype=np.int64) != want).any():
            fails.append(f"{case.name} frame {fi}: association {np.asarray(got).tolist()[:12]}, expected {want.tolist()[:12]}")
    if len(trace.hits) != len(exp.tracks):
        return fails + [f"{case.name}: {len(trace.hits)} tracks, expected {len(exp.tracks)}"]
    want_hits = np.array([len(t) for t in exp.tracks], dtype=np.int64)
    if (np.asarray(trace.hits, dtype=np.int64) != want_hits).any():
        fails.append(f"{case.name}: hit counts {np.asarray(trace.hits).tolist()[:12]}, expected {want_hits.tolist()[:12]}")
    return fails


def worst_ratio(case, trace):
    """-> (largest error / bound over every checked mean component, largest error, largest relative error of p / its bound); anchors of
    checked tracks must equal their first measurement's exact value within the measurement bound too"""
    exp = expected(case)
    worst, worst_err, worst_p = 0.0, 0.0, 0.0
    e_t0, e_q0 = TB.measurement_bound(exp.S)
    for ti, x in enumerate(exp.mp_means):
        if x is None:
            continue
        n_up = len(exp.tracks[ti]) - 1
        for c in range(7):
            err = abs(float(x[c] - float(trace.means[ti][c])))
            worst_err = max(worst_err, err)
            worst = max(worst, err / (exp.bound_t[ti] if c < 3 else exp.bound_q[ti]))
        brho = TB.track_bound(n_up, exp.S, TH, Q, R, P0, 1.0)[2][-1]
        rel_p = abs(float((exp.mp_p[ti] - float(trace.p[ti])) / exp.mp_p[ti]))
        worst_p = max(worst_p, rel_p / brho if brho else (0.0 if rel_p == 0 else np.inf))
    return worst, worst_err, worst_p


def check_case(case, trace):
    """-> list of failures: integers against the oracle, means and p within the bound, never-updated tracks still at their anchor"""
    fails = check_integers(case, trace)
    if fails:
        return fails
    ratio, err, ratio_p = worst_ratio(case, trace)
    if not ratio <= 1.0:
        fails.append(f"{case.name}: a mean lies {ratio:.3g} bounds from the exact recursion (error {err:.3g})")
    if not ratio_p <= 1.0:
        fails.append(f"{case.name}: p lies {ratio_p:.3g} bounds from the exact recursion")
    once = np.asarray(trace.hits) == 1
    if once.any() and trace.anchors[once].tobytes() != trace.means[once].tobytes():
        fails.append(f"{case.name}: a track that was never updated has left its anchor")
    return fails
