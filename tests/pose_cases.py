"""Named input classes for the pose math of flope_amd/csrc/pose_math.h (special Procrustes, conditioning figure, yaw-null), and
their high-precision references.  CPU only; shared by tests/test_pose_bound.py (host compile + Python emulation), the GPU modules
tests/test_gpu_pose_math.py / test_gpu_head.py / test_gpu_guard_select.py and tests/golden/make_pose_goldens.py.

Procrustes classes -- float32 M [n, 3, 3], each from its own seeded generator (numpy PCG64: the stream is pinned by numpy's
compatibility policy), 64 per class unless the class is a finite set:

    gauss_1e-36 gauss_1e-32 gauss_1e-20 gauss_1 gauss_1e20 gauss_1e31 gauss_1e37
                        unit Gaussians times the scale.  |M|_F^2 of the first two and the last two lies outside (1e-60, 1e60),
                        the range procrustes3x3_newton accepts: they take the Jacobi fallback, whatever their conditioning.
    rotations           the identity, the 180-degree turns about x, y, z (quaternion w = 0, where the adjugate row of the
                        w component is the worst choice), 180-degree turns about random axes, random rotations; float32 roundings
    near_rotations      rotation + 1e-3 Gaussian noise: what a trained head emits (l2 = l3 = l4 of Horn's N)
    sv_1e-1_pos ... sv_1e-7_pos, sv_1e-1_neg ... sv_1e-7_neg
                        U diag(s1, s2, +-s3) V^T with s1 in [0.5, 1.5], s2 in eps [0.5, 1.5], s3 in eps [0, 0.45]: the gap
                        s2 + sign(det) s3 is of order eps for both orientations.  (eps = 1e-7 is the order of the float32 rounding
                        of M itself: the reference is computed from the float32 M as given.)
    s1_eq_s2            s = (a, a, b): the top singular value repeated, the case of every rotation-like M; gap of order 1
    s2_eq_s3            s = (a, b, b), det > 0: gap 2 b
    signed_perms        the 24 signed permutation matrices of determinant +1 (rotations with exact zeros: 23 of 24 have a
                        zero quaternion component, 9 have w = 0).  The 24 of determinant -1 have s = (1, 1, 1) and gap exactly 0:
                        they are in `degenerate`, and the two classes together are the 48.
    reflections         float32 roundings of rotation x diag(1, 1, -1) and its row / column variants: s = 1 +- 3e-8, det < 0, so the
                        gap s2 - s3 is the float32 rounding noise itself, 4e-10 ... 1e-7 |M|_F -- the worst conditioning any class
                        reaches above the 1e-10 line, deep inside the Jacobi fallback
    near_reflections    U diag(s1, s2, -s3) V^T with s = 1 + 1e-4 noise: the top three eigenvalues of N close, gap of order 1e-4
    degenerate          rank 2 with det exactly 0 and s2 > 0 (small integer entries, third row = a combination of the other two:
                        the gap is s2, the answer is unique and judged for accuracy), rank 1 (gap 0), the zero matrix, the 24
                        signed permutations of determinant -1 (gap 0).  Where gap / |M|_F < 1e-10 a case is judged as a rotation only.
    nonfinite           a Gaussian M with one NaN, +inf or -inf entry at each of the nine positions (27 matrices)

Yaw-null classes -- float32 R [n, 3, 3]:

    yaw_rotations       random rotations
    yaw_zero            R00 = R01 = 0 exactly (first row (0, 0, +-1)): n = 0, the kernel's c = 1, s = 0 branch -- output = input, in bits
    yaw_tiny            the same with R00, R01 of order 1e-20, and denormal (1e-39 ... 1.4e-45): their squares are far below float32
                        but not below float64, so n > 0 and the angle is a real one
    yaw_pi              yaw of exactly +-pi: R00 < 0 with R01 = +0.0 and R01 = -0.0
    yaw_scaled          Gaussians times 1e-3 ... 1e3: not rotations; the kernel is a plain function of its nine inputs

References are computed from the float32 inputs as given.  procrustes_reference() uses a float64 SVD where gap / |M|_F >= 1e-6 and
mpmath at 60 digits below that (its second argument forces either); yaw_reference() is mpmath at 60 digits.  mpmath is needed only to make the goldens and to regenerate a sample in tests/test_pose_bound.py; the GPU
tests read tests/golden/pose_cases.npz.
"""
import itertools
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_cases.npz")
N_PER_CLASS = 64
GAUSS_SCALES = ("1e-36", "1e-32", "1e-20", "1", "1e20", "1e31", "1e37")
SV_EPS = ("1e-1", "1e-3", "1e-5", "1e-7")
MP_BELOW = 1e-6          # gap / |M|_F under which the float64 SVD is replaced by mpmath
ROTATION_ONLY_BELOW = 1e-10   # gap / |M|_F under which a case is judged as a rotation only

PROCRUSTES_CLASSES = ([f"gauss_{s}" for s in GAUSS_SCALES] + ["rotations", "near_rotations"] + [f"sv_{e}_pos" for e in SV_EPS] +
                      [f"sv_{e}_neg" for e in SV_EPS] + ["s1_eq_s2", "s2_eq_s3", "signed_perms", "reflections", "near_reflections",
                                                         "degenerate", "nonfinite"])
ACCURACY_CLASSES = [c for c in PROCRUSTES_CLASSES if c not in ("degenerate", "nonfinite")]
FINITE_CLASSES = [c for c in PROCRUSTES_CLASSES if c != "nonfinite"]
YAW_CLASSES = ["yaw_rotations", "yaw_zero", "yaw_tiny", "yaw_pi", "yaw_scaled"]


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def random_rotations(n, g):
    """float64 [n, 3, 3], Haar distributed (QR of a Gaussian with the sign conventions fixed), det +1"""
    q, r = np.linalg.qr(g.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    return q * np.sign(np.linalg.det(q))[:, None, None]


def signed_permutations():
    """the 48 signed permutation matrices, float64 [48, 3, 3]"""
    out = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for i in range(3):
                m[i, p[i]] = sg[i]
            out.append(m)
    return np.stack(out)


def _usv(g, n, s):
    U, V = random_rotations(n, g), random_rotations(n, g)
    return U @ (s[:, :, None] * np.eye(3)) @ V.transpose(0, 2, 1)


def procrustes_class(name, n=N_PER_CLASS):
    """-> float32 [n', 3, 3]"""
    g = _rng(name)
    if name.startswith("gauss_"):
        M = g.standard_normal((n, 3, 3)) * float(name[6:])
    elif name == "rotations":
        half = np.stack([np.diag(d) for d in ((1.0, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))])
        ax = g.standard_normal((12, 3))
        ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        turns = 2.0 * ax[:, :, None] * ax[:, None, :] - np.eye(3)              # 180 degrees about ax: w = 0
        M = np.concatenate([half, turns, random_rotations(n - 16, g)])
    elif name == "near_rotations":
        M = random_rotations(n, g) + 1e-3 * g.standard_normal((n, 3, 3))
    elif name.startswith("sv_"):
        eps, sign = float(name.split("_")[1]), (1.0 if name.endswith("pos") else -1.0)
        s = np.stack([0.5 + g.random(n), eps * (0.5 + g.random(n)), sign * eps * 0.45 * g.random(n)], axis=1)
        M = _usv(g, n, s)
    elif name == "s1_eq_s2":
        a = 0.2 + g.random(n)
        M = _usv(g, n, np.stack([a, a, a * g.random(n)], axis=1))
    elif name == "s2_eq_s3":
        a, f = 0.2 + g.random(n), 0.05 + 0.9 * g.random(n)
        M = _usv(g, n, np.stack([a, a * f, a * f], axis=1))
    elif name == "signed_perms":
        P = signed_permutations()
        M = P[np.linalg.det(P) > 0]
    elif name == "reflections":
        R = random_rotations(n, g)
        k = np.arange(n)
        F = np.stack([np.diag(np.where(np.arange(3) == i % 3, -1.0, 1.0)) for i in k])
        M = np.where((k % 2 == 0)[:, None, None], R @ F, F @ R)
    elif name == "near_reflections":
        s = 1.0 + 1e-4 * g.standard_normal((n, 3))
        s = -np.sort(-s, axis=1)
        s[:, 2] *= -1.0
        M = _usv(g, n, s)
    elif name == "degenerate":
        rows = g.integers(-4, 5, size=(16, 2, 3)).astype(np.float64)
        rows[np.all(np.cross(rows[:, 0], rows[:, 1]) == 0, axis=1)] = np.array([[1.0, 2, 0], [0, 1, -3]])   # keep rank 2
        co = g.integers(-3, 4, size=(16, 2)).astype(np.float64)
        rank2 = np.concatenate([rows, (co[:, :, None] * rows).sum(axis=1, keepdims=True)], axis=1)    # small integers: det is exactly 0
        rank2[8:] = rank2[8:].transpose(0, 2, 1) * 0.375                         # dependent columns; a dyadic scale keeps det exactly 0
        u, v = g.standard_normal((15, 3)), g.standard_normal((15, 3))
        rank1 = u[:, :, None] * v[:, None, :]
        P = signed_permutations()
        M = np.concatenate([rank2, rank1, np.zeros((1, 3, 3)), P[np.linalg.det(P) < 0]])
    elif name == "nonfinite":
        M = g.standard_normal((27, 3, 3))
        for i in range(27):
            M[i].flat[i % 9] = (np.nan, np.inf, -np.inf)[i // 9]
    else:
        raise KeyError(name)
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(M, dtype=np.float32)


def yaw_class(name, n=N_PER_CLASS):
    """-> float32 [n', 3, 3]"""
    g = _rng(name)

    def first_row_z(n):
        # first row (0, 0, sg): rows 1 and 2 turn in the xy plane
        phi, sg = g.uniform(-np.pi, np.pi, n), np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        R = np.zeros((n, 3, 3))
        R[:, 0, 2] = sg
        R[:, 1, 0], R[:, 1, 1] = np.sin(phi), np.cos(phi)
        R[:, 2, 0], R[:, 2, 1] = -sg * np.cos(phi), sg * np.sin(phi)
        return R

    if name == "yaw_rotations":
        R = random_rotations(n, g)
    elif name == "yaw_zero":
        R = first_row_z(n)
    elif name == "yaw_tiny":
        R = first_row_z(n).astype(np.float32)
        mag = np.array([1e-20, 3e-20, 1e-39, 1e-42, 1.4e-45, 7e-45, 1e-38, 1e-30], dtype=np.float32)
        k = np.arange(n)
        R[:, 0, 0] = mag[k % 8] * np.where(k // 8 % 2 == 0, 1, -1)
        R[:, 0, 1] = mag[(k // 2) % 8] * np.where(k // 16 % 2 == 0, 1, -1)
        R[k % 5 == 4, 0, 1] = 0.0                                                # one of the two exactly zero
        R[k % 7 == 6, 0, 0] = 0.0
        both = (R[:, 0, 0] == 0) & (R[:, 0, 1] == 0)
        R[both, 0, 0] = np.float32(1.4e-45)
        return R
    elif name == "yaw_pi":
        beta = g.uniform(-1.5, 1.5, n)
        c, s = np.cos(beta), np.sin(beta)
        R = np.zeros((n, 3, 3), dtype=np.float32)
        R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = -c, s, -1.0, s, c
        R[:, 0, 1] = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        return R
    elif name == "yaw_scaled":
        R = g.standard_normal((n, 3, 3)) * (10.0 ** g.uniform(-3, 3, n))[:, None, None]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(R, dtype=np.float32)


# ---- references ------------------------------------------------------------------------------------------------------------------
def _f64_reference(M):
    """float64 SVD: -> (R, gap, fro) of float32 or float64 M [n, 3, 3]"""
    Md = M.astype(np.float64)
    U, s, Vt = np.linalg.svd(Md)
    d = np.linalg.det(U) * np.linalg.det(Vt)
    R = (U * np.stack([np.ones_like(d), np.ones_like(d), d], axis=1)[:, None, :]) @ Vt
    return R, s[:, 1] + np.sign(np.linalg.det(Md)) * s[:, 2], np.sqrt((Md * Md).sum(axis=(1, 2)))


def _mp_reference_one(M, digits=60):
    """One matrix by mpmath arithmetic alone: a cyclic Jacobi eigen-solve of M^T M (12 sweeps at most, every loop bounded), then
    R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T -- U diag(1, 1, det(U V^T)) V^T written without the third singular pair, which a
    rank-2 M does not define.  M^T M squares the condition number: of 60 digits, 40 and more are left at s3 / s1 = 1e-10."""
    import mpmath as mp
    with mp.workdps(digits):
        m = [[mp.mpf(float(v)) for v in row] for row in M]
        fro = mp.sqrt(sum(v * v for row in m for v in row))
        if fro == 0:
            return np.eye(3), 0.0, 0.0
        m = [[v / fro for v in row] for row in m]
        A = [[sum(m[k][i] * m[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        V = [[mp.mpf(int(i == j)) for j in range(3)] for i in range(3)]
        tiny = mp.mpf(10) ** (-2 * digits)
        for _ in range(12):
            if A[0][1] ** 2 + A[0][2] ** 2 + A[1][2] ** 2 <= tiny:
                break
            for p, q in ((0, 1), (0, 2), (1, 2)):
                if A[p][q] == 0:
                    continue
                th = (A[q][q] - A[p][p]) / (2 * A[p][q])
                t = (1 if th >= 0 else -1) / (abs(th) + mp.sqrt(th * th + 1))
                c = 1 / mp.sqrt(t * t + 1)
                sn = t * c
                for k in range(3):
                    A[k][p], A[k][q] = c * A[k][p] - sn * A[k][q], sn * A[k][p] + c * A[k][q]
                for k in range(3):
                    A[p][k], A[q][k] = c * A[p][k] - sn * A[q][k], sn * A[p][k] + c * A[q][k]
                for k in range(3):
                    V[k][p], V[k][q] = c * V[k][p] - sn * V[k][q], sn * V[k][p] + c * V[k][q]
        order = sorted(range(3), key=lambda i: -A[i][i])
        lam = [max(A[i][i], mp.mpf(0)) for i in order]
        sv = [mp.sqrt(x) for x in lam]
        det = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
               m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
        gap = (sv[1] + mp.sign(det) * sv[2]) * fro
        if sv[1] < mp.mpf(10) ** (-digits // 2):                   # rank <= 1: no unique answer; judged as a rotation only
            return np.eye(3), 0.0, float(fro)
        v = [[V[k][i] for k in range(3)] for i in order[:2]]
        u = [[sum(m[r][k] * v[i][k] for k in range(3)) / sv[i] for r in range(3)] for i in range(2)]
        d = sum(u[0][k] * u[1][k] for k in range(3))               # (Gram-Schmidt: u2 is exact to working precision already)
        u[1] = [u[1][k] - d * u[0][k] for k in range(3)]
        for w in (u[0], u[1]):
            nrm = mp.sqrt(sum(x * x for x in w))
            w[:] = [x / nrm for x in w]
        cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]   # noqa: E731
        u3, v3 = cr(u[0], u[1]), cr(v[0], v[1])
        R = [[float(u[0][i] * v[0][j] + u[1][i] * v[1][j] + u3[i] * v3[j]) for j in range(3)] for i in range(3)]
        return np.array(R), float(gap), float(fro)


def procrustes_reference(M, force=None):
    """R_ref float64 [n, 3, 3] (the float64 rounding of the exact special-Procrustes rotation), gap and |M|_F float64 [n], and
    which rows came from mpmath.  force: None = by conditioning, "f64" or "mp" = every row by that method.  Finite M only."""
    M = np.asarray(M)
    assert np.isfinite(M).all()
    R, gap, fro = _f64_reference(M)
    with np.errstate(invalid="ignore", divide="ignore"):
        ill = ~(gap / fro >= MP_BELOW) & (fro > 0)
    use_mp = np.full(len(M), force == "mp") if force else ill
    for i in np.nonzero(use_mp)[0]:
        R[i], gap[i], fro[i] = _mp_reference_one(M[i])
    return R, gap, fro, use_mp


def yaw_reference(R):
    """O_ref float64 [n, 3, 3]: the float64 rounding of R Rz(a)^T, a = atan2(-R01, R00) of the float32 R as given, Rz(a) =
    [[cos a, -sin a, 0], [sin a, cos a, 0], [0, 0, 1]] -- the statement of mvg.py (zeroing the first 'zyx' Euler angle), by
    mpmath's atan2 / cos / sin at 60 digits, not the kernel's c0 / n form."""
    import mpmath as mp
    R = np.asarray(R)
    out = np.empty(R.shape, dtype=np.float64)
    with mp.workdps(60):
        for i, r in enumerate(R):
            x, y = mp.mpf(float(r[0, 0])), -mp.mpf(float(r[0, 1]))
            a = mp.atan2(y, x) if (x != 0 or y != 0) else mp.mpf(0)
            c, s = mp.cos(a), mp.sin(a)
            for k in range(3):
                p, q = mp.mpf(float(r[k, 0])), mp.mpf(float(r[k, 1]))
                out[i, k] = (float(p * c - q * s), float(p * s + q * c), float(r[k, 2]))     # row k of R times Rz(a)^T
    return out


# ---- the goldens -----------------------------------------------------------------------------------------------------------------
def load_goldens():
    """{"M/<class>", "R/<class>", "gap/<class>", "fro/<class>", "mp/<class>", "yawR/<class>", "yawO/<class>"} of the committed file"""
    return dict(np.load(GOLDEN))


def interleave(parts):
    """rows of the arrays in `parts` (equal trailing shape) dealt out one by one -> (array, [(class index, row)] per output row);
    shorter arrays simply run out"""
    order = [(c, r) for r in range(max(len(p) for p in parts)) for c, p in enumerate(parts) if r < len(p)]
    return np.stack([parts[c][r] for c, r in order]), order
