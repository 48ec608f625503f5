"""Bounds for the pose math of flope_amd/csrc/pose_math.h against the references of tests/pose_cases.py, a numpy emulation of
that code, and broken copies of the emulation (tests/test_pose_bound.py shows what the bounds catch).  CPU only.

Everything below is derived from the code's operation counts and thresholds; nothing is fitted to an output.  u = 2^-24 (float32),
e = 2^-53 (float64), |M| = |M|_F, gap = s2 + sign(det M) s3, both of the float32 M as given.

PROCRUSTES      |R - R_ref|_ij <= u |R_ref_ij| + C e |M| / gap + 2^-150

  The first term is the one float32 rounding of the result (2^-150: the same rounding below the normal range).  The second is the
  float64 solve.  Horn's N (4x4 symmetric, linear in M, |N|_F = 2 |M|) has the eigenvalues l1 = s1 + s2 + t s3 >= l2 = s1 - s2 - t s3
  >= ..., t = sign(det M), so l1 - l2 = 2 gap.  A symmetric perturbation E of N turns its top eigenvector q by |dq| <= |E|_2 /
  (l1 - l2 - |E|_2), and R(q) is quadratic in the unit q with |dR_ij| <= 2 |dq| (each entry is 2 (q_a q_b +- q_c q_d) or, on the
  diagonal and to first order in a dq orthogonal to q, 2 (w dw + x dx - y dy - z dz); Cauchy-Schwarz).  Hence
  |dR_ij| <= |E|_2 / gap: DESIGN.md section 5's law |dR| gap <= 3 |dM| in its first-principles form (a dM of M is an E with
  |E|_F = 2 |dM|_F).  An absolute error d of q that is not amplified costs 2 d <= 2 sqrt(2) d |M| / gap, since gap <= sqrt(2) |M|.

  Jacobi fallback (procrustes3x3_jacobi), in units of e |M|:
      forming N: <= 2 additions per entry                                                      |E|_F <=    9
      12 sweeps x 6 rotations = 72 rotations at most.  (c, s) is a rotation up to 1 + 4e (t t, + 1, sqrt, 1 /, t c); every updated
      element c a - s b takes two products and a sum, 2e sqrt(a^2 + b^2) (fewer roundings under FMA contraction, never more);
      A <- A J and A <- J^T A touch two columns / rows each: (2 + 4) e |N|_F per side, 12 e |N|_F = 24 e |M| per rotation       1728
      stopping at off^2 <= 1e-30 diag^2 leaves |off|_F <= 1e-15 |N|_F = 9.01 e |N|_F                                               18.02
      V <- V J: 72 x 6e of absolute error in the chosen column, not amplified: 2 x 432 x sqrt(2)                                 1222
      normalisation (|q| - 1 <= 4e, twice in the quadratic form) and R's own 4 operations per entry: 24e absolute, x sqrt(2)       34
                                                                                                                   C_JACOBI =   3011
  Newton fast path (procrustes3x3_newton), |M| = 1 after its scaling.  With r the row of the largest diagonal cofactor, |q1[r]| >=
  1/2, and adj(N - l I) for l = l1 + d has the row  -P'(l1) q1[r] (q1 + (d / (l1 - l2)) (q2[r] / q1[r]) q2 + ...): an error d of the
  eigenvalue turns the vector by at most 2 d / (l1 - l2), so it counts as |E|_2 = 2 d.
      accepted at |dl| <= 1e-13 l, l <= sqrt(3): d <= 1.74e-13 = 1560 e                                                         3120
      rounding of the polynomial (c0, c1 and Horner: 30e at values below 9) moves its root by 30e / P'(l1), and the twelve minors
      (12e each) turn the row by 4 x 12e / P'(l1);  P'(l1) = (l1 - l2)(l1 - l3)(l1 - l4) = 2 gap a b with a = 2 (s1 + t s3),
      b = 2 (s1 + s2), so in units of e / gap this is (30 + 96) / (a b)                                                  126 / (a b)
      (a b >= 1 unless s1 - s3 is small with det M < 0, the near-reflections: there P'(l1) falls under the adjugate threshold
      best > 1e-7 and the row takes the fallback.  The bound carries 1 / min(1, a b) per row from the reference's singular values;
      rows whose P'(l1) = 2 gap a b cannot reach the threshold carry C_JACOBI alone.  It is 1 in all but single Gaussian rows and the near-reflections just above
      the threshold; tests/test_pose_bound.py prints the lowest a b.)
                                                                                                     C_NEWTON = 3120 + 126 =   3246
  C = max(C_JACOBI, C_NEWTON) = 3246, whichever path a row took (the device's choice cannot be observed).

  A case is judged for accuracy unless gap / |M| < 1e-10; below that line as a rotation only.

ROTATION        |R R^T - I|_ik <= 2 u (1 + 2^-20),  |det R - 1| <= 3 u (1 + 2^-20), for EVERY finite input

  Both paths normalise q in float64, so R(q) is a rotation to some 24e whatever M was; its nine entries are then rounded once,
  r_ij = r*_ij (1 + d_ij), |d_ij| <= u:  (R R^T - I)_ik = sum_j r*_ij r*_kj (d_ij + d_kj) <= 2u |r*_i| |r*_k| = 2u, and the cofactors
  of a rotation are its entries, so |det R - 1| <= u sum r*_ij^2 = 3u.  2^-20 covers the u^2 terms and the 24e.

YAW-NULL        |O - O_ref| <= u |O_ref| + K e (|a| + |b|) + 2^-150,  K = 6, per row (a, b) = (R_k0, R_k1) of the float32 R as given

  n = sqrt(c0^2 + s0^2): two squares, a sum, a root = 2e relative; c = c0 / n, s = s0 / n: 3e; a c - b s: two products and a sum on
  |c|, |s| <= 1: (3 + 2) e (|a| + |b|); 1 for the float64 rounding of the stored reference.  Column 2 is a copy: equal bits.  O01 is
  0 in exact arithmetic, so it lies within the second and third term alone.  At R00 = R01 = 0 the output is R itself, in bits.

GAP             |gap_dev - gap| <= 8 u |M|: the project's existing tolerance (tests/test_guard_host.py), unchanged.
"""
import numpy as np

import pose_cases as PC

U32, U64, SUB32 = 2.0 ** -24, 2.0 ** -53, 2.0 ** -150
C_JACOBI = 9 + 1728 + 18.02 + 1222 + 34
C_NEWTON = 3120 + 126
C = max(C_JACOBI, C_NEWTON)
K_YAW = 6
ORTH_BOUND, DET_BOUND = 2 * U32 * (1 + 2.0 ** -20), 3 * U32 * (1 + 2.0 ** -20)
GAP_TOL = 8 * U32


def newton_ab(M, gap, fro):
    """a b of the derivation from the float32 M's singular values in units |M| = 1 (float64 SVD: two digits suffice); +inf for rows
    whose P'(l1) lies under the adjugate threshold, which can only take the fallback"""
    Md = np.asarray(M, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = np.linalg.svd(Md, compute_uv=False) / np.where(fro > 0, fro, 1.0)[:, None]
        t = np.sign(np.linalg.det(Md))
        ab = 2 * (s[:, 0] + t * s[:, 2]) * 2 * (s[:, 0] + s[:, 1])
        can_be_newton = 2 * (gap / np.where(fro > 0, fro, 1.0)) * ab > 0.99e-7     # best <= P'(l1) = 2 gap a b must exceed 1e-7 (1 % for the rounding of best)
    return np.where(can_be_newton, ab, np.inf)


def procrustes_bound(R_ref, gap, fro, ab=None):
    """-> bound [n, 3, 3]; rows with gap / |M| < 1e-10 (or gap = 0) get +inf: judged as rotations only"""
    with np.errstate(all="ignore"):
        c = np.full(len(gap), C) if ab is None else np.maximum(C_JACOBI, 3120 + 126 / np.minimum(1.0, ab))
    with np.errstate(all="ignore"):
        cond = np.where(gap / fro >= PC.ROTATION_ONLY_BELOW, c * U64 * fro / gap, np.inf)
    return U32 * np.abs(R_ref) + cond[:, None, None] + SUB32


def judge_procrustes(R, R_ref, gap, fro, ab=None):
    """-> (worst err / bound per row (0 for rotation-only rows), judged-for-accuracy mask)"""
    bound = procrustes_bound(R_ref, gap, fro, ab)
    with np.errstate(all="ignore"):
        ratio = (np.abs(np.asarray(R, dtype=np.float64) - R_ref) / bound).max(axis=(1, 2))
        acc = gap / fro >= PC.ROTATION_ONLY_BELOW
    return np.where(acc, np.nan_to_num(ratio, nan=np.inf), 0.0), acc


def rotation_defect(R):
    """-> (|R R^T - I| max / ORTH_BOUND, |det R - 1| / DET_BOUND) per row; non-finite R gives inf"""
    Rd = np.asarray(R, dtype=np.float64)
    with np.errstate(all="ignore"):
        o = np.abs(Rd @ Rd.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)) / ORTH_BOUND
        d = np.abs(np.linalg.det(Rd) - 1.0) / DET_BOUND
    return np.nan_to_num(o, nan=np.inf), np.nan_to_num(d, nan=np.inf)


def yaw_bound(O_ref, R):
    ab = (np.abs(R[:, :, 0].astype(np.float64)) + np.abs(R[:, :, 1].astype(np.float64)))[:, :, None]
    b = U32 * np.abs(O_ref) + K_YAW * U64 * ab + SUB32
    b[:, :, 2] = 0.0                                                   # column 2: equal bits
    return b


def judge_yaw(O, O_ref, R):
    """-> worst err / bound per row over columns 0, 1 (inf where column 2 is not R's in bits)"""
    bound = yaw_bound(O_ref, R)
    err = np.abs(np.asarray(O, dtype=np.float64) - O_ref)
    ratio = (err[:, :, :2] / bound[:, :, :2]).max(axis=(1, 2))
    same = (np.asarray(O)[:, :, 2].view(np.uint32) == np.asarray(R)[:, :, 2].view(np.uint32)).all(axis=1)
    return np.where(same, ratio, np.inf)


# ---- numpy emulation of pose_math.h (vectorised over the batch; same formulas and thresholds, not the same bits) ---------------------
def _horn(m, dt):
    n = np.zeros((len(m), 4, 4), dtype=dt)
    n[:, 0, 0] = m[:, 0] + m[:, 4] + m[:, 8]; n[:, 1, 1] = m[:, 0] - m[:, 4] - m[:, 8]     # noqa: E702
    n[:, 2, 2] = -m[:, 0] + m[:, 4] - m[:, 8]; n[:, 3, 3] = -m[:, 0] - m[:, 4] + m[:, 8]   # noqa: E702
    for (i, j), v in (((0, 1), m[:, 7] - m[:, 5]), ((0, 2), m[:, 2] - m[:, 6]), ((0, 3), m[:, 3] - m[:, 1]), ((1, 2), m[:, 1] + m[:, 3]),
                      ((1, 3), m[:, 2] + m[:, 6]), ((2, 3), m[:, 5] + m[:, 7])):
        n[:, i, j] = n[:, j, i] = v
    return n


def _rot_of_quat(q, dt, normalise=True):
    if normalise:
        q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    w, x, y, z = q.T
    one, two = dt(1), dt(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w), two * (x * y + z * w), one - two * (x * x + z * z),
                  two * (y * z - x * w), two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)], axis=1)
    return R.astype(np.float32).reshape(-1, 3, 3)


def _jacobi(A, dt, second_if_close=False):
    """cyclic Jacobi of symmetric A [n, 4, 4] -> quaternion [n, 4] of the largest eigenvalue"""
    A = A.copy()
    n = len(A)
    V = np.tile(np.eye(4, dtype=dt), (n, 1, 1))
    for _ in range(12):
        d2 = (np.diagonal(A, axis1=1, axis2=2) ** 2).sum(axis=1)
        o2 = 2 * sum(A[:, i, j] ** 2 for i in range(3) for j in range(i + 1, 4))
        live = ~((o2 <= dt(1e-30) * d2) | (o2 == 0))
        if not live.any():
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[:, p, q]
                act = live & (apq != 0)
                th = (A[:, q, q] - A[:, p, p]) / np.where(act, 2 * apq, 1)
                t = np.where(th >= 0, 1, -1) / (np.abs(th) + np.sqrt(th * th + 1))
                c = np.where(act, 1 / np.sqrt(t * t + 1), 1).astype(dt)
                s = np.where(act, t * c, 0).astype(dt)
                for X in (A, V):
                    xp, xq = X[:, :, p].copy(), X[:, :, q].copy()
                    X[:, :, p], X[:, :, q] = c[:, None] * xp - s[:, None] * xq, s[:, None] * xp + c[:, None] * xq
                xp, xq = A[:, p, :].copy(), A[:, q, :].copy()
                A[:, p, :], A[:, q, :] = c[:, None] * xp - s[:, None] * xq, s[:, None] * xp + c[:, None] * xq
    ev = np.diagonal(A, axis1=1, axis2=2)
    order = np.argsort(-ev, axis=1, kind="stable")
    pick = order[:, 0].copy()
    if second_if_close:
        l1, l2 = np.take_along_axis(ev, order[:, :1], 1)[:, 0], np.take_along_axis(ev, order[:, 1:2], 1)[:, 0]
        pick = np.where(l1 - l2 < 1e-3 * np.abs(l1), order[:, 1], pick)
    return V[np.arange(n), :, pick]


def emulate_procrustes(M, mutate=None):
    """pose_math.h: procrustes3x3 on float32 M [n, 3, 3] -> (R float32 [n, 3, 3], took the Newton path [n]).
    mutate: None | "polar" | "transposed" | "float32" | "second_eig" | "unnormalised"  (the broken copies)"""
    M = np.asarray(M, dtype=np.float32)
    n = len(M)
    with np.errstate(all="ignore"):
        if mutate == "polar":                                          # plain polar factor: no det-sign fix
            U, _, Vt = np.linalg.svd(M.astype(np.float64))
            return (U @ Vt).astype(np.float32), np.zeros(n, dtype=bool)
        dt = np.float32 if mutate == "float32" else np.float64
        m0 = M.reshape(n, 9).astype(dt)
        qj = _jacobi(_horn(m0, dt), dt, second_if_close=(mutate == "second_eig"))
        # ---- Newton fast path ----
        fro2 = (m0.astype(np.float64) ** 2).sum(axis=1)
        ok = (fro2 > 1e-60) & (fro2 < 1e60)
        m = (m0 * (1 / np.sqrt(np.where(ok, fro2, 1)))[:, None].astype(dt)).astype(dt)
        N = _horn(m, dt)
        det = np.linalg.det(m.reshape(n, 3, 3)).astype(dt)
        c1, c0 = dt(-8) * det, np.linalg.det(N).astype(dt)
        lf, c1f, c0f = np.full(n, 1.7320509, dtype=np.float32), c1.astype(np.float32), c0.astype(np.float32)
        act = np.ones(n, dtype=bool)
        for _ in range(10):
            l2 = lf * lf
            pv, dv = (l2 - np.float32(2)) * l2 + c1f * lf + c0f, (np.float32(4) * l2 - np.float32(4)) * lf + c1f
            act &= dv > np.float32(1e-6)
            lf = np.where(act, lf - pv / np.where(act, dv, 1), lf).astype(np.float32)
        lam = (lf.astype(dt) * dt(1 + 1e-6) + dt(1e-9)).astype(dt)
        conv, fail, act, dl_last = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.ones(n, dtype=bool), np.ones(n, dtype=dt)
        for _ in range(8):
            l2 = lam * lam
            pv, dv = (l2 - 2) * l2 + c1 * lam + c0, (4 * l2 - 4) * lam + c1
            fail |= act & ~(dv > 1e-9)
            act &= ~fail
            dl = pv / np.where(act, dv, 1)
            lam = np.where(act, lam - dl, lam).astype(dt)
            dl_last = np.where(act, dl, dl_last)
            done = act & (np.abs(dl) <= 4e-16 * lam)
            conv |= done
            act &= ~done
        ok &= ~fail & (conv | (np.abs(dl_last) <= 1e-13 * lam))
        S = N - lam[:, None, None] * np.eye(4, dtype=dt)
        cof = np.empty((n, 4, 4), dtype=dt)
        for r in range(4):
            for j in range(4):
                sub = np.delete(np.delete(S, r, axis=1), j, axis=2)
                cof[:, r, j] = (-1) ** (r + j) * np.linalg.det(sub)
        dg = np.abs(np.diagonal(cof, axis1=1, axis2=2))
        r = np.argmax(dg, axis=1)
        ok &= dg[np.arange(n), r] > 1e-7
        qn = cof[np.arange(n), r]
        R = np.where(ok[:, None, None], _rot_of_quat(qn, dt, normalise=(mutate != "unnormalised")), _rot_of_quat(qj, dt))
        if mutate == "transposed":
            R = R.transpose(0, 2, 1)
        return np.ascontiguousarray(R, dtype=np.float32), ok


def emulate_yaw(R, mutate=None):
    """pose_math.h: nullify_yaw3x3 on float32 R [n, 3, 3].  mutate: None | "atan2_sign" (angle from atan2(R01, R00)) | "rz" (Rz(a)
    instead of Rz(a)^T)"""
    R = np.asarray(R, dtype=np.float32)
    with np.errstate(all="ignore"):
        c0 = R[:, 0, 0].astype(np.float64)
        s0 = (R[:, 0, 1] if mutate == "atan2_sign" else -R[:, 0, 1]).astype(np.float64)
        nrm = np.sqrt(c0 * c0 + s0 * s0)
        c, s = np.where(nrm > 0, c0 / nrm, 1.0), np.where(nrm > 0, s0 / nrm, 0.0)
    if mutate == "rz":
        s = -s
    a, b = R[:, :, 0].astype(np.float64), R[:, :, 1].astype(np.float64)
    O = np.stack([(a * c[:, None] - b * s[:, None]).astype(np.float32), (a * s[:, None] + b * c[:, None]).astype(np.float32), R[:, :, 2]], axis=2)
    return np.ascontiguousarray(O)


PROCRUSTES_MUTATIONS = ("polar", "transposed", "float32", "second_eig", "unnormalised")
YAW_MUTATIONS = ("atan2_sign", "rz")
