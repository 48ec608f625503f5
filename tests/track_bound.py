"""How far the float64 tracker (flope_amd/csrc/track_math.h: the device kernels and the host compile alike) may lie from an exact
evaluation of the same recursion, derived from the roundings the header performs -- and that exact evaluation (mpmath).  DESIGN.md 45
states the same derivation.  Used by tests/test_track_host.py (CPU) and tests/test_gpu_track.py (device).

Notation: u = 2^-53.  A sum, difference or product is one rounding (relative error <= u).  A division or a square root is counted
as 2u (one ulp): IEEE gives u, and nothing more is assumed of the device's float64 library.  Inputs are float64 numbers taken as
exact; the pose's rotation and the camera's are orthogonal to float64 precision, so rows and columns have norm 1 (+ O(u)).
Second-order terms are covered by rounding every constant up.

Measurement (track_measure)
  W[i][j] is a 4-term chain: products and sums give |dW| <= 4u sum_k |C_ik||P_kj| (Higham's gamma_4).  For the rotation part the
  sum is <= |C_i||P_j| = 1 by Cauchy-Schwarz, so eR = 4u; for the translation it is <= |t_pose|_2 + |t_cam|_inf =: S, so
      E_T = 5u S                                        (gamma_4 rounded up)
  The unnormalised quaternion q~: the trace (two sums) has error <= 3 eR + 6u; a component is at most (1 - tr) + 2 R_ii, i.e. two more
  roundings of magnitude <= 4 and two more entries: <= 5 eR + 14u = 34u; every other component is one rounding (magnitude <= 2) of two
  entries: 2 eR + 2u.  With delta = 40u per component, |dq~|_2 <= 2 delta.  The rule picks the largest of (R00, R11, R22, tr), which
  is the largest quaternion component (4 q_i^2 = 1 - tr + 2 R_ii, 4 w^2 = 1 + tr), so |q~|_2 = 4 max|q_i| >= 2.  x -> x / |x| has
  Lipschitz constant 1 / |x|, so the direction error is <= 2 delta / 1.99 < 41u, and the norm itself (four squares, three sums: 4u on
  the sum of squares, 2u + 2u for the root after halving, 2u for the division) adds 8u:
      E_Q = 49u    (2-norm of the quaternion error, hence also per component)

Filter (track_filter_update), update j with gain k_j
  p:  p -> p' = p + q (u), k = p' / (p' + r): k is increasing in p' with d ln k / d ln p' = r / (p' + r) <= 1, one sum and one
      division more, so rel(k) <= kappa = rho + u + 3u where rho = rel(p).  p_new = (1 - k)^2 p' + k^2 r is the Joseph form: it is
      stationary in k at the exact gain, so the error of k enters in second order only, and d ln p_new / d ln p' = 1 - k.  Its own
      roundings (1 - k, two squares, two products, one sum: 6) and a margin:   rho <- (1 - k)(rho + u) + 8u.
  x:  x' = x + k (z - x) has three roundings: the difference (u |z - x|), the product (u k |z - x|), the sum (u |x'|).  With D >= |z - x|:
      e <- (1 - k) e + k E + D k (kappa + 2u) + u X                 (E: the measurement's error, X >= |x'|)
      Translations: every measurement of a track lies within th of its anchor and x is a convex combination of them, so D = 2 th;
      X = S.  Quaternion part, in the 2-norm: D = 2 (two unit vectors), X = 1, and then the division by the norm nu of x':
      e <- e / nu + 8u.  nu is 1 when z = x and smaller the further the measurements of a track are apart; the caller passes a
      lower bound nu_min taken from the exact evaluation.
  An update multiplies the old error by 1 - k < 1 (by (1 - k) / nu for the quaternion), so the bound grows at most linearly with the
  number of updates, and it settles where what an update adds equals what it removes.
"""
import numpy as np

U = 2.0 ** -53
E_Q = 49 * U


def measurement_bound(S):
    """-> (E_T, E_Q): per-component error of a measurement's translation, 2-norm error of its quaternion"""
    return 5 * U * S, E_Q


def gains(n_updates, q, r, p0):
    """k_1 .. k_n of the recursion (float64: the gains themselves are only weights of the bound)"""
    ks, p = [], p0
    for _ in range(n_updates):
        p = p + q
        k = p / (p + r)
        p = (1 - k) ** 2 * p + k ** 2 * r
        ks.append(k)
    return ks


def track_bound(n_updates, S, th, q, r, p0, nu_min=1.0):
    """-> (bt, bq, brho): bt[j] / bq[j] bound a mean's translation components / quaternion components after j updates
    (j = 0 .. n_updates), brho[j] the relative error of p.  S >= |t_pose|_2 + |t_cam|_inf of every measurement, th the gate (metres),
    nu_min <= the norm of the quaternion part before each renormalisation."""
    assert 0 < nu_min <= 1.0 + 1e-12
    e_t, e_q = measurement_bound(S)
    E_T, rho = e_t, 0.0
    bt, bq, brho = [e_t], [e_q], [rho]
    for k in gains(n_updates, q, r, p0):
        kappa = rho + 4 * U
        e_t = (1 - k) * e_t + k * E_T + 2 * th * k * (kappa + 2 * U) + U * S
        e_q = ((1 - k) * e_q + k * E_Q + 2 * k * (kappa + 2 * U) + U) / nu_min + 8 * U
        rho = (1 - k) * (rho + U) + 8 * U
        bt.append(e_t); bq.append(e_q); brho.append(rho)
    return np.array(bt), np.array(bq), np.array(brho)


# ---- the exact evaluation ----------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def mp_measure(pose, cam):
    """pose, cam: float64 [4,4] -> 7 mpf: the rule of track_measure on the exact product (the branch is decided on exact values; the
    cases keep the four candidates of the rule apart)"""
    mp = _mp()
    P = [[mp.mpf(float(v)) for v in row] for row in np.asarray(pose, dtype=np.float64)]
    C = [[mp.mpf(float(v)) for v in row] for row in np.asarray(cam, dtype=np.float64)]
    W = [[sum(C[i][k] * P[k][j] for k in range(4)) for j in range(4)] for i in range(3)]
    tr = W[0][0] + W[1][1] + W[2][2]
    dec = [W[0][0], W[1][1], W[2][2], tr]
    c = max(range(4), key=lambda m: (dec[m], -m))
    if c < 3:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q = [None] * 4
        q[i] = 1 - tr + 2 * W[i][i]
        q[j] = W[j][i] + W[i][j]
        q[k] = W[k][i] + W[i][k]
        q[3] = W[k][j] - W[j][k]
    else:
        q = [W[2][1] - W[1][2], W[0][2] - W[2][0], W[1][0] - W[0][1], 1 + tr]
    n = mp.sqrt(sum(v * v for v in q))
    margin = float(min(abs(dec[c] - dec[m]) for m in range(4) if m != c))
    return [W[0][3], W[1][3], W[2][3]] + [v / n for v in q], margin


def mp_track(z_seq, q, r, p0):
    """z_seq: measurements (7 mpf each), the first opens the track -> (x[7], p, nu_min): the recursion of oracle/fusion_ref.py's
    scalar_track, exactly"""
    mp = _mp()
    q, r, p = mp.mpf(float(q)), mp.mpf(float(r)), mp.mpf(float(p0))
    x = list(z_seq[0])
    nu_min = 1.0
    for z in z_seq[1:]:
        p = p + q
        k = p / (p + r)
        x = [xi + k * (zi - xi) for xi, zi in zip(x, z)]
        p = (1 - k) ** 2 * p + k ** 2 * r
        n = mp.sqrt(sum(v * v for v in x[3:]))
        nu_min = min(nu_min, float(n))
        x = x[:3] + [v / n for v in x[3:]]
    return x, p, nu_min
