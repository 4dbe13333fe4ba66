"""NumPy model of roam_pose_graph_optimize (include/roam_abi.h), operation by operation: g2o's EdgeSE2 error and Jacobians, the Huber
kernel, the additive update with the angle normalised, and g2o's Levenberg-Marquardt.  The contract of the device kernel; PARITY
UNPINNED against g2o itself (not installed, and the reference keeps no output of it).

The system is dense here and solved by numpy.linalg.solve.  `chol=True` solves it by a Cholesky factor and two triangular solves
instead, and `trig_ulp` perturbs every sin and cos by a seeded +-n ulp: a second float64 order of the same algorithm, whose distance
from the first is what tests/pose_graph_cases.py measure_spread() reports.  The trials of an iteration end when one is accepted, when
rho == 0 exactly, after max_trials or when lambda is not finite (g2o: `while (rho < 0 && qmax < maxTrials)`); the optimisation ends
after max_iterations or with the first iteration that accepted no trial."""
import numpy as np

STATS = np.dtype([("iterations", np.int32), ("trials", np.int32), ("rejected", np.int32), ("stop", np.int32),
                  ("chi2_initial", np.float64), ("chi2_final", np.float64), ("lambda_final", np.float64)])


def normalize(th):
    """roam_normalize_angle: fmod(th + pi, 2 pi), + 2 pi if negative, - pi - the bits of (th + pi) % (2 pi) - pi"""
    return (th + np.pi) % (2 * np.pi) - np.pi


class _Trig:
    """sin / cos of arrays, optionally moved by a seeded +-n ulp"""

    def __init__(self, ulp=0, seed=0):
        self.ulp, self.rng = ulp, np.random.default_rng(seed)

    def _shift(self, v):
        if not self.ulp:
            return v
        return v + self.rng.integers(-self.ulp, self.ulp + 1, v.shape) * np.spacing(v)

    def sincos(self, th):
        return self._shift(np.sin(th)), self._shift(np.cos(th))


def edge_terms(x, ij, meas, trig, jac):
    """errors e (E, 3) of all edges at the poses x and, with jac, A = de/dx_i and B = de/dx_j (E, 3, 3)"""
    xi, xj = x[ij[:, 0]], x[ij[:, 1]]
    s, c = trig.sincos(xi[:, 2])
    sz, cz = trig.sincos(meas[:, 2])
    dx, dy = xj[:, 0] - xi[:, 0], xj[:, 1] - xi[:, 1]
    ux, uy = (c * dx + s * dy) - meas[:, 0], (c * dy - s * dx) - meas[:, 1]
    e = np.stack([cz * ux + sz * uy, cz * uy - sz * ux, normalize((xj[:, 2] - xi[:, 2]) - meas[:, 2])], axis=1)
    if not jac:
        return e, None, None
    E = len(ij)
    o, z = np.ones(E), np.zeros(E)
    Z = np.stack([np.stack([cz, sz, z], 1), np.stack([-sz, cz, z], 1), np.stack([z, z, o], 1)], 1)
    A0 = np.stack([np.stack([-c, -s, c * dy - s * dx], 1), np.stack([s, -c, -(c * dx) - s * dy], 1), np.stack([z, z, -o], 1)], 1)
    B0 = np.stack([np.stack([c, s, z], 1), np.stack([-s, c, z], 1), np.stack([z, z, o], 1)], 1)
    return e, Z @ A0, Z @ B0


def robust(e, info, huber):
    """s2 = e^T O e -> (rho, w) per edge; huber 0 = no kernel"""
    s2 = np.einsum("ea,eab,eb->e", e, info, e)
    out = (huber > 0) & (s2 > huber * huber)
    sq = np.sqrt(np.where(out, s2, 1.0))
    return np.where(out, 2 * huber * sq - huber * huber, s2), np.where(out, huber / sq, 1.0)


def chi2_of(x, ij, meas, info, huber, trig=None):
    if len(ij) == 0:
        return 0.0
    e, _, _ = edge_terms(x, ij, meas, trig or _Trig(), False)
    return float(robust(e, info, huber)[0].sum())


def _solve(M, b, chol):
    """-> (delta, ok).  ok False: the Cholesky factorisation met a pivot that is not positive or not finite"""
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return np.zeros_like(b), False
    if not np.isfinite(L).all():
        return np.zeros_like(b), False
    if chol:
        from scipy.linalg import solve_triangular
        return solve_triangular(L.T, solve_triangular(L, b, lower=True), lower=False), True
    return np.linalg.solve(M, b), True


def optimize(poses, fixed, ij, meas, info, huber=None, max_iterations=20, max_trials=10, lambda_init=0.0, chol=False, trig_ulp=0, seed=0):
    """-> (poses (V, 3), stats (a STATS scalar), log: a list of (iteration, trial, rho, lambda, cur, tmp) for every trial, lambda
    being the damping the trial was solved with)"""
    x = np.array(poses, np.float64)
    fixed = np.asarray(fixed) != 0
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    E, V = len(ij), len(x)
    meas = np.asarray(meas, np.float64).reshape(E, 3)
    info = np.broadcast_to(np.asarray(info, np.float64), (E, 3, 3))
    huber = np.zeros(E) if huber is None else np.asarray(huber, np.float64)
    trig = _Trig(trig_ulp, seed)
    max_trials = max_trials or 10
    free = np.flatnonzero(~fixed)
    cidx = np.full(V, -1)
    cidx[free] = np.arange(len(free))
    n = 3 * len(free)
    st = np.zeros((), STATS)
    cur = chi2_of(x, ij, meas, info, huber, trig)
    st["chi2_initial"] = cur
    log = []
    lam, ni = 0.0, 2.0
    for it in range(max_iterations if n and E else 0):
        e, A, B = edge_terms(x, ij, meas, trig, True)
        _, w = robust(e, info, huber)
        H, b = np.zeros((n, n)), np.zeros(n)
        for t in range(E):
            ends = [(cidx[ij[t, 0]], A[t]), (cidx[ij[t, 1]], B[t])]
            for ka, Ja in ends:
                if ka < 0:
                    continue
                b[3 * ka:3 * ka + 3] -= w[t] * (Ja.T @ (info[t] @ e[t]))
                for kb, Jb in ends:
                    if kb >= 0:
                        H[3 * ka:3 * ka + 3, 3 * kb:3 * kb + 3] += w[t] * (Ja.T @ (info[t] @ Jb))
        if it == 0:
            lam = lambda_init if lambda_init > 0 else 1e-5 * float(np.diag(H).max())
        accepted, rho = False, 0.0
        for q in range(max_trials):
            d, ok = _solve(H + lam * np.eye(n), b, chol)
            xt = x.copy()
            xt[free] += d.reshape(-1, 3)
            xt[free, 2] = normalize(xt[free, 2])
            tmp = chi2_of(xt, ij, meas, info, huber, trig) if ok else np.inf
            rho = (cur - tmp) / (float(d @ (lam * d + b)) + 1e-3)
            log.append((it, q, rho, lam, cur, tmp))
            st["trials"] += 1
            if rho > 0 and np.isfinite(tmp):
                a = 2 * rho - 1
                lam *= max(1 / 3, min(1 - a * a * a, 2 / 3))
                ni, cur, x, accepted = 2.0, tmp, xt, True
                break
            lam *= ni
            ni *= 2
            st["rejected"] += 1
            if rho == 0 or not np.isfinite(lam):
                break
        st["iterations"] += 1
        if not np.isfinite(lam):
            st["stop"] = 2
            break
        if not accepted:
            st["stop"] = 1
            break
    st["chi2_final"], st["lambda_final"] = cur, lam
    return x, st, log


def envelope(fixed, ij):
    """the host half's plan in Python -> (first column of every block row of the free system, envelope blocks)"""
    fixed = np.asarray(fixed) != 0
    cidx = np.full(len(fixed), -1)
    cidx[~fixed] = np.arange(int((~fixed).sum()))
    first = np.arange(int((~fixed).sum()))
    for i, j in np.asarray(ij).reshape(-1, 2):
        a, b = sorted((cidx[i], cidx[j]))
        if a >= 0:
            first[b] = min(first[b], a)
    return first, int((np.arange(len(first)) - first + 1).sum())
