"""Float64 model of the motion-distortion solve (csrc/lm_wave.inc, csrc/kabsch_mds.hip): MINPACK lmdif as scipy.optimize.least_squares
(method='lm', jac='2-point') calls it for this problem - ftol = xtol = gtol = 1e-8, maxfev = 100 n (n + 1) = 4200, epsfcn = eps,
factor = 100, mode 2 with diag = 1 - restated from the published description of MINPACK (More, Garbow, Hillstrom 1980: lmdif, fdjac2,
qrfac, lmpar, qrsolv) and from oracle/c/lm.c, with the residual and start vector of MotionDistortionSolver.

The model exists to say which results of a solve hang on rounding and which do not (tests/lm_cases.py), so it takes switches:
  trig_ulp = k, seed = s   every cos, sin, log and atan2 result is multiplied by 1 + j eps, j in -k..k a hash of (the argument's bits,
                           the seed): the same argument gives the same result, as on any real implementation
  order = "pairwise"       the reductions over rows (norm of fvec, column norms, Householder dot products, Q^T f) are summed as a
                           binary tree instead of first row to last
  mutant = NAME            one of MUTANTS: a single-line change of lmpar, qrsolv or the step rules.  Only there so that the CPU test
                           can show that the committed cases see such a change
  sqrt_div_ulp = k         (lmpar alone) every sqrt and quotient of lmpar / qrsolv moved likewise: the bar of the device's lmpar

Norms are sqrt(sum of squares) as on the device; MINPACK's enorm scales against over- and underflow, which is the same number for
components between 1e-150 and 1e150 whose squares do not vanish beside the sum."""
import math
import struct

import numpy as np

EPS = 2.220446049250313e-16
DWARF = 2.2250738585072014e-308
N_PAR = 6
FTOL = XTOL = GTOL = 1e-8
MAXFEV = 100 * N_PAR * (N_PAR + 1)
FACTOR = 100.0
SIGMA5 = np.array([4.0, 4.0, 1.0, 1.0, (5 * np.pi / 180) ** 2])

# whole-solve mutants: change (nfev, info) of some committed case; lmpar-only mutants: no solve with stable counts reaches them
SOLVE_MUTANTS = ("lmpar_one_iter", "qrsolv_rot_sign", "delta_shrink_quarter", "par_halve_missing", "par_div_missing",
                 "first_iter_delta_clip", "newton_parl_skipped")
LMPAR_MUTANTS = ("parl_not_updated", "paru_not_updated", "par_init_no_clamp_hi")
MUTANTS = SOLVE_MUTANTS + LMPAR_MUTANTS

_M64 = (1 << 64) - 1
_C1, _C2, _GOLD = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53, 0x9E3779B97F4A7C15


class Pert:
    """result * (1 + j eps), j = hash(argument bits, seed, tag) mod (2 k + 1) - k"""

    def __init__(self, k=0, seed=0):
        self.k = int(k)
        self.key = (int(seed) * _GOLD) & _M64

    def scalar(self, v, arg, tag):
        if self.k == 0:
            return v
        b = struct.unpack("<Q", struct.pack("<d", arg))[0] ^ ((self.key + tag) & _M64)
        b ^= b >> 33
        b = (b * _C1) & _M64
        b ^= b >> 33
        b = (b * _C2) & _M64
        b ^= b >> 33
        return v * (1.0 + (b % (2 * self.k + 1) - self.k) * EPS)

    def array(self, v, arg, tag):
        if self.k == 0:
            return v
        b = np.ascontiguousarray(arg, np.float64).view(np.uint64) ^ np.uint64((self.key + tag) & _M64)
        b = b ^ (b >> np.uint64(33))
        b = b * np.uint64(_C1)
        b = b ^ (b >> np.uint64(33))
        b = b * np.uint64(_C2)
        b = b ^ (b >> np.uint64(33))
        j = (b % np.uint64(2 * self.k + 1)).astype(np.int64) - self.k
        return v * (1.0 + j * EPS)

    def cos(self, a):
        return self.scalar(math.cos(a), a, 1)

    def sin(self, a):
        return self.scalar(math.sin(a), a, 2)

    def atan2(self, y, x):
        return self.scalar(math.atan2(y, x), y + 3.0 * x, 4)

    def vcos(self, a):
        return self.array(np.cos(a), a, 1)

    def vsin(self, a):
        return self.array(np.sin(a), a, 2)

    def vlog(self, a):
        return self.array(np.log(a), a, 3)

    def vatan2(self, y, x):
        return self.array(np.arctan2(y, x), y + 3.0 * x, 4)


class Arith:
    """sqrt and divide of lmpar / qrsolv; k > 0 moves every result by a hashed j in -k..k ulp"""

    def __init__(self, k=0, seed=0):
        self.p = Pert(k, seed)

    def sqrt(self, a):
        return self.p.scalar(math.sqrt(a), a, 5)

    def div(self, a, b):
        return self.p.scalar(a / b, a + 3.0 * b, 6) if b != 0 and math.isfinite(a) else a / b


_PLAIN = Arith()


def sum_sequential(v):
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


_ZERO1 = np.zeros(1)


def sum_pairwise(v):
    n = len(v)
    if n == 0:
        return 0.0
    while n > 1:
        if n & 1:
            v = np.concatenate((v, _ZERO1))
            n += 1
        v = v[0::2] + v[1::2]
        n >>= 1
    return float(v[0])


def enorm6(v):
    s = 0.0
    for t in v:
        s += t * t
    return math.sqrt(s)


# ------------------------------------------------------------------------------------------------ the MDS problem
class Problem:
    """update_problem of MotionDistortionSolver: T_wj0, p_w (N, 2), p_jt (N, 2), T_init, sigma5 = the covariance diagonals"""

    def __init__(self, T0, p_w, p_jt, T_init, sigma5=SIGMA5, period=0.25, pert=None):
        P = self.pert = pert or Pert()
        self.T0 = np.ascontiguousarray(T0, np.float64)
        self.Ti = np.ascontiguousarray(T_init, np.float64)
        self.p_w = np.ascontiguousarray(np.asarray(p_w)[:, :2], np.float64)
        self.p_jt = np.ascontiguousarray(np.asarray(p_jt)[:, :2], np.float64)
        self.sigma5 = np.ascontiguousarray(sigma5, np.float64)
        self.N = self.p_w.shape[0]
        self.m = 2 * self.N + 3
        self.period = float(period)
        a, b, x, c, d, y = (float(t) for t in self.T0.ravel()[:6])
        det = a * d - b * c
        I = [d / det, -b / det, 0.0, -c / det, a / det, 0.0]
        I[2] = -(I[0] * x + I[1] * y)
        I[5] = -(I[3] * x + I[4] * y)
        self.I = I
        self.ip = [1 / float(self.sigma5[0]), 1 / float(self.sigma5[1])]
        self.iv = [1 / float(self.sigma5[k]) for k in (2, 3, 4)]
        self.px, self.py = self.p_jt[:, 0].copy(), self.p_jt[:, 1].copy()
        self.wx, self.wy = self.p_w[:, 0].copy(), self.p_w[:, 1].copy()
        self.dT = self.period * P.vatan2(-self.py, -self.px) / (2 * math.pi)
        Ti = [float(t) for t in self.Ti.ravel()[:6]]
        r00, r10 = I[0] * Ti[0] + I[1] * Ti[3], I[3] * Ti[0] + I[4] * Ti[3]
        self.x0 = [(I[0] * Ti[2] + I[1] * Ti[5] + I[2]) / self.period, (I[3] * Ti[2] + I[4] * Ti[5] + I[5]) / self.period,
                   P.atan2(r10, r00) / self.period, Ti[2], Ti[5], P.atan2(Ti[3], Ti[0])]

    def resid(self, x):
        """error_vector -> (2 N + 3,)"""
        return self.resid_many(np.array([x], np.float64))[0]

    def resid_many(self, X):
        """error_vector at every row of X (k, 6) -> (k, 2 N + 3): the same operations per entry as one vector at a time (what fdjac2's
        six evaluations cost in NumPy calls is what the CPU test's time goes to)"""
        P, I, N = self.pert, self.I, self.N
        X = np.asarray(X, np.float64)
        k = X.shape[0]
        ct = np.array([P.cos(float(t)) for t in X[:, 5]])
        st = np.array([P.sin(float(t)) for t in X[:, 5]])
        a = X[:, 2, None] * self.dT
        ca, sa = P.vcos(a), P.vsin(a)
        ux = ca * self.px - sa * self.py + X[:, 0, None] * self.dT
        uy = sa * self.px + ca * self.py + X[:, 1, None] * self.dT
        wx, wy = self.wx - X[:, 3, None], self.wy - X[:, 4, None]
        nx = (ct[:, None] * wx + st[:, None] * wy) - ux
        ny = (-st[:, None] * wx + ct[:, None] * wy) - uy
        F = np.empty((k, self.m))
        F[:, 0:2 * N:2] = self.ip[0] * P.vlog(nx * nx / 2 + 1)
        F[:, 1:2 * N:2] = self.ip[1] * P.vlog(ny * ny / 2 + 1)
        Nn = float(N)
        for r in range(k):
            x, c, s_ = [float(t) for t in X[r]], float(ct[r]), float(st[r])
            tx, ty = x[3], x[4]
            m00, m10 = I[0] * c + I[1] * s_, I[3] * c + I[4] * s_
            mdx, mdy = I[0] * tx + I[1] * ty + I[2], I[3] * tx + I[4] * ty + I[5]
            dth = P.atan2(m10, m00)
            d0, d1 = x[0] - mdx / self.period, x[1] - mdy / self.period
            w = math.fmod(x[2] - dth / self.period + math.pi, 2 * math.pi)
            if w < 0:
                w += 2 * math.pi
            d2 = w - math.pi
            F[r, 2 * N] = self.iv[0] * (d0 * Nn)
            F[r, 2 * N + 1] = self.iv[1] * (d1 * Nn)
            F[r, 2 * N + 2] = self.iv[2] * (d2 * Nn)
        return F

    def cost(self, x):
        """|f(x)|^2, unperturbed, first row to last"""
        f = Problem(self.T0, self.p_w, self.p_jt, self.Ti, self.sigma5, self.period).resid([float(t) for t in x])
        return sum_sequential(f * f)


# ------------------------------------------------------------------------------------------------ MINPACK pieces
def fdjac2(prob, x, fvec):
    """forward differences, h = sqrt(eps) |x_j| (sqrt(eps) at 0) -> A (6, m): row j = column j of the Jacobian"""
    eps = math.sqrt(EPS)
    X = np.tile(np.array(x, np.float64), (N_PAR, 1))
    h = np.empty(N_PAR)
    for j in range(N_PAR):
        h[j] = eps * abs(x[j])
        if h[j] == 0:
            h[j] = eps
        X[j, j] = x[j] + h[j]
    return (prob.resid_many(X) - fvec) / h[:, None]


def qrfac(A, rsum):
    """pivoted Householder QR of the columns A[j] in place, with the rdiag down-date -> (ipvt, rdiag, acnorm)"""
    n, m = A.shape
    acnorm = [math.sqrt(rsum(A[j] * A[j])) for j in range(n)]
    rdiag, wa, ipvt = acnorm[:], acnorm[:], list(range(n))
    for j in range(min(m, n)):
        kmax = j
        for k in range(j, n):
            if rdiag[k] > rdiag[kmax]:
                kmax = k
        if kmax != j:
            A[[j, kmax]] = A[[kmax, j]]
            rdiag[kmax] = rdiag[j]
            wa[kmax] = wa[j]
            ipvt[j], ipvt[kmax] = ipvt[kmax], ipvt[j]
        cj = A[j, j:]
        ajnorm = math.sqrt(rsum(cj * cj))
        if ajnorm != 0:
            if cj[0] < 0:
                ajnorm = -ajnorm
            cj /= ajnorm
            cj[0] += 1
            for k in range(j + 1, n):
                ck = A[k, j:]
                temp = rsum(cj * ck) / float(cj[0])
                ck -= temp * cj
                if rdiag[k] != 0:
                    temp = float(ck[0]) / rdiag[k]
                    d = 1 - temp * temp
                    rdiag[k] *= math.sqrt(d if d > 0 else 0.0)
                    q = rdiag[k] / wa[k]
                    if 0.05 * (q * q) <= EPS:
                        rdiag[k] = math.sqrt(rsum(ck[1:] * ck[1:]))
                        wa[k] = rdiag[k]
        rdiag[j] = -ajnorm
    return ipvt, rdiag, acnorm


def qrsolv(r, ipvt, diag, qtb, ar=_PLAIN, mutant=None):
    """r: n x n lists, upper triangle = R; on exit the strict lower triangle holds S^T -> (x, sdiag)"""
    n = len(qtb)
    x, wa, sdiag = [0.0] * n, list(qtb), [0.0] * n
    for j in range(n):
        for i in range(j, n):
            r[i][j] = r[j][i]
        x[j] = r[j][j]
    sign = 1.0 if mutant == "qrsolv_rot_sign" else -1.0
    for j in range(n):
        l = ipvt[j]
        if diag[l] != 0:
            for k in range(j, n):
                sdiag[k] = 0.0
            sdiag[j] = diag[l]
            qtbpj = 0.0
            for k in range(j, n):
                if sdiag[k] == 0:
                    continue
                if abs(r[k][k]) < abs(sdiag[k]):
                    cot = ar.div(r[k][k], sdiag[k])
                    s = ar.div(0.5, ar.sqrt(0.25 + 0.25 * (cot * cot)))
                    c = s * cot
                else:
                    t = ar.div(sdiag[k], r[k][k])
                    c = ar.div(0.5, ar.sqrt(0.25 + 0.25 * (t * t)))
                    s = c * t
                r[k][k] = c * r[k][k] + s * sdiag[k]
                temp = c * wa[k] + s * qtbpj
                qtbpj = sign * s * wa[k] + c * qtbpj
                wa[k] = temp
                for i in range(k + 1, n):
                    temp = c * r[i][k] + s * sdiag[i]
                    sdiag[i] = -s * r[i][k] + c * sdiag[i]
                    r[i][k] = temp
        sdiag[j] = r[j][j]
        r[j][j] = x[j]
    nsing = n
    for j in range(n):
        if sdiag[j] == 0 and nsing == n:
            nsing = j
        if nsing < n:
            wa[j] = 0.0
    for k in range(nsing):
        j = nsing - 1 - k
        s = 0.0
        for i in range(j + 1, nsing):
            s += r[i][j] * wa[i]
        wa[j] = ar.div(wa[j] - s, sdiag[j])
    for j in range(n):
        x[ipvt[j]] = wa[j]
    return x, sdiag


def lmpar(R, ipvt, diag, qtb, delta, par, mutant=None, sqrt_div_ulp=0, seed=0, full=False):
    """More's Levenberg-Marquardt parameter.  R (n, n): upper triangle of the pivoted QR (R[i][j], i <= j), ipvt the pivot order,
    diag the scaling, qtb = the first n of Q^T b, delta the trust radius, par the incoming estimate.
    -> (par, x, sdiag, iterations); iterations = 0: the Gauss-Newton step was accepted (par = 0).
    full: also the final |D x| as a fifth value"""
    ar = Arith(sqrt_div_ulp, seed) if sqrt_div_ulp else _PLAIN
    n = len(qtb)
    r = [[float(R[i][j]) for j in range(n)] for i in range(n)]
    ipvt, diag, qtb = [int(t) for t in ipvt], [float(t) for t in diag], [float(t) for t in qtb]
    delta, par = float(delta), float(par)
    nsing = n
    wa1 = [0.0] * n
    for j in range(n):
        wa1[j] = qtb[j]
        if r[j][j] == 0 and nsing == n:
            nsing = j
        if nsing < n:
            wa1[j] = 0.0
    for k in range(nsing):
        j = nsing - 1 - k
        wa1[j] = ar.div(wa1[j], r[j][j])
        temp = wa1[j]
        for i in range(j):
            wa1[i] -= r[i][j] * temp
    x = [0.0] * n
    for j in range(n):
        x[ipvt[j]] = wa1[j]
    it = 0
    wa2 = [diag[j] * x[j] for j in range(n)]
    nrm = (lambda v: ar.sqrt(_ssq(v))) if ar is not _PLAIN else enorm6
    dxnorm = nrm(wa2)
    fp = dxnorm - delta
    if fp <= 0.1 * delta:
        out = (0.0, x, [0.0] * n, 0)
        return out + (dxnorm,) if full else out
    parl = 0.0
    if nsing >= n and mutant != "newton_parl_skipped":
        for j in range(n):
            l = ipvt[j]
            wa1[j] = diag[l] * ar.div(wa2[l], dxnorm)
        for j in range(n):
            s = 0.0
            for i in range(j):
                s += r[i][j] * wa1[i]
            wa1[j] = ar.div(wa1[j] - s, r[j][j])
        temp = nrm(wa1)
        parl = ar.div(ar.div(ar.div(fp, delta), temp), temp)
    for j in range(n):
        s = 0.0
        for i in range(j + 1):
            s += r[i][j] * qtb[i]
        wa1[j] = ar.div(s, diag[ipvt[j]])
    gnorm = nrm(wa1)
    paru = ar.div(gnorm, delta)
    if paru == 0:
        paru = DWARF / min(delta, 0.1)
    if par < parl:
        par = parl
    if par > paru and mutant != "par_init_no_clamp_hi":
        par = paru
    if par == 0:
        par = ar.div(gnorm, dxnorm)
    last = 1 if mutant == "lmpar_one_iter" else 10
    while True:
        it += 1
        if par == 0:
            par = max(DWARF, 0.001 * paru)
        temp = ar.sqrt(par)
        x, sdiag = qrsolv(r, ipvt, [temp * d for d in diag], qtb, ar, mutant)
        wa2 = [diag[j] * x[j] for j in range(n)]
        dxnorm = nrm(wa2)
        temp = fp
        fp = dxnorm - delta
        if abs(fp) <= 0.1 * delta or (parl == 0 and fp <= temp and temp < 0) or it == last:
            break
        for j in range(n):
            l = ipvt[j]
            wa1[j] = diag[l] * ar.div(wa2[l], dxnorm)
        for j in range(n):
            wa1[j] = ar.div(wa1[j], sdiag[j])
            t = wa1[j]
            for i in range(j + 1, n):
                wa1[i] -= r[i][j] * t
        temp = nrm(wa1)
        parc = ar.div(ar.div(ar.div(fp, delta), temp), temp)
        if fp > 0 and par > parl and mutant != "parl_not_updated":
            parl = par
        if fp < 0 and par < paru and mutant != "paru_not_updated":
            paru = par
        par = max(parl, par + parc)
    out = (par, x, sdiag, it)
    return out + (dxnorm,) if full else out


def _ssq(v):
    s = 0.0
    for t in v:
        s += t * t
    return s


class Result:
    """x (6,), nfev, info, log = [(par, delta, ratio, lmpar iterations)] per trial (par, delta as they entered lmpar), x0, r0 = the
    start and its residual, cost = |f|^2 at x, calls = lmpar's inputs per trial when asked for, gnorms = the scaled gradient norm
    lmdif tests against gtol, per outer iteration"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def counts(self):
        return self.nfev, self.info

    @property
    def rejected(self):
        return sum(1 for t in self.log if t[2] < 1e-4)

    @property
    def lmpar_max(self):
        return max((t[3] for t in self.log), default=0)


def solve(T0, p_w, p_jt, T_init, sigma5=SIGMA5, period=0.25, trig_ulp=0, seed=0, order="sequential", mutant=None, capture=False):
    """update_problem + optimize_library -> Result"""
    assert order in ("sequential", "pairwise") and (mutant is None or mutant in MUTANTS)
    rsum = sum_pairwise if order == "pairwise" else sum_sequential
    prob = Problem(T0, p_w, p_jt, T_init, sigma5, period, Pert(trig_ulp, seed))
    n, m = N_PAR, prob.m
    x = list(prob.x0)
    diag = [1.0] * n
    fvec = prob.resid(x)
    r0 = fvec.copy()
    nfev, info, it = 1, 0, 1
    par = delta = xnorm = 0.0
    fnorm = math.sqrt(rsum(fvec * fvec))
    log, calls, gnorms = [], [], []
    while True:
        A = fdjac2(prob, x, fvec)
        nfev += n
        ipvt, rdiag, acnorm = qrfac(A, rsum)
        if it == 1:
            xnorm = enorm6([diag[j] * x[j] for j in range(n)])
            delta = FACTOR * xnorm
            if delta == 0:
                delta = FACTOR
        wa4 = fvec.copy()
        qtf = [0.0] * n
        for j in range(n):
            ajj = float(A[j, j])
            if ajj != 0:
                temp = -rsum(A[j, j:] * wa4[j:]) / ajj
                wa4[j:] += A[j, j:] * temp
            A[j, j] = rdiag[j]
            qtf[j] = float(wa4[j])
        R = [[float(A[j, i]) if i <= j else 0.0 for j in range(n)] for i in range(n)]
        gnorm = 0.0
        if fnorm != 0:
            for j in range(n):
                l = ipvt[j]
                if acnorm[l] != 0:
                    s = 0.0
                    for i in range(j + 1):
                        s += R[i][j] * (qtf[i] / fnorm)
                    gnorm = max(gnorm, abs(s / acnorm[l]))
        gnorms.append(gnorm)
        if gnorm <= GTOL:
            info = 4
            break
        while True:
            if capture:
                calls.append((np.array(R), np.array(ipvt), np.array(qtf), delta, par))
            par_in, delta_in = par, delta
            par, p, _, lit = lmpar(R, ipvt, diag, qtf, delta, par, mutant)
            wa1 = [-t for t in p]
            xtry = [x[j] + wa1[j] for j in range(n)]
            pnorm = enorm6([diag[j] * wa1[j] for j in range(n)])
            if it == 1 and pnorm < delta and mutant != "first_iter_delta_clip":
                delta = pnorm
            f1 = prob.resid(xtry)
            nfev += 1
            fnorm1 = math.sqrt(rsum(f1 * f1))
            actred = -1.0
            if 0.1 * fnorm1 < fnorm:
                q = fnorm1 / fnorm
                actred = 1 - q * q
            wa3 = [0.0] * n
            for j in range(n):
                temp = wa1[ipvt[j]]
                for i in range(j + 1):
                    wa3[i] += R[i][j] * temp
            temp1 = enorm6(wa3) / fnorm
            temp2 = (math.sqrt(par) * pnorm) / fnorm
            prered = temp1 * temp1 + temp2 * temp2 / 0.5
            dirder = -(temp1 * temp1 + temp2 * temp2)
            ratio = actred / prered if prered != 0 else 0.0
            log.append((par_in, delta_in, ratio, lit))
            if ratio <= 0.25:
                temp = 0.5 if actred >= 0 else 0.5 * dirder / (dirder + 0.5 * actred)
                if 0.1 * fnorm1 >= fnorm or temp < 0.1:
                    temp = 0.25 if mutant == "delta_shrink_quarter" else 0.1
                delta = temp * min(delta, pnorm / 0.1)
                if mutant != "par_div_missing":
                    par /= temp
            elif par == 0 or ratio >= 0.75:
                delta = pnorm / 0.5
                if mutant != "par_halve_missing":
                    par *= 0.5
            if ratio >= 1e-4:
                x = xtry
                xnorm = enorm6([diag[j] * x[j] for j in range(n)])
                fvec, fnorm = f1, fnorm1
                it += 1
            small = abs(actred) <= FTOL and prered <= FTOL and 0.5 * ratio <= 1
            if small:
                info = 1
            if delta <= XTOL * xnorm:
                info = 2
            if small and info == 2:
                info = 3
            if info == 0:
                if nfev >= MAXFEV:
                    info = 5
                if abs(actred) <= EPS and prered <= EPS and 0.5 * ratio <= 1:
                    info = 6
                if delta <= EPS * xnorm:
                    info = 7
                if gnorm <= EPS:
                    info = 8
            if info != 0 or not ratio < 1e-4:
                break
        if info != 0:
            break
    return Result(x=np.array(x), nfev=nfev, info=info, log=log, x0=np.array(prob.x0), r0=r0, cost=fnorm * fnorm, calls=calls, prob=prob,
                  gnorms=gnorms)
