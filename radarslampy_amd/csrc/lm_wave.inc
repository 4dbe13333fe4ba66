// mds_lm_wave_kernel: the motion-distortion solve (MotionDistortionSolver.optimize_library, motionDistortion.py:295-325 = MINPACK lmdif)
// as ONE WAVEFRONT per problem with the whole working set in registers.  Included by kabsch_mds.hip.
//
// Why (round 6): a lone solve of 150 points spent 0.42 ms in mds_lm_kernel, 61 % of it in the pivoted Householder QR and Q^T f of a
// 303 x 6 matrix (s_memtime ablation, profiles/r06_lm_experiments.txt): every one of the ~45 short steps of a factorisation is a round
// trip through LDS (the matrix), a reduction broadcast through LDS and two barriers, and the 6 x 6 trust-region algebra reads its
// operands from LDS one dependent load after the other.  Here
//   * lane t owns the "points" t, t + 64, ... (PPT of them): MINPACK rows 2 i and 2 i + 1 are the two residuals of point i; the three
//     velocity rows 2 N .. 2 N + 2 are the virtual points N (two rows) and N + 1 (one row and a row that stays zero), so that row
//     r lives in lane (r >> 1) & 63, slot r >> 7, component r & 1 - the pivot rows 0..5 are slot 0 of lanes 0..2;
//   * the Jacobian, fvec and Q^T f are register arrays with compile-time indices (the column swap of the pivoting is a chain of
//     wave-uniform `if`s over static register pairs); "rows >= j" is a predicate on slot 0 only;
//   * reductions are the DPP wave sum (every lane gets the result: no broadcast), and the dot products of a reflection with the
//     columns right of it are issued together (they do not depend on each other's updates);
//   * R, Q^T f, the pivot order and all of lmpar / qrsolv are wave-uniform register values computed by every lane alike: no LDS, no
//     barrier, no divergence.
// Same algorithm, same operations per entry as mds_lm_kernel (which stays for more than 254 points); only the grouping of the partial
// sums of a reduction differs (a lane adds ITS rows first), i.e. results agree to rounding, not bit for bit.

struct LmU { double I[6], ip0, ip1, iv0, iv1, iv2, period, Nn; };

__device__ __forceinline__ void lmw_vel_resid(const LmU &U, const double (&x)[6], double ct, double st, double (&out3)[3])
{
    const double tx = x[3], ty = x[4];
    const double m00 = U.I[0] * ct + U.I[1] * st, m10 = U.I[3] * ct + U.I[4] * st;
    const double mdx = U.I[0] * tx + U.I[1] * ty + U.I[2], mdy = U.I[3] * tx + U.I[4] * ty + U.I[5];
    const double dth = atan2(m10, m00);
    const double d0 = x[0] - mdx / U.period, d1 = x[1] - mdy / U.period;
    const double d2 = wrap_pi(x[2] - dth / U.period);
    out3[0] = U.iv0 * (d0 * U.Nn);
    out3[1] = U.iv1 * (d1 * U.Nn);
    out3[2] = U.iv2 * (d2 * U.Nn);
}

__device__ __forceinline__ double lmw_enorm6(const double (&v)[6])
{
    double s = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) s += v[i] * v[i];
    return sqrt(s);
}

// v[idx] for a wave-uniform idx without indexing the register array
__device__ __forceinline__ double lmw_sel6(const double (&v)[6], int idx)
{
    double r = v[0];
#pragma unroll
    for (int k = 1; k < 6; k++) r = idx == k ? v[k] : r;
    return r;
}

// x[ipvt[j]] = w[j]
__device__ __forceinline__ void lmw_scatter6(double (&x)[6], const int (&ipvt)[6], const double (&w)[6])
{
#pragma unroll
    for (int l = 0; l < 6; l++) {
        double r = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) r = ipvt[j] == l ? w[j] : r;
        x[l] = r;
    }
}

// qrsolv with diag = dval in every position (the solver's scaling vector is all ones: scipy's x_scale = 1, lmdif mode 2).
// R: upper triangle incl. diagonal; Tl: workspace, on exit its strict lower triangle holds S; sdiag: the diagonal of S
__device__ __forceinline__ void lmw_qrsolv(const double (&R)[6][6], double (&Tl)[6][6], const int (&ipvt)[6], double dval,
                                           const double (&qtb)[6], double (&x)[6], double (&sdiag)[6])
{
    double wa[6];
#pragma unroll
    for (int j = 0; j < 6; j++) {
#pragma unroll
        for (int i = j; i < 6; i++) Tl[i][j] = R[j][i];
        wa[j] = qtb[j];
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        if (dval != 0) {
#pragma unroll
            for (int k = j; k < 6; k++) sdiag[k] = 0;
            sdiag[j] = dval;
            double qtbpj = 0;
#pragma unroll
            for (int k = j; k < 6; k++) {
                if (sdiag[k] != 0) {
                    double c, s;
                    if (fabs(Tl[k][k]) < fabs(sdiag[k])) {
                        const double cot = Tl[k][k] / sdiag[k];
                        s = 0.5 / sqrt(0.25 + 0.25 * (cot * cot)); c = s * cot;
                    } else {
                        const double tn = sdiag[k] / Tl[k][k];
                        c = 0.5 / sqrt(0.25 + 0.25 * (tn * tn)); s = c * tn;
                    }
                    Tl[k][k] = c * Tl[k][k] + s * sdiag[k];
                    const double temp = c * wa[k] + s * qtbpj;
                    qtbpj = -s * wa[k] + c * qtbpj;
                    wa[k] = temp;
#pragma unroll
                    for (int i = k + 1; i < 6; i++) {
                        const double tt = c * Tl[i][k] + s * sdiag[i];
                        sdiag[i] = -s * Tl[i][k] + c * sdiag[i];
                        Tl[i][k] = tt;
                    }
                }
            }
        }
        sdiag[j] = Tl[j][j];
        Tl[j][j] = R[j][j];
    }
    int nsing = 6;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        if (sdiag[j] == 0 && nsing == 6) nsing = j;
        if (nsing < 6) wa[j] = 0;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int j = 5 - k;                                              // (= nsing - 1 - k of the columns below nsing)
        if (j < nsing) {
            double sum = 0;
#pragma unroll
            for (int i = j + 1; i < 6; i++)
                if (i < nsing) sum += Tl[i][j] * wa[i];
            wa[j] = (wa[j] - sum) / sdiag[j];
        }
    }
    lmw_scatter6(x, ipvt, wa);
}

__device__ __forceinline__ void lmw_lmpar(const double (&R)[6][6], double (&Tl)[6][6], const int (&ipvt)[6], const double (&qtb)[6],
                                          double delta, double &par, double (&x)[6], double (&sdiag)[6])
{
    double wa1[6], wa2[6];
    int nsing = 6;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        wa1[j] = qtb[j];
        if (R[j][j] == 0 && nsing == 6) nsing = j;
        if (nsing < 6) wa1[j] = 0;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int j = 5 - k;
        if (j < nsing) {
            wa1[j] /= R[j][j];
            const double temp = wa1[j];
#pragma unroll
            for (int i = 0; i < j; i++) wa1[i] -= R[i][j] * temp;
        }
    }
    lmw_scatter6(x, ipvt, wa1);
    int iter = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) wa2[j] = x[j];                           // diag = 1
    double dxnorm = lmw_enorm6(wa2);
    double fp = dxnorm - delta;
    if (fp <= 0.1 * delta) { par = 0; return; }
    double parl = 0;
    if (nsing >= 6) {
#pragma unroll
        for (int j = 0; j < 6; j++) wa1[j] = lmw_sel6(wa2, ipvt[j]) / dxnorm;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double sum = 0;
#pragma unroll
            for (int i = 0; i < j; i++) sum += R[i][j] * wa1[i];
            wa1[j] = (wa1[j] - sum) / R[j][j];
        }
        const double temp = lmw_enorm6(wa1);
        parl = ((fp / delta) / temp) / temp;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double sum = 0;
#pragma unroll
        for (int i = 0; i <= j; i++) sum += R[i][j] * qtb[i];
        wa1[j] = sum;                                                     // / diag[ipvt[j]] = 1
    }
    const double gnorm = lmw_enorm6(wa1);
    double paru = gnorm / delta;
    if (paru == 0) paru = DWARF / (delta < 0.1 ? delta : 0.1);
    if (par < parl) par = parl;
    if (par > paru) par = paru;
    if (par == 0) par = gnorm / dxnorm;
    for (;;) {
        iter++;
        if (par == 0) { const double tq = 0.001 * paru; par = DWARF > tq ? DWARF : tq; }
        double temp = sqrt(par);
        lmw_qrsolv(R, Tl, ipvt, temp, qtb, x, sdiag);
#pragma unroll
        for (int j = 0; j < 6; j++) wa2[j] = x[j];
        dxnorm = lmw_enorm6(wa2);
        temp = fp;
        fp = dxnorm - delta;
        if (fabs(fp) <= 0.1 * delta || (parl == 0 && fp <= temp && temp < 0) || iter == 10) break;
#pragma unroll
        for (int j = 0; j < 6; j++) wa1[j] = lmw_sel6(wa2, ipvt[j]) / dxnorm;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            wa1[j] /= sdiag[j];
            const double tq = wa1[j];
#pragma unroll
            for (int i = j + 1; i < 6; i++) wa1[i] -= Tl[i][j] * tq;
        }
        temp = lmw_enorm6(wa1);
        const double parc = ((fp / delta) / temp) / temp;
        if (fp > 0 && par > parl) parl = par;
        if (fp < 0 && par < paru) paru = par;
        const double np_ = par + parc;
        par = parl > np_ ? parl : np_;
    }
}

// the register budget is cut to two wavefronts per SIMD (the solve wants ~290 registers: in a batch that shares the CUs with other
// steps' kernels, resident waves are what counts - launch_mds_solve)
template <int PPT>
__global__ __launch_bounds__(64, 2) void mds_lm_wave_kernel(MdsProblemDesc P, double *__restrict__ out6, int32_t *__restrict__ nfev_out,
                                                         int32_t *__restrict__ info_out, double *__restrict__ x0_out,
                                                         double *__restrict__ r0_out)
{
    // the lane's own points (jt x, jt y, world x, world y, dT): written and read by the same lane only - a register file extension
    __shared__ double pts[5][64 * PPT];
    const int b = blockIdx.x, t = threadIdx.x;
    const int N = P.count ? min(P.count[b], P.nmax) : P.N;
    if (N + 2 > 64 * PPT) {                           // mds_lm_kernel's problem (launch_mds_solve)
        if (P.big && t == 0) {
            int32_t *L = P.big + (size_t)P.big_slot * (1 + P.B);
            L[1 + atomicAdd(L, 1)] = b;
        }
        return;
    }
    if (N < 2) {                                      // lmdif needs m >= n; the caller keeps the previous pose
        if (t == 0) { nfev_out[b] = 0; info_out[b] = -1; for (int j = 0; j < 6; j++) out6[(size_t)b * 6 + j] = 0.0; }
        return;
    }
    const int mmax = 2 * P.nmax + 3;
    const double *p_w = P.p_w + (size_t)b * P.nstride * 2;
    const double *p_jt = P.p_jt + (size_t)b * P.nstride * 2;
    const double *T0 = P.T_wj0 + (size_t)b * 9, *Ti = P.T_init + (size_t)b * 9;
    LmU U;
    double x[6];
    {
        const double ta = T0[0], tb = T0[1], tx = T0[2], tc = T0[3], td = T0[4], ty = T0[5];
        const double det = ta * td - tb * tc;
        U.I[0] = td / det; U.I[1] = -tb / det; U.I[3] = -tc / det; U.I[4] = ta / det;
        U.I[2] = -(U.I[0] * tx + U.I[1] * ty); U.I[5] = -(U.I[3] * tx + U.I[4] * ty);
        U.ip0 = 1 / P.sigma5[0]; U.ip1 = 1 / P.sigma5[1];
        U.iv0 = 1 / P.sigma5[2]; U.iv1 = 1 / P.sigma5[3]; U.iv2 = 1 / P.sigma5[4];
        U.period = P.period; U.Nn = (double)N;
        const double r00 = U.I[0] * Ti[0] + U.I[1] * Ti[3], r10 = U.I[3] * Ti[0] + U.I[4] * Ti[3];
        x[0] = (U.I[0] * Ti[2] + U.I[1] * Ti[5] + U.I[2]) / P.period;
        x[1] = (U.I[3] * Ti[2] + U.I[4] * Ti[5] + U.I[5]) / P.period;
        x[2] = atan2(r10, r00) / P.period;
        x[3] = Ti[2]; x[4] = Ti[5]; x[5] = atan2(Ti[3], Ti[0]);
    }
#pragma unroll
    for (int p = 0; p < PPT; p++) {
        const int i = t + 64 * p;
        double px = 0, py = 0, wx = 0, wy = 0, d = 0;
        if (i < N) {
            px = p_jt[2 * i]; py = p_jt[2 * i + 1]; wx = p_w[2 * i]; wy = p_w[2 * i + 1];
            d = P.period * atan2(-py, -px) / TWO_PI;
        }
        pts[0][p * 64 + t] = px; pts[1][p * 64 + t] = py; pts[2][p * 64 + t] = wx; pts[3][p * 64 + t] = wy; pts[4][p * 64 + t] = d;
    }
    if (x0_out && t < 6) {
#pragma unroll
        for (int j = 0; j < 6; j++) if (t == j) x0_out[(size_t)b * 6 + j] = x[j];
    }

    // error_vector (motionDistortion.py:162-205) at xx: the lane's rows -> f, the velocity residuals (uniform) -> v3
    auto resid = [&](const double (&xx)[6], double (&f)[PPT][2], double (&v3)[3]) {
        const double th = xx[5], tx = xx[3], ty = xx[4];
        const double ct = cos(th), st = sin(th);
        lmw_vel_resid(U, xx, ct, st, v3);
#pragma unroll
        for (int p = 0; p < PPT; p++) {
            const int i = t + 64 * p;
            double f0 = 0, f1 = 0;
            if (p * 64 < N) {                                             // (uniform: the slot holds points)
                const double px = pts[0][p * 64 + t], py = pts[1][p * 64 + t], pwx = pts[2][p * 64 + t], pwy = pts[3][p * 64 + t];
                const double d = pts[4][p * 64 + t];
                const double a = xx[2] * d, ddx = xx[0] * d, ddy = xx[1] * d;
                const double ca = cos(a), sa = sin(a);
                const double ux = ca * px - sa * py + ddx;
                const double uy = sa * px + ca * py + ddy;
                const double wx = pwx - tx, wy = pwy - ty;
                const double ex = ct * wx + st * wy;
                const double ey = -st * wx + ct * wy;
                const double nx = ex - ux, ny = ey - uy;
                f0 = U.ip0 * log(nx * nx / 2 + 1);
                f1 = U.ip1 * log(ny * ny / 2 + 1);
                if (i >= N) { f0 = 0; f1 = 0; }
            }
            if (i == N) { f0 = v3[0]; f1 = v3[1]; }
            if (i == N + 1) { f0 = v3[2]; f1 = 0; }
            f[p][0] = f0; f[p][1] = f1;
        }
    };
    auto sumsq = [&](const double (&f)[PPT][2]) {
        double s = 0;
#pragma unroll
        for (int p = 0; p < PPT; p++) { s += f[p][0] * f[p][0]; s += f[p][1] * f[p][1]; }
        return wave_sum_d(s);
    };

    double fvec[PPT][2], fvel[3];
    resid(x, fvec, fvel);
    if (r0_out) {
#pragma unroll
        for (int p = 0; p < PPT; p++) {
            const int i = t + 64 * p;
            if (i <= N) { r0_out[(size_t)b * mmax + 2 * i] = fvec[p][0]; r0_out[(size_t)b * mmax + 2 * i + 1] = fvec[p][1]; }
            if (i == N + 1) r0_out[(size_t)b * mmax + 2 * i] = fvec[p][0];
        }
    }
    double fnorm = sqrt(sumsq(fvec));
    const double eps = sqrt(EPSMCH);            // epsfcn = EPS -> sqrt(max(epsfcn, epsmch))
    int info = 0, nfev = 1, iter = 1, ipvt[6];
    double par = 0, delta = 0, xnorm = 0, gnorm = 0;
    double A[PPT][2][6];
#ifdef LM_TIMING
    unsigned long long tk[6] = {0, 0, 0, 0, 0, 0}, tl = __builtin_amdgcn_s_memtime(), tn;
#define LMW_TICK(k) { tn = __builtin_amdgcn_s_memtime(); tk[k] += tn - tl; tl = tn; }
#else
#define LMW_TICK(k)
#endif

    for (;;) {   // ------------------------------------------------ outer loop
        LMW_TICK(0)
        // ---- fdjac2 (see mds_jac: the six forward-difference columns with the shared subexpressions evaluated once)
        double xp[6], hh[6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double h = eps * fabs(x[j]);
            if (h == 0) h = eps;
            hh[j] = h;
            xp[j] = x[j] + h;
        }
        {
            const double tx = x[3], ty = x[4];
            const double ct0 = cos(x[5]), st0 = sin(x[5]);
            const double ct5 = cos(xp[5]), st5 = sin(xp[5]);
#pragma unroll
            for (int p = 0; p < PPT; p++) {
#pragma unroll
                for (int j = 0; j < 6; j++) { A[p][0][j] = 0; A[p][1][j] = 0; }
                if (p * 64 < N) {
                    const int i = t + 64 * p;
                    const double px = pts[0][p * 64 + t], py = pts[1][p * 64 + t], pwx = pts[2][p * 64 + t], pwy = pts[3][p * 64 + t];
                    const double d = pts[4][p * 64 + t];
                    const double f0x = fvec[p][0], f0y = fvec[p][1];
                    const double a0 = x[2] * d, a2 = xp[2] * d;
                    const double ca0 = cos(a0), sa0 = sin(a0), ca2 = cos(a2), sa2 = sin(a2);
                    const double rx0 = ca0 * px - sa0 * py, ry0 = sa0 * px + ca0 * py;
                    const double ux0 = rx0 + x[0] * d, uy0 = ry0 + x[1] * d;
                    const double wx0 = pwx - tx, wy0 = pwy - ty;
                    const double ex0 = ct0 * wx0 + st0 * wy0, ey0 = -st0 * wx0 + ct0 * wy0;
                    double nx, ny, q[2][6];
                    nx = ex0 - (rx0 + xp[0] * d);
                    q[0][0] = (U.ip0 * log(nx * nx / 2 + 1) - f0x) / hh[0];
                    q[1][0] = 0.0;
                    ny = ey0 - (ry0 + xp[1] * d);
                    q[0][1] = 0.0;
                    q[1][1] = (U.ip1 * log(ny * ny / 2 + 1) - f0y) / hh[1];
                    nx = ex0 - ((ca2 * px - sa2 * py) + x[0] * d);
                    ny = ey0 - ((sa2 * px + ca2 * py) + x[1] * d);
                    q[0][2] = (U.ip0 * log(nx * nx / 2 + 1) - f0x) / hh[2];
                    q[1][2] = (U.ip1 * log(ny * ny / 2 + 1) - f0y) / hh[2];
                    {
                        const double wx = pwx - xp[3];
                        nx = (ct0 * wx + st0 * wy0) - ux0;
                        ny = (-st0 * wx + ct0 * wy0) - uy0;
                        q[0][3] = (U.ip0 * log(nx * nx / 2 + 1) - f0x) / hh[3];
                        q[1][3] = (U.ip1 * log(ny * ny / 2 + 1) - f0y) / hh[3];
                    }
                    {
                        const double wy = pwy - xp[4];
                        nx = (ct0 * wx0 + st0 * wy) - ux0;
                        ny = (-st0 * wx0 + ct0 * wy) - uy0;
                        q[0][4] = (U.ip0 * log(nx * nx / 2 + 1) - f0x) / hh[4];
                        q[1][4] = (U.ip1 * log(ny * ny / 2 + 1) - f0y) / hh[4];
                    }
                    nx = (ct5 * wx0 + st5 * wy0) - ux0;
                    ny = (-st5 * wx0 + ct5 * wy0) - uy0;
                    q[0][5] = (U.ip0 * log(nx * nx / 2 + 1) - f0x) / hh[5];
                    q[1][5] = (U.ip1 * log(ny * ny / 2 + 1) - f0y) / hh[5];
                    if (i < N) {
#pragma unroll
                        for (int j = 0; j < 6; j++) { A[p][0][j] = q[0][j]; A[p][1][j] = q[1][j]; }
                    }
                }
            }
            // the velocity rows: lane 63 - j evaluates column j, the owners of the rows fetch the quotients
            const int jv = 63 - t;
            double xv[6], o3[3], dq[3];
#pragma unroll
            for (int k = 0; k < 6; k++) xv[k] = (k == jv) ? xp[k] : x[k];
            lmw_vel_resid(U, xv, jv == 5 ? ct5 : ct0, jv == 5 ? st5 : st0, o3);
            double hv = hh[0];
#pragma unroll
            for (int k = 1; k < 6; k++) hv = (k == jv) ? hh[k] : hv;
#pragma unroll
            for (int k = 0; k < 3; k++) dq[k] = (o3[k] - fvel[k]) / hv;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double c0 = readlane_d(dq[0], 63 - j), c1 = readlane_d(dq[1], 63 - j), c2 = readlane_d(dq[2], 63 - j);
#pragma unroll
                for (int p = 0; p < PPT; p++) {
                    const int i = t + 64 * p;
                    if (i == N) { A[p][0][j] = c0; A[p][1][j] = c1; }
                    if (i == N + 1) { A[p][0][j] = c2; A[p][1][j] = 0.0; }
                }
            }
        }
        nfev += 6;
        LMW_TICK(1)
        // ---- qrfac with column pivoting
        double rdiag[6], acnorm[6], wa3[6];
        {
            double s[6];
#pragma unroll
            for (int j = 0; j < 6; j++) {
                double sj = 0;
#pragma unroll
                for (int p = 0; p < PPT; p++) { sj += A[p][0][j] * A[p][0][j]; sj += A[p][1][j] * A[p][1][j]; }
                s[j] = sj;
            }
#pragma unroll
            for (int j = 0; j < 6; j++) { acnorm[j] = sqrt(wave_sum_d(s[j])); rdiag[j] = acnorm[j]; wa3[j] = acnorm[j]; ipvt[j] = j; }
        }
        double hjj[6];                                                    // the Householder vectors' leading entries (A(j,j) of qrfac's output)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const int pl = j >> 1, pc = j & 1;                            // the pivot row: lane pl, slot 0, component pc
            int kmax = j;
            double best = rdiag[j];
#pragma unroll
            for (int k = j + 1; k < 6; k++) if (rdiag[k] > best) { best = rdiag[k]; kmax = k; }
#pragma unroll
            for (int k = j + 1; k < 6; k++) {
                if (kmax == k) {                                          // (uniform)
#pragma unroll
                    for (int p = 0; p < PPT; p++) {
                        double tq = A[p][0][j]; A[p][0][j] = A[p][0][k]; A[p][0][k] = tq;
                        tq = A[p][1][j]; A[p][1][j] = A[p][1][k]; A[p][1][k] = tq;
                    }
                    rdiag[k] = rdiag[j]; wa3[k] = wa3[j];
                    const int tp = ipvt[j]; ipvt[j] = ipvt[k]; ipvt[k] = tp;
                }
            }
            const bool ge0 = 2 * t + 0 >= j, ge1 = 2 * t + 1 >= j;        // slot 0: is the row at or below the pivot row?
            double s = 0;
            s += ge0 ? A[0][0][j] * A[0][0][j] : 0.0;
            s += ge1 ? A[0][1][j] * A[0][1][j] : 0.0;
#pragma unroll
            for (int p = 1; p < PPT; p++) { s += A[p][0][j] * A[p][0][j]; s += A[p][1][j] * A[p][1][j]; }
            double ajnorm = sqrt(wave_sum_d(s));
            hjj[j] = 0;
            if (ajnorm != 0) {
                const double ajj0 = readlane_d(A[0][pc][j], pl);
                if (ajj0 < 0) ajnorm = -ajnorm;
                if (ge0) A[0][0][j] /= ajnorm;
                if (ge1) A[0][1][j] /= ajnorm;
#pragma unroll
                for (int p = 1; p < PPT; p++) { A[p][0][j] /= ajnorm; A[p][1][j] /= ajnorm; }
                if (t == pl) A[0][pc][j] += 1;
                const double ajj = ajj0 / ajnorm + 1;
                hjj[j] = ajj;
                double dots[6];
#pragma unroll
                for (int k = j + 1; k < 6; k++) {
                    double d = 0;
                    d += ge0 ? A[0][0][j] * A[0][0][k] : 0.0;
                    d += ge1 ? A[0][1][j] * A[0][1][k] : 0.0;
#pragma unroll
                    for (int p = 1; p < PPT; p++) { d += A[p][0][j] * A[p][0][k]; d += A[p][1][j] * A[p][1][k]; }
                    dots[k] = d;
                }
#pragma unroll
                for (int k = j + 1; k < 6; k++) dots[k] = wave_sum_d(dots[k]);
#pragma unroll
                for (int k = j + 1; k < 6; k++) {
                    const double temp = dots[k] / ajj;
                    if (ge0) A[0][0][k] -= temp * A[0][0][j];
                    if (ge1) A[0][1][k] -= temp * A[0][1][j];
#pragma unroll
                    for (int p = 1; p < PPT; p++) { A[p][0][k] -= temp * A[p][0][j]; A[p][1][k] -= temp * A[p][1][j]; }
                    // rdiag down-date
                    double rk = rdiag[k];
                    if (rk != 0) {
                        const double ajk = readlane_d(A[0][pc][k], pl);
                        const double tq = ajk / rk;
                        const double dd = 1 - tq * tq;
                        rk *= sqrt(dd > 0 ? dd : 0);
                        const double q = rk / wa3[k];
                        if (0.05 * (q * q) <= EPSMCH) {
                            const bool gt0 = 2 * t + 0 > j, gt1 = 2 * t + 1 > j;
                            double s2 = 0;
                            s2 += gt0 ? A[0][0][k] * A[0][0][k] : 0.0;
                            s2 += gt1 ? A[0][1][k] * A[0][1][k] : 0.0;
#pragma unroll
                            for (int p = 1; p < PPT; p++) { s2 += A[p][0][k] * A[p][0][k]; s2 += A[p][1][k] * A[p][1][k]; }
                            rk = sqrt(wave_sum_d(s2));
                            wa3[k] = rk;
                        }
                    }
                    rdiag[k] = rk;
                }
            }
            rdiag[j] = -ajnorm;
        }
        if (iter == 1) {
            xnorm = lmw_enorm6(x);                                        // diag = 1
            delta = 100.0 * xnorm;
            if (delta == 0) delta = 100.0;
        }
        LMW_TICK(2)
        // ---- Q^T fvec -> qtf, and R out of the pivot rows
        double qtf[6], R[6][6];
        {
            double w4[PPT][2];
#pragma unroll
            for (int p = 0; p < PPT; p++) { w4[p][0] = fvec[p][0]; w4[p][1] = fvec[p][1]; }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const int pl = j >> 1, pc = j & 1;
                const bool ge0 = 2 * t + 0 >= j, ge1 = 2 * t + 1 >= j;
                if (hjj[j] != 0) {
                    double sum = 0;
                    sum += ge0 ? A[0][0][j] * w4[0][0] : 0.0;
                    sum += ge1 ? A[0][1][j] * w4[0][1] : 0.0;
#pragma unroll
                    for (int p = 1; p < PPT; p++) { sum += A[p][0][j] * w4[p][0]; sum += A[p][1][j] * w4[p][1]; }
                    sum = wave_sum_d(sum);
                    const double temp = -sum / hjj[j];
                    if (ge0) w4[0][0] += A[0][0][j] * temp;
                    if (ge1) w4[0][1] += A[0][1][j] * temp;
#pragma unroll
                    for (int p = 1; p < PPT; p++) { w4[p][0] += A[p][0][j] * temp; w4[p][1] += A[p][1][j] * temp; }
                }
                qtf[j] = readlane_d(w4[0][pc], pl);
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
#pragma unroll
                for (int i = 0; i < 6; i++) R[i][j] = 0;
#pragma unroll
                for (int i = 0; i < j; i++) R[i][j] = readlane_d(A[0][i & 1][j], i >> 1);
                R[j][j] = rdiag[j];
            }
        }
        // ---- gradient norm
        gnorm = 0;
        if (fnorm != 0) {
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double an = lmw_sel6(acnorm, ipvt[j]);
                if (an != 0) {
                    double sum = 0;
#pragma unroll
                    for (int i = 0; i <= j; i++) sum += R[i][j] * (qtf[i] / fnorm);
                    const double g = fabs(sum / an);
                    if (g > gnorm) gnorm = g;
                }
            }
        }
        if (gnorm <= 1e-8) info = 4;
        LMW_TICK(3)
        if (info != 0) break;
        for (;;) {   // -------------------------------------------- inner loop
            double pv[6], sd[6], Tl[6][6], wa1[6], xtry[6];
            lmw_lmpar(R, Tl, ipvt, qtf, delta, par, pv, sd);
#pragma unroll
            for (int j = 0; j < 6; j++) { wa1[j] = -pv[j]; xtry[j] = x[j] + wa1[j]; }
            const double pnorm = lmw_enorm6(wa1);
            if (iter == 1 && pnorm < delta) delta = pnorm;
            LMW_TICK(4)
            double w4[PPT][2], v3[3];
            resid(xtry, w4, v3);
            const double fnorm1 = sqrt(sumsq(w4));
            nfev++;
            double actred = -1;
            if (0.1 * fnorm1 < fnorm) { const double r = fnorm1 / fnorm; actred = 1 - r * r; }
            double w3[6];
#pragma unroll
            for (int j = 0; j < 6; j++) w3[j] = 0;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double temp = lmw_sel6(wa1, ipvt[j]);
#pragma unroll
                for (int i = 0; i <= j; i++) w3[i] += R[i][j] * temp;
            }
            const double temp1 = lmw_enorm6(w3) / fnorm;
            const double temp2 = (sqrt(par) * pnorm) / fnorm;
            const double prered = temp1 * temp1 + temp2 * temp2 / 0.5;
            const double dirder = -(temp1 * temp1 + temp2 * temp2);
            double ratio = 0;
            if (prered != 0) ratio = actred / prered;
            if (ratio <= 0.25) {
                double temp;
                if (actred >= 0) temp = 0.5;
                else temp = 0.5 * dirder / (dirder + 0.5 * actred);
                if (0.1 * fnorm1 >= fnorm || temp < 0.1) temp = 0.1;
                const double dm = pnorm / 0.1;
                delta = temp * (delta < dm ? delta : dm);
                par /= temp;
            } else if (par == 0 || ratio >= 0.75) {
                delta = pnorm / 0.5;
                par *= 0.5;
            }
            if (ratio >= 1e-4) {
#pragma unroll
                for (int j = 0; j < 6; j++) x[j] = xtry[j];
                xnorm = lmw_enorm6(x);
                fnorm = fnorm1;
                iter++;
#pragma unroll
                for (int p = 0; p < PPT; p++) { fvec[p][0] = w4[p][0]; fvec[p][1] = w4[p][1]; }
#pragma unroll
                for (int k = 0; k < 3; k++) fvel[k] = v3[k];
            }
            info = 0;
            if (fabs(actred) <= 1e-8 && prered <= 1e-8 && 0.5 * ratio <= 1) info = 1;
            if (delta <= 1e-8 * xnorm) info = 2;
            if (fabs(actred) <= 1e-8 && prered <= 1e-8 && 0.5 * ratio <= 1 && info == 2) info = 3;
            if (info == 0) {
                if (nfev >= 100 * 6 * 7) info = 5;
                if (fabs(actred) <= EPSMCH && prered <= EPSMCH && 0.5 * ratio <= 1) info = 6;
                if (delta <= EPSMCH * xnorm) info = 7;
                if (gnorm <= EPSMCH) info = 8;
            }
            LMW_TICK(5)
            if (info != 0 || !(ratio < 1e-4)) break;
        }
        if (info != 0) break;
    }
#ifdef LM_TIMING
    if (x0_out && t == 0) for (int k = 0; k < 6; k++) x0_out[(size_t)b * 6 + k] = (double)tk[k];
#endif
#pragma unroll
    for (int j = 0; j < 6; j++) if (t == j) out6[(size_t)b * 6 + j] = x[j];
    if (t == 0) { nfev_out[b] = nfev; info_out[b] = info; }
}
