// qrsolv and lmpar of the workgroup form (mds_lm_kernel).  Included by kabsch_mds.hip with LM6(name) naming the two functions: once
// for the solver, and once more as the copy lm_debug_lmpar_kernel runs - a second caller of the solver's own functions would change how
// the compiler inlines them into mds_lm_kernel, and with that the kernel's machine code.
// serial 6x6 pieces (thread 0 only), operating on the first 6 rows of `a`
__device__ void LM6(qrsolv6)(int m, double *a, const int *ipvt, const double *diag, const double *qtb,
                        double *x, double *sdiag, double *wa)
{
    const int n = 6;
    for (int j = 0; j < n; j++) {
        for (int i = j; i < n; i++) A_(i, j) = A_(j, i);
        x[j] = A_(j, j); wa[j] = qtb[j];
    }
    for (int j = 0; j < n; j++) {
        const int l = ipvt[j];
        if (diag[l] != 0) {
            for (int k = j; k < n; k++) sdiag[k] = 0;
            sdiag[j] = diag[l];
            double qtbpj = 0;
            for (int k = j; k < n; k++) {
                if (sdiag[k] == 0) continue;
                double c, s;
                if (fabs(A_(k, k)) < fabs(sdiag[k])) {
                    double cot = A_(k, k) / sdiag[k];
                    s = 0.5 / sqrt(0.25 + 0.25 * (cot * cot)); c = s * cot;
                } else {
                    double t = sdiag[k] / A_(k, k);
                    c = 0.5 / sqrt(0.25 + 0.25 * (t * t)); s = c * t;
                }
                A_(k, k) = c * A_(k, k) + s * sdiag[k];
                double temp = c * wa[k] + s * qtbpj;
                qtbpj = -s * wa[k] + c * qtbpj;
                wa[k] = temp;
                for (int i = k + 1; i < n; i++) {
                    temp = c * A_(i, k) + s * sdiag[i];
                    sdiag[i] = -s * A_(i, k) + c * sdiag[i];
                    A_(i, k) = temp;
                }
            }
        }
        sdiag[j] = A_(j, j);
        A_(j, j) = x[j];
    }
    int nsing = n;
    for (int j = 0; j < n; j++) {
        if (sdiag[j] == 0 && nsing == n) nsing = j;
        if (nsing < n) wa[j] = 0;
    }
    for (int k = 0; k < nsing; k++) {
        const int j = nsing - 1 - k;
        double sum = 0;
        for (int i = j + 1; i < nsing; i++) sum += A_(i, j) * wa[i];
        wa[j] = (wa[j] - sum) / sdiag[j];
    }
    for (int j = 0; j < n; j++) x[ipvt[j]] = wa[j];
}

__device__ void LM6(lmpar6)(int m, double *a, const int *ipvt, const double *diag, const double *qtb,
                       double delta, double *par, double *x, double *sdiag, double *wa1, double *wa2)
{
    const int n = 6;
    int nsing = n;
    for (int j = 0; j < n; j++) {
        wa1[j] = qtb[j];
        if (A_(j, j) == 0 && nsing == n) nsing = j;
        if (nsing < n) wa1[j] = 0;
    }
    for (int k = 0; k < nsing; k++) {
        const int j = nsing - 1 - k;
        wa1[j] /= A_(j, j);
        const double temp = wa1[j];
        for (int i = 0; i < j; i++) wa1[i] -= A_(i, j) * temp;
    }
    for (int j = 0; j < n; j++) x[ipvt[j]] = wa1[j];
    int iter = 0;
    for (int j = 0; j < n; j++) wa2[j] = diag[j] * x[j];
    double dxnorm = enorm6(wa2);
    double fp = dxnorm - delta;
    if (fp <= 0.1 * delta) { *par = 0; return; }
    double parl = 0;
    if (nsing >= n) {
        for (int j = 0; j < n; j++) { const int l = ipvt[j]; wa1[j] = diag[l] * (wa2[l] / dxnorm); }
        for (int j = 0; j < n; j++) {
            double sum = 0;
            for (int i = 0; i < j; i++) sum += A_(i, j) * wa1[i];
            wa1[j] = (wa1[j] - sum) / A_(j, j);
        }
        const double temp = enorm6(wa1);
        parl = ((fp / delta) / temp) / temp;
    }
    for (int j = 0; j < n; j++) {
        double sum = 0;
        for (int i = 0; i <= j; i++) sum += A_(i, j) * qtb[i];
        wa1[j] = sum / diag[ipvt[j]];
    }
    const double gnorm = enorm6(wa1);
    double paru = gnorm / delta;
    if (paru == 0) paru = DWARF / (delta < 0.1 ? delta : 0.1);
    if (*par < parl) *par = parl;
    if (*par > paru) *par = paru;
    if (*par == 0) *par = gnorm / dxnorm;
    for (;;) {
        iter++;
        if (*par == 0) { const double t = 0.001 * paru; *par = DWARF > t ? DWARF : t; }
        double temp = sqrt(*par);
        for (int j = 0; j < n; j++) wa1[j] = temp * diag[j];
        LM6(qrsolv6)(m, a, ipvt, wa1, qtb, x, sdiag, wa2);
        for (int j = 0; j < n; j++) wa2[j] = diag[j] * x[j];
        dxnorm = enorm6(wa2);
        temp = fp;
        fp = dxnorm - delta;
        if (fabs(fp) <= 0.1 * delta || (parl == 0 && fp <= temp && temp < 0) || iter == 10) break;
        for (int j = 0; j < n; j++) { const int l = ipvt[j]; wa1[j] = diag[l] * (wa2[l] / dxnorm); }
        for (int j = 0; j < n; j++) {
            wa1[j] /= sdiag[j];
            const double t = wa1[j];
            for (int i = j + 1; i < n; i++) wa1[i] -= A_(i, j) * t;
        }
        temp = enorm6(wa1);
        const double parc = ((fp / delta) / temp) / temp;
        if (fp > 0 && *par > parl) parl = *par;
        if (fp < 0 && *par < paru) paru = *par;
        const double np_ = *par + parc;
        *par = parl > np_ ? parl : np_;
    }
}
