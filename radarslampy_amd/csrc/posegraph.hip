// Batched SE(2) pose-graph optimisation (reference PoseGraphLib.py: g2o's SparseOptimizer with OptimizationAlgorithmLevenberg over
// VertexSE2 / EdgeSE2; the project is 2-D throughout).  Kernels, launcher and the two ABI entries of the unit.
//
// One workgroup of PG_THREADS lanes per graph, all graphs of a chunk in one launch, the whole Levenberg-Marquardt loop inside the
// kernel: linearisation, chi2, the block envelope Cholesky of H + lambda I, the two triangular solves, the trial update and
// accept / reject.  Every loop is bounded by a count the host computed (max_iterations, max_trials, the envelope); nothing waits on data.
//
// The matrix.  The free vertices of a graph are numbered in their given order (no reordering).  Block row k of H (3 x 3 blocks)
// is stored from its lowest-numbered free neighbour first[k] to the diagonal - the envelope (skyline), which the Cholesky factor
// fills and never leaves.  The cost of a graph is therefore its envelope: about the vertex count plus the sum of j - i over its
// non-consecutive edges, in blocks of 72 bytes (two copies: H and the factor), and in the worst case the square of a row's length
// in operations.  The factorisation is right-looking by block column c: its rows are the list col(c) = {k > c : first[k] <= c}, which
// the host builds; the diagonal block is factored (by every lane, redundantly: the decision "pivot not positive" is then uniform),
// the lanes scale the blocks (k, c), then the pairs (k, j) of col(c) take their update - each block has one writer per column, in
// column order, so the sums have one order whatever the batch.  The solves are column-oriented forward and row-oriented backward for
// the same reason.  The linearisation runs the lanes over the free vertices, each gathering its own incident edges in list order
// (no atomics): vertex k writes its diagonal block, its part of b and the blocks (k, j) of its lower-numbered neighbours.
//
// All arithmetic is float64 and un-contracted; a graph's operations do not depend on the batch, so its result is the same bits
// alone, anywhere in a batch and in any chunk.
#include "roam_internal.h"
#include <math.h>
#include <stdlib.h>

#define PG_THREADS 256
#define PG_MAX_GRAPHS 65535
#define PG_MAX_VERTICES 32768
#define PG_MAX_ITERATIONS 1000
#define PG_MAX_TRIALS 1000
#define PG_CHUNK_BYTES ((int64_t)2000 << 20)     // scratch of one launch, as in the other batched stages
#define PG_CHUNK_ENV "ROAM_POSE_GRAPH_CHUNK_BYTES"      // the tests' smaller figure

// One graph of a chunk.  i_*: offsets into the chunk's int32 slab, d_*: into its float64 slab; v0 / e0: first vertex / edge of the
// graph in the chunk's pose and edge arrays
struct PgDesc {
    int32_t V, F, E, env;
    int64_t v0, e0;
    int64_t i_cidx;      // V: free index of a vertex, -1 = fixed
    int64_t i_fv;        // F: vertex of a free index
    int64_t i_first;     // F: first block column of row k
    int64_t i_rowoff;    // F + 1: first block of row k in the envelope
    int64_t i_colptr;    // F + 1: col(c) = colrows[colptr[c] .. colptr[c + 1])
    int64_t i_colrows;   // env - F
    int64_t i_incptr;    // F + 1: the edges at free vertex k, ascending
    int64_t i_inc;
    int64_t d_H, d_W;    // env x 9 each: H of the linearisation, H + lambda I and then its factor (strictly lower blocks)
    int64_t d_LD;        // F x 6: the factors of the diagonal blocks {l00 l10 l11 l20 l21 l22}
    int64_t d_b, d_d, d_y;   // F x 3 each: b, right-hand side and then the step, the forward solve's result
    int64_t d_xold;      // V x 3
};

struct PgEdges {
    const int32_t *ij;
    const double *meas, *info, *huber;
};

// ---------------------------------------------------------------------------------------------------------------- device
// EdgeSE2: e = [R(z_th)^T (R(th_i)^T (t_j - t_i) - z_t); normalize(th_j - th_i - z_th)] and, on request, A = de/dx_i, B = de/dx_j
__device__ static void pg_edge(const double *xi, const double *xj, const double *z, double *e, double *A, double *B, bool jac)
{
    double s, c, sz, cz;
    sincos(xi[2], &s, &c);
    sincos(z[2], &sz, &cz);
    const double dx = xj[0] - xi[0], dy = xj[1] - xi[1];
    const double ux = (c * dx + s * dy) - z[0], uy = (c * dy - s * dx) - z[1];
    e[0] = cz * ux + sz * uy;
    e[1] = cz * uy - sz * ux;
    e[2] = roam_normalize_angle((xj[2] - xi[2]) - z[2]);
    if (!jac) return;
    const double a0[6] = {-c, -s, c * dy - s * dx, s, -c, -(c * dx) - s * dy};     // rows 0 and 1 of dE/dx_i before Z
    const double b0[6] = {c, s, 0.0, -s, c, 0.0};
    for (int m = 0; m < 3; ++m) {
        A[m] = cz * a0[m] + sz * a0[3 + m];
        A[3 + m] = cz * a0[3 + m] - sz * a0[m];
        B[m] = cz * b0[m] + sz * b0[3 + m];
        B[3 + m] = cz * b0[3 + m] - sz * b0[m];
    }
    A[6] = 0.0; A[7] = 0.0; A[8] = -1.0;
    B[6] = 0.0; B[7] = 0.0; B[8] = 1.0;
}

// O (3 x 3 symmetric from {xx xy xt yy yt tt}) times a 3 x n matrix M (row-major, n = 1 or 3)
__device__ static void pg_info_mul(const double *o, const double *M, int n, double *out)
{
    for (int cidx = 0; cidx < n; ++cidx) {
        const double m0 = M[cidx], m1 = M[n + cidx], m2 = M[2 * n + cidx];
        out[cidx] = (o[0] * m0 + o[1] * m1) + o[2] * m2;
        out[n + cidx] = (o[1] * m0 + o[3] * m1) + o[4] * m2;
        out[2 * n + cidx] = (o[2] * m0 + o[4] * m1) + o[5] * m2;
    }
}

// Huber: s2 = e^T O e -> rho, weight
__device__ static void pg_robust(double s2, double delta, double *rho, double *w)
{
    if (delta > 0.0 && s2 > delta * delta) {
        const double sq = sqrt(s2);
        *rho = 2.0 * delta * sq - delta * delta;
        *w = delta / sq;
    } else {
        *rho = s2;
        *w = 1.0;
    }
}

// acc (3 x 3) += w * J1^T M2, M2 = O J2
__device__ static void pg_add_jtm(double *acc, const double *J1, const double *M2, double w)
{
    for (int r = 0; r < 3; ++r)
        for (int cidx = 0; cidx < 3; ++cidx)
            acc[3 * r + cidx] += w * ((J1[r] * M2[cidx] + J1[3 + r] * M2[3 + cidx]) + J1[6 + r] * M2[6 + cidx]);
}

// the fixed-shape tree: every lane returns the same sum / maximum
__device__ static double pg_block_sum(double v, double *red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int h = PG_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[t] = red[t] + red[t + h];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ static double pg_block_max(double v, double *red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int h = PG_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[t] = fmax(red[t], red[t + h]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// chi2 = sum of rho over the edges at the poses x: lane t takes the edges t, t + PG_THREADS, ... in order, then the tree
__device__ static double pg_chi2(const PgDesc &g, const PgEdges &ed, const double *x, double *red)
{
    double acc = 0.0;
    for (int t = threadIdx.x; t < g.E; t += PG_THREADS) {
        const int64_t q = g.e0 + t;
        double e[3], oe[3], rho, w;
        pg_edge(x + 3 * ed.ij[2 * q], x + 3 * ed.ij[2 * q + 1], ed.meas + 3 * q, e, nullptr, nullptr, false);
        pg_info_mul(ed.info + 6 * q, e, 1, oe);
        pg_robust((e[0] * oe[0] + e[1] * oe[1]) + e[2] * oe[2], ed.huber[q], &rho, &w);
        acc += rho;
    }
    return pg_block_sum(acc, red);
}

__global__ __launch_bounds__(PG_THREADS) void pose_graph_lm_kernel(const PgDesc *descs, const int32_t *ints, double *dbl, double *poses,
                                                                    PgEdges ed, roam_pose_graph_opts opts, roam_pose_graph_stats *stats)
{
    __shared__ double red[PG_THREADS];
    const PgDesc g = descs[blockIdx.x];
    const int tid = threadIdx.x;
    const int F = g.F;
    double *x = poses + 3 * g.v0;
    const int32_t *cidx = ints + g.i_cidx, *fv = ints + g.i_fv, *first = ints + g.i_first, *rowoff = ints + g.i_rowoff;
    const int32_t *colptr = ints + g.i_colptr, *colrows = ints + g.i_colrows, *incptr = ints + g.i_incptr, *inc = ints + g.i_inc;
    double *H = dbl + g.d_H, *W = dbl + g.d_W, *LD = dbl + g.d_LD, *bv = dbl + g.d_b, *dv = dbl + g.d_d, *yv = dbl + g.d_y;
    double *xold = dbl + g.d_xold;

    double cur = pg_chi2(g, ed, x, red);
    const double chi2_initial = cur;
    double lambda = 0.0, ni = 2.0;
    int iterations = 0, trials = 0, rejected = 0, stop = 0;
    const int max_it = (F > 0 && g.E > 0) ? opts.max_iterations : 0;
    const int max_trials = opts.max_trials > 0 ? opts.max_trials : 10;
    const int64_t nH = (int64_t)g.env * 9;

    for (int it = 0; it < max_it; ++it) {
        // ---- linearise at x
        for (int64_t q = tid; q < nH; q += PG_THREADS) H[q] = 0.0;
        __syncthreads();
        for (int k = tid; k < F; k += PG_THREADS) {
            const int v = fv[k];
            double hd[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bk[3] = {0, 0, 0};
            for (int p = incptr[k]; p < incptr[k + 1]; ++p) {
                const int64_t q = g.e0 + inc[p];
                const int vi = ed.ij[2 * q], vj = ed.ij[2 * q + 1];
                double e[3], A[9], B[9], oe[3], rho, w;
                pg_edge(x + 3 * vi, x + 3 * vj, ed.meas + 3 * q, e, A, B, true);
                pg_info_mul(ed.info + 6 * q, e, 1, oe);
                pg_robust((e[0] * oe[0] + e[1] * oe[1]) + e[2] * oe[2], ed.huber[q], &rho, &w);
                const double *Jk = (v == vi) ? A : B, *Jo = (v == vi) ? B : A;     // this vertex's Jacobian, the other end's
                const int ko = cidx[(v == vi) ? vj : vi];
                double M[9];
                pg_info_mul(ed.info + 6 * q, Jk, 3, M);
                pg_add_jtm(hd, Jk, M, w);
                for (int r = 0; r < 3; ++r) bk[r] -= w * ((Jk[r] * oe[0] + Jk[3 + r] * oe[1]) + Jk[6 + r] * oe[2]);
                if (ko >= 0 && ko < k) {
                    pg_info_mul(ed.info + 6 * q, Jo, 3, M);
                    pg_add_jtm(H + ((int64_t)rowoff[k] + (ko - first[k])) * 9, Jk, M, w);
                }
            }
            double *D = H + ((int64_t)rowoff[k + 1] - 1) * 9;
            for (int r = 0; r < 9; ++r) D[r] = hd[r];
            for (int r = 0; r < 3; ++r) bv[3 * k + r] = bk[r];
        }
        __syncthreads();
        if (it == 0) {
            if (opts.lambda_init > 0.0) {
                lambda = opts.lambda_init;
            } else {
                double m = 0.0;
                for (int k = tid; k < F; k += PG_THREADS) {
                    const double *D = H + ((int64_t)rowoff[k + 1] - 1) * 9;
                    m = fmax(m, fmax(D[0], fmax(D[4], D[8])));
                }
                lambda = 1e-5 * pg_block_max(m, red);
            }
        }

        // ---- trials
        double rho = 0.0;
        bool accepted = false;
        int q = 0;
        while (q < max_trials) {
            for (int64_t p = tid; p < nH; p += PG_THREADS) W[p] = H[p];
            for (int p = tid; p < 3 * F; p += PG_THREADS) dv[p] = bv[p];
            __syncthreads();
            for (int k = tid; k < F; k += PG_THREADS) {
                double *D = W + ((int64_t)rowoff[k + 1] - 1) * 9;
                D[0] += lambda; D[4] += lambda; D[8] += lambda;
            }
            __syncthreads();
            // block envelope Cholesky, right-looking by column
            bool fail = false;
            for (int c = 0; c < F; ++c) {
                const double *D = W + ((int64_t)rowoff[c + 1] - 1) * 9;
                const double d00 = D[0], d10 = D[3], d11 = D[4], d20 = D[6], d21 = D[7], d22 = D[8];
                bool ok = d00 > 0.0 && isfinite(d00);
                const double l00 = sqrt(d00), l10 = d10 / l00, l20 = d20 / l00;
                const double t11 = d11 - l10 * l10;
                ok = ok && t11 > 0.0 && isfinite(t11);
                const double l11 = sqrt(t11), l21 = (d21 - l20 * l10) / l11;
                const double t22 = (d22 - l20 * l20) - l21 * l21;
                ok = ok && t22 > 0.0 && isfinite(t22);
                const double l22 = sqrt(t22);
                if (!ok) { fail = true; break; }        // every lane read the same block: uniform
                if (tid == 0) {
                    double *o = LD + 6 * (int64_t)c;
                    o[0] = l00; o[1] = l10; o[2] = l11; o[3] = l20; o[4] = l21; o[5] = l22;
                }
                const int32_t *rows = colrows + colptr[c];
                const int s = colptr[c + 1] - colptr[c];
                for (int a = tid; a < s; a += PG_THREADS) {       // L(k, c) = A(k, c) L(c, c)^-T
                    const int k = rows[a];
                    double *Bk = W + ((int64_t)rowoff[k] + (c - first[k])) * 9;
                    for (int r = 0; r < 3; ++r) {
                        const double x0 = Bk[3 * r] / l00;
                        const double x1 = (Bk[3 * r + 1] - x0 * l10) / l11;
                        const double x2 = ((Bk[3 * r + 2] - x0 * l20) - x1 * l21) / l22;
                        Bk[3 * r] = x0; Bk[3 * r + 1] = x1; Bk[3 * r + 2] = x2;
                    }
                }
                __syncthreads();
                const int64_t npair = (int64_t)s * s;
                for (int64_t p = tid; p < npair; p += PG_THREADS) {     // A(k, j) -= L(k, c) L(j, c)^T, j <= k both in col(c)
                    const int a = (int)(p / s), bq = (int)(p % s);
                    if (bq > a) continue;
                    const int k = rows[a], j = rows[bq];
                    const double *Lk = W + ((int64_t)rowoff[k] + (c - first[k])) * 9;
                    const double *Lj = W + ((int64_t)rowoff[j] + (c - first[j])) * 9;
                    double *T = W + ((int64_t)rowoff[k] + (j - first[k])) * 9;
                    for (int r = 0; r < 3; ++r)
                        for (int u = 0; u < 3; ++u)
                            T[3 * r + u] -= (Lk[3 * r] * Lj[3 * u] + Lk[3 * r + 1] * Lj[3 * u + 1]) + Lk[3 * r + 2] * Lj[3 * u + 2];
                }
                __syncthreads();
            }
            // a failed column leaves the loop between its read of the diagonal block and any barrier: no lane goes on to write W
            // (the next trial's copy) before every lane has read that block and taken the same branch
            __syncthreads();
            double tmp = INFINITY, scale = 1e-3;
            if (!fail) {
                // forward: L y = b, by column
                for (int c = 0; c < F; ++c) {
                    const double *l = LD + 6 * (int64_t)c;
                    const double y0 = dv[3 * c] / l[0];
                    const double y1 = (dv[3 * c + 1] - l[1] * y0) / l[2];
                    const double y2 = ((dv[3 * c + 2] - l[3] * y0) - l[4] * y1) / l[5];
                    if (tid == 0) { yv[3 * c] = y0; yv[3 * c + 1] = y1; yv[3 * c + 2] = y2; }
                    const int32_t *rows = colrows + colptr[c];
                    const int s = colptr[c + 1] - colptr[c];
                    for (int a = tid; a < s; a += PG_THREADS) {
                        const int k = rows[a];
                        const double *Lk = W + ((int64_t)rowoff[k] + (c - first[k])) * 9;
                        for (int r = 0; r < 3; ++r)
                            dv[3 * k + r] -= (Lk[3 * r] * y0 + Lk[3 * r + 1] * y1) + Lk[3 * r + 2] * y2;
                    }
                    __syncthreads();
                }
                // backward: L^T delta = y, by row
                for (int k = F - 1; k >= 0; --k) {
                    const double *l = LD + 6 * (int64_t)k;
                    const double x2 = yv[3 * k + 2] / l[5];
                    const double x1 = (yv[3 * k + 1] - l[4] * x2) / l[2];
                    const double x0 = ((yv[3 * k] - l[1] * x1) - l[3] * x2) / l[0];
                    if (tid == 0) { dv[3 * k] = x0; dv[3 * k + 1] = x1; dv[3 * k + 2] = x2; }
                    const double *Lrow = W + (int64_t)rowoff[k] * 9;
                    for (int c = first[k] + tid; c < k; c += PG_THREADS) {
                        const double *Lk = Lrow + (int64_t)(c - first[k]) * 9;
                        for (int u = 0; u < 3; ++u)
                            yv[3 * c + u] -= (Lk[u] * x0 + Lk[3 + u] * x1) + Lk[6 + u] * x2;
                    }
                    __syncthreads();
                }
                // the trial step (VertexSE2::oplus) and its chi2
                double part = 0.0;
                for (int p = tid; p < 3 * F; p += PG_THREADS) part += dv[p] * (lambda * dv[p] + bv[p]);
                for (int p = tid; p < 3 * g.V; p += PG_THREADS) xold[p] = x[p];
                __syncthreads();
                for (int k = tid; k < F; k += PG_THREADS) {
                    double *xv = x + 3 * fv[k];
                    xv[0] += dv[3 * k];
                    xv[1] += dv[3 * k + 1];
                    xv[2] = roam_normalize_angle(xv[2] + dv[3 * k + 2]);
                }
                __syncthreads();
                scale = pg_block_sum(part, red) + 1e-3;
                tmp = pg_chi2(g, ed, x, red);
            }
            rho = (cur - tmp) / scale;
            ++trials;
            ++q;
            if (rho > 0.0 && isfinite(tmp)) {
                const double a = 2.0 * rho - 1.0;
                lambda *= fmax(1.0 / 3.0, fmin(1.0 - a * a * a, 2.0 / 3.0));
                ni = 2.0;
                cur = tmp;
                accepted = true;
                break;
            }
            lambda *= ni;
            ni *= 2.0;
            ++rejected;
            if (!fail) {
                for (int p = tid; p < 3 * g.V; p += PG_THREADS) x[p] = xold[p];
                __syncthreads();
            }
            if (rho == 0.0 || !isfinite(lambda)) break;
        }
        ++iterations;
        if (!isfinite(lambda)) { stop = 2; break; }
        if (!accepted) { stop = 1; break; }      // the trials ran out, or rho == 0
    }
    if (tid == 0) {
        roam_pose_graph_stats s;
        s.iterations = iterations; s.trials = trials; s.rejected = rejected; s.stop = stop;
        s.chi2_initial = chi2_initial; s.chi2_final = cur; s.lambda_final = lambda;
        stats[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
// What the host half makes of one graph: the free numbering, the envelope, the column lists and the incidence lists
struct PgGraphPlan {
    int V = 0, F = 0, E = 0;
    int64_t env = 0, nnz = 0;
    std::vector<int32_t> cidx, fv, first;
};

static int64_t pg_graph_bytes(const PgGraphPlan &p)
{
    const int64_t V = p.V, F = p.F, E = p.E;
    const int64_t dbl = 18 * p.env + 6 * F + 9 * F + 3 * V /* xold */ + 3 * V /* poses */ + 10 * E;
    const int64_t ints = V + 2 * F + 3 * (F + 1) + (p.env - F) + p.nnz + 2 * E;
    return 8 * dbl + 4 * ints + (int64_t)sizeof(PgDesc) + (int64_t)sizeof(roam_pose_graph_stats) + 64;
}

#define PG_FAIL(...) do { if (err) snprintf(err, cap, __VA_ARGS__); return ROAM_E_ARG; } while (0)

// structure of graph g: checks, compaction, envelope (no list is built here: a graph that is too large is refused first)
static int32_t pg_plan_graph(char *err, size_t cap, int g, int V, int E, const uint8_t *fixed, const int32_t *ij, PgGraphPlan *out)
{
    PgGraphPlan &p = *out;
    p.V = V; p.E = E; p.F = 0;
    p.cidx.assign(V, -1);
    p.fv.clear();
    for (int v = 0; v < V; ++v)
        if (!fixed[v]) { p.cidx[v] = p.F++; p.fv.push_back(v); }
    if (p.F == V) PG_FAIL("pose graph %d: no fixed vertex", g);
    p.first.resize(p.F);
    for (int k = 0; k < p.F; ++k) p.first[k] = k;
    p.nnz = 0;
    for (int t = 0; t < E; ++t) {
        const int i = ij[2 * t], j = ij[2 * t + 1];
        if (i < 0 || i >= V || j < 0 || j >= V) PG_FAIL("pose graph %d, edge %d: vertex index (%d, %d) outside [0, %d)", g, t, i, j, V);
        if (i == j) PG_FAIL("pose graph %d, edge %d: both ends are vertex %d", g, t, i);
        const int ki = p.cidx[i], kj = p.cidx[j];
        p.nnz += (ki >= 0) + (kj >= 0);
        if (ki >= 0 && kj >= 0) {
            const int hi = ki > kj ? ki : kj, lo = ki > kj ? kj : ki;
            if (lo < p.first[hi]) p.first[hi] = lo;
        }
    }
    p.env = 0;
    for (int k = 0; k < p.F; ++k) p.env += k - p.first[k] + 1;
    const int64_t bytes = pg_graph_bytes(p);
    if (bytes > PG_CHUNK_BYTES)
        PG_FAIL("pose graph %d: an envelope of %lld blocks needs %lld bytes of scratch, more than the %lld of a launch (no reordering: "
                "the envelope is the vertex count plus the span of every loop edge)", g, (long long)p.env, (long long)bytes,
                (long long)PG_CHUNK_BYTES);
    return ROAM_OK;
}

static int32_t pg_plan_all(char *err, size_t cap, int32_t n_graphs, const int32_t *vertex_off, const uint8_t *fixed, const int32_t *edge_off,
                           const int32_t *edge_ij, std::vector<PgGraphPlan> *plans)
{
    if (n_graphs < 1 || n_graphs > PG_MAX_GRAPHS) PG_FAIL("pose graph: 1 to %d graphs, not %d", PG_MAX_GRAPHS, n_graphs);
    if (!vertex_off || !fixed || !edge_off) PG_FAIL("pose graph: a null pointer");
    if (vertex_off[0] != 0 || edge_off[0] != 0) PG_FAIL("pose graph: offsets start at 0");
    plans->resize(n_graphs);
    for (int g = 0; g < n_graphs; ++g) {
        const int64_t V = (int64_t)vertex_off[g + 1] - vertex_off[g], E = (int64_t)edge_off[g + 1] - edge_off[g];
        if (V < 1 || V > PG_MAX_VERTICES) PG_FAIL("pose graph %d: 1 to %d vertices, not %lld", g, PG_MAX_VERTICES, (long long)V);
        if (E < 0) PG_FAIL("pose graph %d: edge offsets decrease", g);
        if (E > 0 && !edge_ij) PG_FAIL("pose graph: a null pointer");
        const int32_t rc = pg_plan_graph(err, cap, g, (int)V, (int)E, fixed + vertex_off[g], edge_ij ? edge_ij + 2 * (int64_t)edge_off[g] : nullptr,
                                         &(*plans)[g]);
        if (rc != ROAM_OK) return rc;
    }
    return ROAM_OK;
}

// consecutive graphs, as many as stay under the limit (at least one): [begin, end) of the chunk that starts at `begin`, and its bytes.
// The limit is roam_chunk_limit(PG_CHUNK_ENV, PG_CHUNK_BYTES): it only decides where a batch is cut; a single graph is refused against
// PG_CHUNK_BYTES alone and always fits a chunk of its own
static int pg_chunk_end(const std::vector<PgGraphPlan> &plans, int begin, int64_t limit, int64_t *bytes)
{
    int64_t sum = 0;
    int end = begin;
    while (end < (int)plans.size()) {
        const int64_t b = pg_graph_bytes(plans[end]);
        if (end > begin && sum + b > limit) break;
        sum += b;
        ++end;
    }
    *bytes = sum;
    return end;
}

extern "C" int32_t roam_pose_graph_plan(int32_t n_graphs, const int32_t *vertex_off, const uint8_t *fixed, const int32_t *edge_off,
                                        const int32_t *edge_ij, int64_t *envelope_blocks, int64_t *scratch_bytes)
{
    std::vector<PgGraphPlan> plans;
    const int32_t rc = pg_plan_all(nullptr, 0, n_graphs, vertex_off, fixed, edge_off, edge_ij, &plans);
    if (rc != ROAM_OK) return rc;
    int64_t worst = 0;
    const int64_t limit = roam_chunk_limit(PG_CHUNK_ENV, PG_CHUNK_BYTES);
    for (int begin = 0; begin < n_graphs;) {
        int64_t bytes;
        begin = pg_chunk_end(plans, begin, limit, &bytes);
        if (bytes > worst) worst = bytes;
    }
    for (int g = 0; g < n_graphs && envelope_blocks; ++g) envelope_blocks[g] = plans[g].env;
    if (scratch_bytes) *scratch_bytes = worst;
    return ROAM_OK;
}

static bool pg_all_finite(const double *v, int64_t n)
{
    for (int64_t q = 0; q < n; ++q)
        if (!std::isfinite(v[q])) return false;
    return true;
}

extern "C" int32_t roam_pose_graph_optimize(roam_ctx *ctx, int32_t n_graphs, const int32_t *vertex_off, double *poses, const uint8_t *fixed,
                                            const int32_t *edge_off, const int32_t *edge_ij, const double *edge_meas,
                                            const double *edge_info, const double *edge_huber, const roam_pose_graph_opts *opts,
                                            roam_pose_graph_stats *stats)
{
    if (!ctx) return ROAM_E_ARG;
    // ---- everything that can be refused is refused here, before the first device call
    ARG_CHECK(ctx, poses && opts && stats);
    std::vector<PgGraphPlan> plans;
    int32_t rc = pg_plan_all(ctx->err, sizeof(ctx->err), n_graphs, vertex_off, fixed, edge_off, edge_ij, &plans);
    if (rc != ROAM_OK) return rc;
    if (opts->max_iterations < 0 || opts->max_iterations > PG_MAX_ITERATIONS || opts->max_trials < 0 || opts->max_trials > PG_MAX_TRIALS ||
        !(std::isfinite(opts->lambda_init) && opts->lambda_init >= 0.0)) {
        ROAM_SET_ERR(ctx, "pose graph options: max_iterations in [0, %d], max_trials in [0, %d], lambda_init finite and >= 0, not %d, %d, %g",
                     PG_MAX_ITERATIONS, PG_MAX_TRIALS, opts->max_iterations, opts->max_trials, opts->lambda_init);
        return ROAM_E_ARG;
    }
    const int64_t Vtot = vertex_off[n_graphs], Etot = edge_off[n_graphs];
    ARG_CHECK(ctx, Etot == 0 || (edge_meas && edge_info));
    for (int g = 0; g < n_graphs; ++g) {
        for (int v = vertex_off[g]; v < vertex_off[g + 1]; ++v)
            if (!pg_all_finite(poses + 3 * (int64_t)v, 3)) {
                ROAM_SET_ERR(ctx, "pose graph %d, vertex %d: a pose that is not finite", g, v - vertex_off[g]);
                return ROAM_E_ARG;
            }
        for (int t = edge_off[g]; t < edge_off[g + 1]; ++t) {
            const bool ok = pg_all_finite(edge_meas + 3 * (int64_t)t, 3) && pg_all_finite(edge_info + 6 * (int64_t)t, 6);
            if (!ok || (edge_huber && !(std::isfinite(edge_huber[t]) && edge_huber[t] >= 0.0))) {
                ROAM_SET_ERR(ctx, "pose graph %d, edge %d: %s", g, t - edge_off[g],
                             ok ? "a Huber width that is negative or not finite" : "a measurement or information entry that is not finite");
                return ROAM_E_ARG;
            }
        }
    }

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int64_t limit = roam_chunk_limit(PG_CHUNK_ENV, PG_CHUNK_BYTES);
    for (int begin = 0; begin < n_graphs;) {
        int64_t chunk_bytes;
        const int end = pg_chunk_end(plans, begin, limit, &chunk_bytes);
        const int nb = end - begin;
        // ---- the chunk's lists: per graph cidx | fv | first | rowoff | colptr | colrows | incptr | inc
        std::vector<PgDesc> descs(nb);
        std::vector<int32_t> ints;
        int64_t nd = 0;
        const int64_t v_base = vertex_off[begin], e_base = edge_off[begin];
        for (int g = begin; g < end; ++g) {
            const PgGraphPlan &p = plans[g];
            PgDesc &d = descs[g - begin];
            const int32_t *ij = edge_ij + 2 * (int64_t)edge_off[g];
            d.V = p.V; d.F = p.F; d.E = p.E; d.env = (int32_t)p.env;
            d.v0 = vertex_off[g] - v_base;
            d.e0 = edge_off[g] - e_base;
            d.i_cidx = (int64_t)ints.size(); ints.insert(ints.end(), p.cidx.begin(), p.cidx.end());
            d.i_fv = (int64_t)ints.size(); ints.insert(ints.end(), p.fv.begin(), p.fv.end());
            d.i_first = (int64_t)ints.size(); ints.insert(ints.end(), p.first.begin(), p.first.end());
            d.i_rowoff = (int64_t)ints.size();
            int32_t off = 0;
            for (int k = 0; k < p.F; ++k) { ints.push_back(off); off += k - p.first[k] + 1; }
            ints.push_back(off);
            // col(c): the rows k > c with first[k] <= c, ascending
            std::vector<int32_t> cnt(p.F + 1, 0);
            for (int k = 0; k < p.F; ++k)
                for (int c = p.first[k]; c < k; ++c) ++cnt[c + 1];
            for (int c = 0; c < p.F; ++c) cnt[c + 1] += cnt[c];
            d.i_colptr = (int64_t)ints.size(); ints.insert(ints.end(), cnt.begin(), cnt.end());
            d.i_colrows = (int64_t)ints.size();
            ints.resize(ints.size() + (size_t)(p.env - p.F));
            {
                std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
                for (int k = 0; k < p.F; ++k)
                    for (int c = p.first[k]; c < k; ++c) ints[(size_t)d.i_colrows + fill[c]++] = k;
            }
            // the edges at each free vertex, ascending
            std::vector<int32_t> ip(p.F + 1, 0);
            for (int t = 0; t < p.E; ++t)
                for (int side = 0; side < 2; ++side) {
                    const int k = p.cidx[ij[2 * t + side]];
                    if (k >= 0) ++ip[k + 1];
                }
            for (int k = 0; k < p.F; ++k) ip[k + 1] += ip[k];
            d.i_incptr = (int64_t)ints.size(); ints.insert(ints.end(), ip.begin(), ip.end());
            d.i_inc = (int64_t)ints.size();
            ints.resize(ints.size() + (size_t)p.nnz);
            {
                std::vector<int32_t> fill(ip.begin(), ip.end() - 1);
                for (int t = 0; t < p.E; ++t)
                    for (int side = 0; side < 2; ++side) {
                        const int k = p.cidx[ij[2 * t + side]];
                        if (k >= 0) ints[(size_t)d.i_inc + fill[k]++] = t;
                    }
            }
            d.d_H = nd; nd += 9 * p.env;
            d.d_W = nd; nd += 9 * p.env;
            d.d_LD = nd; nd += 6 * (int64_t)p.F;
            d.d_b = nd; nd += 3 * (int64_t)p.F;
            d.d_d = nd; nd += 3 * (int64_t)p.F;
            d.d_y = nd; nd += 3 * (int64_t)p.F;
            d.d_xold = nd; nd += 3 * (int64_t)p.V;
        }
        const int64_t nv = vertex_off[end] - v_base, ne = edge_off[end] - e_base;
        std::vector<double> hub((size_t)ne, 0.0);
        if (edge_huber)
            for (int64_t t = 0; t < ne; ++t) hub[t] = edge_huber[e_base + t];

        double *d_dbl = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * (size_t)nd);
        int32_t *d_int = (int32_t *)roam_scratch(ctx, S_TMP1, sizeof(int32_t) * ints.size());
        double *d_pose = (double *)roam_scratch(ctx, S_IN0, sizeof(double) * 3 * (size_t)nv);
        int32_t *d_ij = (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * 2 * (size_t)ne);
        double *d_edge = (double *)roam_scratch(ctx, S_IN2, sizeof(double) * 10 * (size_t)ne);
        PgDesc *d_desc = (PgDesc *)roam_scratch(ctx, S_IN3, sizeof(PgDesc) * (size_t)nb);
        roam_pose_graph_stats *d_stats = (roam_pose_graph_stats *)roam_scratch(ctx, S_OUT0, sizeof(roam_pose_graph_stats) * (size_t)nb);
        if (!d_dbl || !d_int || !d_pose || !d_ij || !d_edge || !d_desc || !d_stats) return ROAM_E_HIP;
        HIP_TRY(ctx, hipMemcpyAsync(d_int, ints.data(), sizeof(int32_t) * ints.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_pose, poses + 3 * v_base, sizeof(double) * 3 * (size_t)nv, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_desc, descs.data(), sizeof(PgDesc) * (size_t)nb, hipMemcpyHostToDevice, st));
        PgEdges ed;
        ed.ij = d_ij; ed.meas = d_edge; ed.info = d_edge + 3 * ne; ed.huber = d_edge + 9 * ne;
        if (ne > 0) {
            HIP_TRY(ctx, hipMemcpyAsync(d_ij, edge_ij + 2 * e_base, sizeof(int32_t) * 2 * (size_t)ne, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_edge, edge_meas + 3 * e_base, sizeof(double) * 3 * (size_t)ne, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_edge + 3 * ne, edge_info + 6 * e_base, sizeof(double) * 6 * (size_t)ne, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_edge + 9 * ne, hub.data(), sizeof(double) * (size_t)ne, hipMemcpyHostToDevice, st));
        }
        hipLaunchKernelGGL(pose_graph_lm_kernel, dim3(nb), dim3(PG_THREADS), 0, st, d_desc, d_int, d_dbl, d_pose, ed, *opts, d_stats);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(poses + 3 * v_base, d_pose, sizeof(double) * 3 * (size_t)nv, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(stats + begin, d_stats, sizeof(roam_pose_graph_stats) * (size_t)nb, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));      // the host vectors of the chunk live until here
        begin = end;
    }
    return ROAM_OK;
}
