// Loop-closure candidates: the distance of queries to every entry of the database, and the selection of each query's k nearest.
// Map of the family: loop.h.
//
// Distance (loop_distance_kernel), the hot path: S S R multiply-adds per pair.  With normalised columns the cosine sum of shift k is
// the k-th wrapped diagonal of Qn Cn^T.  A workgroup takes one candidate and sixteen queries.  The candidate's columns go to LDS
// transposed and doubled along the sectors (cT[r][t], t < 2S), so that lane k reads the contiguous window cT[r][s + k] - consecutive
// lanes, consecutive addresses, no bank conflict.  A wave takes four queries; lane k (and k + 64, ... when S > 64) owns shift k.  The
// queries' values are wave-uniform and read straight from global memory (scalar loads, four rings at a time): one LDS read feeds
// four float64 fma.  When the doubled candidate does not fit 32 KiB of LDS the rings are taken in phases of RL = sc_phase_rings(S, R).
// Order of a pair's sum, a function of (S, R) alone: for each phase, for each sector s, the dot of the phase's rings in ring order
// from zero, then added to the shift's accumulator.  The count of valid sector pairs is the same correlation on the flags, in
// integers.  d_k = 1 - sum / count (1 when count = 0); the lowest k of the minimum wins (lane-local in ascending k, then a butterfly
// on (d, k)).  Nothing in a pair's arithmetic depends on where the candidate sits, on the other queries or on the chunk, so its
// (distance, shift) are the same bits in any call.
//
// Variants.  The kernel reads its queries as rows of (qnrm, qvalid): the database's own entries, or the variant store of a database
// that keeps offsets, where row q n_off + o is variant o + 1 of entry q.  A query over the variants runs the kernel twice - the plain
// entries, then the store - and loop_variant_fold_kernel takes per pair the minimum over the variants in ascending order with a
// strict <, so a tie keeps the lower variant and a result equal to the plain one reports variant 0.
//
// Selection (loop_select_kernel): one workgroup per query, k <= 32 passes, each the lexicographic minimum of (distance, index)
// above the previous pick, among the indices below max_index with distance <= max_distance.
#include "loop.h"
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

// ---------------------------------------------------------------------------------------------------------------- device
// rings of one LDS phase: all of them (padded to a multiple of four) when the doubled candidate fits, else the largest multiple of four
__host__ __device__ static int sc_phase_rings(int S, int Rp)
{
    const int fit = (SC_LDS_BYTES / (8 * (2 * S + 1))) & ~3;
    return Rp < fit ? Rp : fit;
}

// dist / shift: nq x count, row q = query row qidx[q] of (qnrm, qvalid).  qmax (optional): candidate j is computed for query q only
// when j < qmax[q]
template <int TK>
__global__ __launch_bounds__(SC_THREADS) void loop_distance_kernel(const double *__restrict__ nrm, const int32_t *__restrict__ valid,
                                                                   const double *__restrict__ qnrm, const int32_t *__restrict__ qvalid,
                                                                   const int32_t *__restrict__ qidx, const int32_t *__restrict__ qmax, int nq,
                                                                   int count, int S, int Rp, int RL, double *__restrict__ dist,
                                                                   int32_t *__restrict__ shift)
{
    extern __shared__ __align__(16) unsigned char ld_lds[];
    const int L = 2 * S + 1;
    double *cT = (double *)ld_lds;                        // RL x L: ring r of the phase, sectors 0 .. S-1, 0 .. S-1
    int32_t *vc = (int32_t *)(cT + (size_t)RL * L);       // 2S flags
    const int j = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q0 = blockIdx.y * SC_QB + wv * SC_QW;
    int qi[SC_QW];
    bool live[SC_QW], wave_live = false;
    for (int i = 0; i < SC_QW; ++i) {
        const int q = q0 + i < nq ? q0 + i : nq - 1;      // a slot past the end repeats the last query and writes nothing
        qi[i] = __builtin_amdgcn_readfirstlane(qidx[q]);
        live[i] = q0 + i < nq && (!qmax || j < qmax[q]);
        wave_live = wave_live || live[i];
    }
    if (!__syncthreads_or(wave_live)) return;

    const double *cj = nrm + (int64_t)j * S * Rp;
    for (int t = threadIdx.x; t < 2 * S; t += SC_THREADS) vc[t] = valid[(int64_t)j * S + (t >= S ? t - S : t)];
    int kk[TK];
    for (int u = 0; u < TK; ++u) kk[u] = lane + 64 * u < S ? lane + 64 * u : 0;      // a lane past S reads shift 0 and is left out below
    double acc[TK][SC_QW];
    for (int u = 0; u < TK; ++u)
        for (int i = 0; i < SC_QW; ++i) acc[u][i] = 0.0;

    for (int r0 = 0; r0 < Rp; r0 += RL) {
        const int rl = Rp - r0 < RL ? Rp - r0 : RL;
        __syncthreads();                                  // the previous phase has been read
        for (int idx = threadIdx.x; idx < 2 * S * rl; idx += SC_THREADS) {
            const int t = idx / rl, r = idx - t * rl;
            cT[r * L + t] = cj[(int64_t)(t >= S ? t - S : t) * Rp + r0 + r];
        }
        __syncthreads();
        if (!wave_live) continue;
        for (int s = 0; s < S; ++s) {
            double dot[TK][SC_QW];
            for (int u = 0; u < TK; ++u)
                for (int i = 0; i < SC_QW; ++i) dot[u][i] = 0.0;
            for (int r = 0; r < rl; r += 4) {
                double qv[SC_QW][4];
                for (int i = 0; i < SC_QW; ++i) {
                    const double *qp = qnrm + ((int64_t)qi[i] * S + s) * Rp + r0 + r;      // wave-uniform: scalar loads
                    for (int m = 0; m < 4; ++m) qv[i][m] = qp[m];
                }
                for (int m = 0; m < 4; ++m)
                    for (int u = 0; u < TK; ++u) {
                        const double c = cT[(r + m) * L + s + kk[u]];
                        for (int i = 0; i < SC_QW; ++i) dot[u][i] = fma(qv[i][m], c, dot[u][i]);
                    }
            }
            for (int u = 0; u < TK; ++u)
                for (int i = 0; i < SC_QW; ++i) acc[u][i] += dot[u][i];
        }
    }
    if (!wave_live) return;

    int cnt[TK][SC_QW];
    for (int u = 0; u < TK; ++u)
        for (int i = 0; i < SC_QW; ++i) cnt[u][i] = 0;
    for (int s = 0; s < S; ++s) {
        int vq[SC_QW];
        for (int i = 0; i < SC_QW; ++i) vq[i] = qvalid[(int64_t)qi[i] * S + s];
        for (int u = 0; u < TK; ++u) {
            const int v = vc[s + kk[u]];
            for (int i = 0; i < SC_QW; ++i) cnt[u][i] += vq[i] * v;
        }
    }
    for (int i = 0; i < SC_QW; ++i) {
        double bd = std::numeric_limits<double>::infinity();
        int bk = 0x7fffffff;
        for (int u = 0; u < TK; ++u) {
            const int k = lane + 64 * u;
            if (k >= S) continue;
            const double d = cnt[u][i] > 0 ? 1.0 - acc[u][i] / (double)cnt[u][i] : 1.0;
            if (d < bd) { bd = d; bk = k; }
        }
        for (int m = 32; m > 0; m >>= 1) {
            const double od = __shfl_xor(bd, m);
            const int ok = __shfl_xor(bk, m);
            if (od < bd || (od == bd && ok < bk)) { bd = od; bk = ok; }
        }
        if (lane == 0 && live[i]) {
            dist[(int64_t)(q0 + i) * count + j] = bd;
            shift[(int64_t)(q0 + i) * count + j] = bk;
        }
    }
}

// the minimum over the variants of every pair (q, j) that was computed: dist / shift hold variant 0 on entry and the minimum on exit
__global__ __launch_bounds__(SC_THREADS) void loop_variant_fold_kernel(double *__restrict__ dist, int32_t *__restrict__ shift,
                                                                       int32_t *__restrict__ var, const double *__restrict__ vdist,
                                                                       const int32_t *__restrict__ vshift, const int32_t *__restrict__ qmax,
                                                                       int nq, int count, int n_off)
{
    const int64_t p = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (p >= (int64_t)nq * count) return;
    const int64_t q = p / count;
    const int j = (int)(p - q * count);
    if (qmax && j >= qmax[q]) return;
    double bd = dist[p];
    int bs = shift[p], ba = 0;
    for (int o = 0; o < n_off; ++o) {
        const int64_t v = (q * n_off + o) * count + j;
        if (vdist[v] < bd) { bd = vdist[v]; bs = vshift[v]; ba = o + 1; }
    }
    dist[p] = bd;
    shift[p] = bs;
    var[p] = ba;
}

// the winning variant of every candidate slot (0 for an unused one)
__global__ __launch_bounds__(SC_THREADS) void loop_variant_gather_kernel(const int32_t *__restrict__ ci, const int32_t *__restrict__ var, int n_slots,
                                                                         int k, int count, int32_t *__restrict__ cv)
{
    const int p = blockIdx.x * SC_THREADS + threadIdx.x;
    if (p >= n_slots) return;
    cv[p] = ci[p] >= 0 ? var[(int64_t)(p / k) * count + ci[p]] : 0;
}

// per query the k smallest by (distance, index) among j < qmax[q] with distance <= max_distance; unused slots -1, +inf, 0
__global__ __launch_bounds__(SC_THREADS) void loop_select_kernel(const double *__restrict__ dist, const int32_t *__restrict__ shift,
                                                                 const int32_t *__restrict__ qmax, int count, int k, double max_distance,
                                                                 int32_t *__restrict__ ci, double *__restrict__ cd, int32_t *__restrict__ cs)
{
    __shared__ double red_d[SC_THREADS];
    __shared__ int32_t red_j[SC_THREADS];
    const int64_t q = blockIdx.x;
    const int t = threadIdx.x;
    const double *row = dist + q * count;
    const int lim = qmax[q] < count ? qmax[q] : count;
    const double inf = std::numeric_limits<double>::infinity();
    double pd = -inf;
    int pj = -1;
    for (int slot = 0; slot < k; ++slot) {
        double bd = inf;
        int bj = 0x7fffffff;
        for (int j = t; j < lim; j += SC_THREADS) {
            const double d = row[j];
            const bool above = d > pd || (d == pd && j > pj);
            if (d <= max_distance && above && (d < bd || (d == bd && j < bj))) { bd = d; bj = j; }
        }
        red_d[t] = bd;
        red_j[t] = bj;
        __syncthreads();
        for (int h = SC_THREADS / 2; h > 0; h >>= 1) {
            if (t < h && (red_d[t + h] < red_d[t] || (red_d[t + h] == red_d[t] && red_j[t + h] < red_j[t]))) {
                red_d[t] = red_d[t + h];
                red_j[t] = red_j[t + h];
            }
            __syncthreads();
        }
        pd = red_d[0];
        pj = red_j[0];
        __syncthreads();
        const bool found = pj != 0x7fffffff;
        if (t == 0) {
            ci[q * k + slot] = found ? pj : -1;
            cd[q * k + slot] = found ? pd : inf;
            cs[q * k + slot] = found ? shift[q * count + pj] : 0;
        }
        if (!found) { pd = inf; pj = 0x7ffffffe; }       // nothing is above this: the remaining slots stay empty
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
// the distance kernel for nq queries (d_q: their indices, d_mask: optional max_index) against every entry, and the selection
// variants: the queries are rows of the variant store, not entries
static hipError_t sc_launch_distance(hipStream_t st, const roam_loop_db *db, const int32_t *d_q, const int32_t *d_mask, int nq, double *d_dist,
                                     int32_t *d_shift, bool variants = false)
{
    const double *qn = variants ? db->vnrm : db->nrm;
    const int32_t *qv = variants ? db->vvalid : db->valid;
    const int count = db->count, S = db->S, Rp = db->Rp;
    const int RL = sc_phase_rings(S, Rp);
    const size_t lds = sizeof(double) * (size_t)RL * (2 * S + 1) + sizeof(int32_t) * 2 * S;
    const dim3 grid(count, (nq + SC_QB - 1) / SC_QB);
    switch ((S + 63) / 64) {
    case 1: hipLaunchKernelGGL(loop_distance_kernel<1>, grid, dim3(SC_THREADS), lds, st, db->nrm, db->valid, qn, qv, d_q, d_mask, nq, count, S, Rp, RL, d_dist, d_shift); break;
    case 2: hipLaunchKernelGGL(loop_distance_kernel<2>, grid, dim3(SC_THREADS), lds, st, db->nrm, db->valid, qn, qv, d_q, d_mask, nq, count, S, Rp, RL, d_dist, d_shift); break;
    case 3: hipLaunchKernelGGL(loop_distance_kernel<3>, grid, dim3(SC_THREADS), lds, st, db->nrm, db->valid, qn, qv, d_q, d_mask, nq, count, S, Rp, RL, d_dist, d_shift); break;
    default: hipLaunchKernelGGL(loop_distance_kernel<4>, grid, dim3(SC_THREADS), lds, st, db->nrm, db->valid, qn, qv, d_q, d_mask, nq, count, S, Rp, RL, d_dist, d_shift); break;
    }
    return hipGetLastError();
}

static hipError_t sc_launch_select(hipStream_t st, const roam_loop_db *db, const int32_t *d_qmax, int nq, int k, double max_distance,
                                   const double *d_dist, const int32_t *d_shift, int32_t *d_ci, double *d_cd, int32_t *d_cs)
{
    hipLaunchKernelGGL(loop_select_kernel, dim3(nq), dim3(SC_THREADS), 0, st, d_dist, d_shift, d_qmax, db->count, k, max_distance, d_ci, d_cd, d_cs);
    return hipGetLastError();
}

// a query over the variants, after the plain distance: the store's rows against every entry, then the fold into dist / shift / var
static hipError_t sc_launch_variants(hipStream_t st, const roam_loop_db *db, const LoopQueryBufs &b, int nq, bool every_pair)
{
    hipError_t e = sc_launch_distance(st, db, b.d_vq, every_pair ? nullptr : b.d_vqmax, nq * b.n_off, b.d_vdist, b.d_vshift, true);
    if (e != hipSuccess) return e;
    const int64_t pairs = (int64_t)nq * db->count;
    hipLaunchKernelGGL(loop_variant_fold_kernel, dim3((unsigned)((pairs + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, st, b.d_dist, b.d_shift,
                       b.d_var, b.d_vdist, b.d_vshift, every_pair ? nullptr : b.d_qmax, nq, db->count, b.n_off);
    return hipGetLastError();
}

int32_t sc_check_query(roam_ctx *ctx, const roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index, int32_t k,
                       double max_distance)
{
    if (!db || !query_index || !max_index) {
        ROAM_SET_ERR(ctx, "loop db query: %s is null", !db ? "db" : !query_index ? "query_index" : "max_index");
        return ROAM_E_ARG;
    }
    if (n_query < 1) { ROAM_SET_ERR(ctx, "loop db query: n_query >= 1, not %d", n_query); return ROAM_E_ARG; }
    if (k < 1 || k > ROAM_LOOP_MAX_K) { ROAM_SET_ERR(ctx, "loop db query: k in [1, %d], not %d", ROAM_LOOP_MAX_K, k); return ROAM_E_ARG; }
    if (std::isnan(max_distance)) { ROAM_SET_ERR(ctx, "loop db query: max_distance is not a number"); return ROAM_E_ARG; }
    for (int q = 0; q < n_query; ++q)
        if (query_index[q] < 0 || query_index[q] >= db->count) {
            ROAM_SET_ERR(ctx, "loop db query: query_index[%d] = %d outside the %d entries stored", q, query_index[q], db->count);
            return ROAM_E_ARG;
        }
    return ROAM_OK;
}

// ---- the query pass of a chunk, in the order its callers run it: clamp (once per call), stage, enqueue, download
std::vector<int32_t> loop_query_clamp(const roam_loop_db *db, int32_t n_query, const int32_t *max_index)
{
    const int count = db->count;
    std::vector<int32_t> qm((size_t)n_query);
    for (int q = 0; q < n_query; ++q) qm[q] = max_index[q] < 0 ? 0 : max_index[q] > count ? count : max_index[q];
    return qm;
}

int64_t loop_query_bytes(const roam_loop_db *db, bool with_variants)
{
    const int64_t pair = (int64_t)(sizeof(double) + sizeof(int32_t)) * db->count;
    return with_variants ? pair * (1 + db->n_off) + (int64_t)sizeof(int32_t) * db->count : pair;
}

// the variants' side of the stage: scratch, and the rows q n_off + o with their queries' maxima
static int32_t loop_query_stage_variants(roam_ctx *ctx, const roam_loop_db *db, int nq, int k, const int32_t *query_index, const int32_t *qmax,
                                         LoopQueryBufs *b)
{
    const int n_off = db->n_off;
    const size_t vrows = (size_t)nq * n_off, vpairs = vrows * db->count;
    b->n_off = n_off;
    b->d_vdist = (double *)roam_scratch(ctx, S_TMP2, sizeof(double) * vpairs);
    b->d_vshift = (int32_t *)roam_scratch(ctx, S_TMP5, sizeof(int32_t) * vpairs);
    b->d_var = (int32_t *)roam_scratch(ctx, S_TMP6, sizeof(int32_t) * (size_t)nq * db->count);
    b->d_vq = (int32_t *)roam_scratch(ctx, S_TMP7, sizeof(int32_t) * 2 * vrows);
    b->d_vqmax = b->d_vq ? b->d_vq + vrows : nullptr;
    b->d_cv = (int32_t *)roam_scratch(ctx, S_IN0, sizeof(int32_t) * (size_t)nq * k);
    if (!b->d_vdist || !b->d_vshift || !b->d_var || !b->d_vq || !b->d_cv) return ROAM_E_HIP;
    std::vector<int32_t> &rows = b->h_rows;                       // the caller's: alive until the chunk's wait
    rows.resize(2 * vrows);
    for (int q = 0; q < nq; ++q)
        for (int o = 0; o < n_off; ++o) {
            rows[(size_t)q * n_off + o] = query_index[q] * n_off + o;
            rows[vrows + (size_t)q * n_off + o] = qmax[q];
        }
    HIP_TRY(ctx, hipMemcpyAsync(b->d_vq, rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice, ctx->stream));
    return ROAM_OK;
}

int32_t loop_query_stage(roam_ctx *ctx, const roam_loop_db *db, int nq, int k, const int32_t *query_index, const int32_t *qmax, LoopQueryBufs *b,
                         bool with_variants)
{
    b->n_off = 0;
    b->d_vdist = nullptr; b->d_vshift = b->d_var = b->d_vq = b->d_vqmax = b->d_cv = nullptr;
    const size_t pairs = (size_t)nq * db->count, cands = (size_t)nq * k;
    b->d_dist = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * pairs);
    b->d_shift = (int32_t *)roam_scratch(ctx, S_TMP1, sizeof(int32_t) * pairs);
    b->d_q = (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * 2 * (size_t)nq);
    b->d_qmax = b->d_q ? b->d_q + nq : nullptr;
    b->d_ci = (int32_t *)roam_scratch(ctx, S_OUT0, sizeof(int32_t) * cands);
    b->d_cd = (double *)roam_scratch(ctx, S_OUT1, sizeof(double) * cands);
    b->d_cs = (int32_t *)roam_scratch(ctx, S_OUT2, sizeof(int32_t) * cands);
    if (!b->d_dist || !b->d_shift || !b->d_q || !b->d_ci || !b->d_cd || !b->d_cs) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(b->d_q, query_index, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(b->d_qmax, qmax, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
    if (with_variants && db->n_off) LOOP_TRY(loop_query_stage_variants(ctx, db, nq, k, query_index, qmax, b));
    return ROAM_OK;
}

int32_t loop_query_enqueue(roam_ctx *ctx, const roam_loop_db *db, const LoopQueryBufs &b, int nq, int k, double max_distance, bool every_pair)
{
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, sc_launch_distance(st, db, b.d_q, every_pair ? nullptr : b.d_qmax, nq, b.d_dist, b.d_shift));
    if (b.n_off) HIP_TRY(ctx, sc_launch_variants(st, db, b, nq, every_pair));
    HIP_TRY(ctx, sc_launch_select(st, db, b.d_qmax, nq, k, max_distance, b.d_dist, b.d_shift, b.d_ci, b.d_cd, b.d_cs));
    if (b.n_off) {
        hipLaunchKernelGGL(loop_variant_gather_kernel, dim3((nq * k + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, st, b.d_ci, b.d_var, nq * k, k,
                           db->count, b.d_cv);
        HIP_TRY(ctx, hipGetLastError());
    }
    return ROAM_OK;
}

int32_t loop_query_download(roam_ctx *ctx, const LoopQueryBufs &b, int nq, int k, int32_t *cand_index, double *cand_dist, int32_t *cand_shift)
{
    const size_t cands = (size_t)nq * k;
    HIP_TRY(ctx, hipMemcpyAsync(cand_index, b.d_ci, sizeof(int32_t) * cands, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(cand_dist, b.d_cd, sizeof(double) * cands, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(cand_shift, b.d_cs, sizeof(int32_t) * cands, hipMemcpyDeviceToHost, ctx->stream));
    return ROAM_OK;
}

// roam_loop_db_query and roam_loop_db_query_offsets: variants = the queries are the entries' variants as well (a database that keeps
// offsets); cand_var / var_full: the winning variants, zero without variants
static int32_t sc_query_run(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index, int32_t k,
                            double max_distance, bool variants, int32_t *cand_index, double *cand_dist, int32_t *cand_shift, int32_t *cand_var,
                            double *dist_full, int32_t *shift_full, int32_t *var_full)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int count = db->count;
    int64_t chunk = roam_chunk_limit(SC_CHUNK_ENV, SC_DB_BYTES) / loop_query_bytes(db, variants);
    if (chunk < 1) chunk = 1;
    const int64_t rows_per_query = variants ? db->n_off : 1;
    if (chunk > 65535 * SC_QB / rows_per_query) chunk = 65535 * SC_QB / rows_per_query;     // the grid's y extent
    const std::vector<int32_t> qm = loop_query_clamp(db, n_query, max_index);
    const bool full = dist_full || shift_full || var_full;
    for (int64_t q0 = 0; q0 < n_query; q0 += chunk) {
        const int nq = (int)(n_query - q0 < chunk ? n_query - q0 : chunk);
        const size_t pairs = (size_t)nq * count;
        LoopQueryBufs b;
        LOOP_TRY(loop_query_stage(ctx, db, nq, k, query_index + q0, qm.data() + q0, &b, variants));
        LOOP_TRY(loop_query_enqueue(ctx, db, b, nq, k, max_distance, full));
        LOOP_TRY(loop_query_download(ctx, b, nq, k, cand_index + q0 * k, cand_dist + q0 * k, cand_shift + q0 * k));
        if (dist_full) HIP_TRY(ctx, hipMemcpyAsync(dist_full + q0 * count, b.d_dist, sizeof(double) * pairs, hipMemcpyDeviceToHost, st));
        if (shift_full) HIP_TRY(ctx, hipMemcpyAsync(shift_full + q0 * count, b.d_shift, sizeof(int32_t) * pairs, hipMemcpyDeviceToHost, st));
        if (variants) {
            if (cand_var) HIP_TRY(ctx, hipMemcpyAsync(cand_var + q0 * k, b.d_cv, sizeof(int32_t) * (size_t)nq * k, hipMemcpyDeviceToHost, st));
            if (var_full) HIP_TRY(ctx, hipMemcpyAsync(var_full + q0 * count, b.d_var, sizeof(int32_t) * pairs, hipMemcpyDeviceToHost, st));
        } else {
            if (cand_var) memset(cand_var + q0 * k, 0, sizeof(int32_t) * (size_t)nq * k);
            if (var_full) memset(var_full + q0 * count, 0, sizeof(int32_t) * pairs);
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_query(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                      int32_t k, double max_distance, int32_t *cand_index, double *cand_dist, int32_t *cand_shift,
                                      double *dist_full, int32_t *shift_full)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_query(ctx, db, n_query, query_index, max_index, k, max_distance));
    if (!cand_index || !cand_dist || !cand_shift) {
        ROAM_SET_ERR(ctx, "loop db query: %s is null", !cand_index ? "cand_index" : !cand_dist ? "cand_dist" : "cand_shift");
        return ROAM_E_ARG;
    }
    return sc_query_run(ctx, db, n_query, query_index, max_index, k, max_distance, false, cand_index, cand_dist, cand_shift, nullptr, dist_full,
                        shift_full, nullptr);
}

extern "C" int32_t roam_loop_db_query_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                              int32_t k, double max_distance, int32_t *cand_index, double *cand_dist, int32_t *cand_shift,
                                              int32_t *cand_offset, double *dist_full, int32_t *shift_full, int32_t *offset_full)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_query(ctx, db, n_query, query_index, max_index, k, max_distance));
    if (!cand_index || !cand_dist || !cand_shift || !cand_offset) {
        ROAM_SET_ERR(ctx, "loop db query: %s is null", !cand_index ? "cand_index" : !cand_dist ? "cand_dist" : !cand_shift ? "cand_shift" : "cand_offset");
        return ROAM_E_ARG;
    }
    return sc_query_run(ctx, db, n_query, query_index, max_index, k, max_distance, db->n_off > 0, cand_index, cand_dist, cand_shift, cand_offset,
                        dist_full, shift_full, offset_full);
}

extern "C" int32_t roam_time_loop_db_query(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                           int32_t k, double max_distance, int32_t reps, float *distance_ms, float *select_ms)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_query(ctx, db, n_query, query_index, max_index, k, max_distance));
    ARG_CHECK(ctx, reps >= 1 && distance_ms && select_ms);
    const int count = db->count;
    if ((int64_t)n_query * count * (int64_t)(sizeof(double) + sizeof(int32_t)) > SC_DB_BYTES || n_query > 65535 * SC_QB) {
        ROAM_SET_ERR(ctx, "loop db timing: %d queries against %d entries do not fit one launch", n_query, count);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const std::vector<int32_t> qm = loop_query_clamp(db, n_query, max_index);
    LoopQueryBufs b;
    LOOP_TRY(loop_query_stage(ctx, db, n_query, k, query_index, qm.data(), &b));
    LOOP_TRY(roam_time_launches(ctx, st, reps, distance_ms, [&] { return sc_launch_distance(st, db, b.d_q, b.d_qmax, n_query, b.d_dist, b.d_shift); }));
    return roam_time_launches(ctx, st, reps, select_ms,
                              [&] { return sc_launch_select(st, db, b.d_qmax, n_query, k, max_distance, b.d_dist, b.d_shift, b.d_ci, b.d_cd, b.d_cs); });
}

extern "C" int32_t roam_time_loop_db_query_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index,
                                                   const int32_t *max_index, int32_t k, double max_distance, int32_t reps, float *plain_ms,
                                                   float *variants_ms, float *select_ms)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_query(ctx, db, n_query, query_index, max_index, k, max_distance));
    ARG_CHECK(ctx, reps >= 1 && plain_ms && variants_ms && select_ms);
    if (!db->n_off) { ROAM_SET_ERR(ctx, "loop db timing: db keeps no offsets"); return ROAM_E_ARG; }
    if (n_query * loop_query_bytes(db, true) > SC_DB_BYTES || (int64_t)n_query * db->n_off > 65535 * SC_QB) {
        ROAM_SET_ERR(ctx, "loop db timing: %d queries against %d entries do not fit one launch", n_query, db->count);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const std::vector<int32_t> qm = loop_query_clamp(db, n_query, max_index);
    LoopQueryBufs b;
    LOOP_TRY(loop_query_stage(ctx, db, n_query, k, query_index, qm.data(), &b, true));
    LOOP_TRY(roam_time_launches(ctx, st, reps, plain_ms, [&] { return sc_launch_distance(st, db, b.d_q, b.d_qmax, n_query, b.d_dist, b.d_shift); }));
    LOOP_TRY(roam_time_launches(ctx, st, reps, variants_ms, [&] { return sc_launch_variants(st, db, b, n_query, false); }));
    return roam_time_launches(ctx, st, reps, select_ms,
                              [&] { return sc_launch_select(st, db, b.d_qmax, n_query, k, max_distance, b.d_dist, b.d_shift, b.d_ci, b.d_cd, b.d_cs); });
}
