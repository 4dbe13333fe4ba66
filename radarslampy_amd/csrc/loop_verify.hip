// Verification of loop-closure candidates from the database's resident peak clouds.  Map of the family: loop.h.
//
// Verification (roam_loop_db_verify, roam_loop_db_query_verify) runs icp.hip's store kernel on pairs of slots; the
// query form enqueues distance, selection, loop_pairs_kernel (candidates -> pairs and their yaw seeds) and the ICP on one stream.
#include "loop.h"
#include <cmath>
#include <cstring>

// ---------------------------------------------------------------------------------------------------------------- device
// query_verify: slot (q, s) of the selection -> pair q k + s: the query's cloud onto the candidate's (-1: an empty pair) from
// (yaw, 0, 0), yaw = 2 pi shift / S in (-pi, pi] by LoopClosure._yaw's operations.  cv (optional, a database that keeps offsets): the
// slot's winning variant; variant a >= 1 with the offset o = off_m[a - 1] seeds (yaw, -R(yaw) o), variant 0 as before
__global__ __launch_bounds__(SC_THREADS) void loop_pairs_kernel(const int32_t *__restrict__ qidx, const int32_t *__restrict__ ci,
                                                                const int32_t *__restrict__ cs, const int32_t *__restrict__ cv,
                                                                const double *__restrict__ off_m, int n_pairs, int k, int S,
                                                                int32_t *__restrict__ src_index, int32_t *__restrict__ dst_index,
                                                                double *__restrict__ init)
{
    const int p = blockIdx.x * SC_THREADS + threadIdx.x;
    if (p >= n_pairs) return;
    src_index[p] = qidx[p / k];
    dst_index[p] = ci[p];
    const double a = (6.283185307179586 * (double)cs[p]) / (double)S;
    const double yaw = a > 3.141592653589793 ? a - 6.283185307179586 : a;
    double tx = 0.0, ty = 0.0;
    if (cv && cv[p] > 0) {
        const double ox = off_m[2 * (cv[p] - 1)], oy = off_m[2 * (cv[p] - 1) + 1], c = cos(yaw), s = sin(yaw);
        tx = -(c * ox - s * oy);
        ty = -(s * ox + c * oy);
    }
    init[3 * (int64_t)p] = yaw;
    init[3 * (int64_t)p + 1] = tx;
    init[3 * (int64_t)p + 2] = ty;
}

// ---------------------------------------------------------------------------------------------------------------- host
// device bytes one pair of a verification launch takes: partners, indices, seed, pose, statistics
static int64_t sc_pair_bytes(const roam_loop_db *db)
{
    return (int64_t)db->max_points * sizeof(int32_t) + 2 * sizeof(int32_t) + 6 * sizeof(double) + sizeof(roam_icp_stats);
}

// the scratch of np pairs -> A (the indices and seeds are the caller's to fill: A's pointers are writable device memory)
static int32_t sc_verify_scratch(roam_ctx *ctx, const roam_loop_db *db, int np, const roam_icp_opts &o, IcpStoreArgs *A)
{
    int32_t *d_pair = (int32_t *)roam_scratch(ctx, S_IN2, sizeof(int32_t) * 2 * (size_t)np);
    double *d_init = (double *)roam_scratch(ctx, S_IN3, sizeof(double) * 3 * (size_t)np);
    int32_t *d_partner = (int32_t *)roam_scratch(ctx, S_TMP3, sizeof(int32_t) * (size_t)np * db->max_points);
    double *d_pose = (double *)roam_scratch(ctx, S_OUT3, sizeof(double) * 3 * (size_t)np);
    roam_icp_stats *d_stats = (roam_icp_stats *)roam_scratch(ctx, S_TMP4, sizeof(roam_icp_stats) * (size_t)np);
    if (!d_pair || !d_init || !d_partner || !d_pose || !d_stats) return ROAM_E_HIP;
    *A = IcpStoreArgs{db->cloud, db->cloud_n, db->max_points, d_pair, d_pair + np, d_init, d_partner, d_pose, d_stats, o};
    return ROAM_OK;
}

// pairs per launch under the scratch limit and the grid's extent
static int64_t sc_pair_chunk(const roam_loop_db *db)
{
    int64_t chunk = roam_chunk_limit(SC_CHUNK_ENV, SC_DB_BYTES) / sc_pair_bytes(db);
    return chunk < 1 ? 1 : chunk > ROAM_ICP_MAX_PAIRS ? ROAM_ICP_MAX_PAIRS : chunk;
}

static int32_t sc_check_pairs(roam_ctx *ctx, const roam_loop_db *db, int32_t n_pairs, const int32_t *src_index, const int32_t *dst_index,
                              const double *init)
{
    if (!db) { ROAM_SET_ERR(ctx, "loop db verify: db is null"); return ROAM_E_ARG; }
    if (!db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db verify: db keeps no clouds (roam_loop_db_keep_clouds)"); return ROAM_E_STATE; }
    if (!src_index || !dst_index || !init) {
        ROAM_SET_ERR(ctx, "loop db verify: %s is null", !src_index ? "src_index" : !dst_index ? "dst_index" : "init");
        return ROAM_E_ARG;
    }
    if (n_pairs < 1 || n_pairs > ROAM_ICP_MAX_PAIRS) { ROAM_SET_ERR(ctx, "loop db verify: n_pairs in [1, %d], not %d", ROAM_ICP_MAX_PAIRS, n_pairs); return ROAM_E_ARG; }
    for (int p = 0; p < n_pairs; ++p) {
        if (src_index[p] < 0 || src_index[p] >= db->count) {
            ROAM_SET_ERR(ctx, "loop db verify: src_index[%d] = %d outside the %d entries stored", p, src_index[p], db->count);
            return ROAM_E_ARG;
        }
        if (dst_index[p] < 0 || dst_index[p] >= db->count) {
            ROAM_SET_ERR(ctx, "loop db verify: dst_index[%d] = %d outside the %d entries stored", p, dst_index[p], db->count);
            return ROAM_E_ARG;
        }
        if (!(std::isfinite(init[3 * p]) && fabs(init[3 * p + 1]) <= ROAM_ICP_MAX_COORD && fabs(init[3 * p + 2]) <= ROAM_ICP_MAX_COORD)) {
            ROAM_SET_ERR(ctx, "loop db verify: init of pair %d: a pose that is not finite or beyond %g m", p, ROAM_ICP_MAX_COORD);
            return ROAM_E_ARG;
        }
    }
    return ROAM_OK;
}

// upload the pairs [p0, p0 + np) into A's scratch
static int32_t sc_stage_pairs(roam_ctx *ctx, const IcpStoreArgs &A, int p0, int np, const int32_t *src_index, const int32_t *dst_index,
                              const double *init)
{
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync((void *)A.src_index, src_index + p0, sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync((void *)A.dst_index, dst_index + p0, sizeof(int32_t) * (size_t)np, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync((void *)A.init, init + 3 * (int64_t)p0, sizeof(double) * 3 * (size_t)np, hipMemcpyHostToDevice, st));
    return ROAM_OK;
}

// the results of np pairs from A's scratch -> the host, from pair p0 on
static int32_t sc_download_pairs(roam_ctx *ctx, const IcpStoreArgs &A, int64_t p0, int np, double *pose_out, roam_icp_stats *stats)
{
    HIP_TRY(ctx, hipMemcpyAsync(pose_out + 3 * p0, A.pose, sizeof(double) * 3 * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(stats + p0, A.stats, sizeof(roam_icp_stats) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_pairs, const int32_t *src_index, const int32_t *dst_index,
                                       const double *init, const roam_icp_opts *opts, double *pose_out, roam_icp_stats *stats)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_pairs(ctx, db, n_pairs, src_index, dst_index, init));
    if (!pose_out || !stats) { ROAM_SET_ERR(ctx, "loop db verify: %s is null", !pose_out ? "pose_out" : "stats"); return ROAM_E_ARG; }
    roam_icp_opts o;
    LOOP_TRY(roam_icp_resolve_opts(ctx, opts, &o));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int64_t chunk = sc_pair_chunk(db);
    for (int64_t p0 = 0; p0 < n_pairs; p0 += chunk) {
        const int np = (int)(n_pairs - p0 < chunk ? n_pairs - p0 : chunk);
        IcpStoreArgs A;
        LOOP_TRY(sc_verify_scratch(ctx, db, np, o, &A));
        LOOP_TRY(sc_stage_pairs(ctx, A, (int)p0, np, src_index, dst_index, init));
        HIP_TRY(ctx, launch_icp2d_store(st, A, np));
        LOOP_TRY(sc_download_pairs(ctx, A, p0, np, pose_out, stats));
        HIP_TRY(ctx, hipStreamSynchronize(st));           // the next chunk reuses the scratch
    }
    return ROAM_OK;
}

extern "C" int32_t roam_time_loop_db_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_pairs, const int32_t *src_index, const int32_t *dst_index,
                                            const double *init, const roam_icp_opts *opts, int32_t reps, float *ms_per_rep)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_pairs(ctx, db, n_pairs, src_index, dst_index, init));
    ARG_CHECK(ctx, reps >= 1 && ms_per_rep);
    roam_icp_opts o;
    LOOP_TRY(roam_icp_resolve_opts(ctx, opts, &o));
    if (n_pairs * sc_pair_bytes(db) > SC_DB_BYTES) { ROAM_SET_ERR(ctx, "loop db timing: %d pairs do not fit one launch", n_pairs); return ROAM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    IcpStoreArgs A;
    LOOP_TRY(sc_verify_scratch(ctx, db, n_pairs, o, &A));
    LOOP_TRY(sc_stage_pairs(ctx, A, 0, n_pairs, src_index, dst_index, init));
    return roam_time_launches(ctx, st, reps, ms_per_rep, [&] { return launch_icp2d_store(st, A, n_pairs); });
}

// roam_loop_db_query_verify and its _offsets form: cand_offset (optional) = the winning variants, zero for a database without offsets
static int32_t sc_query_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index, int32_t k,
                               double max_distance, const roam_icp_opts *opts, int32_t *cand_index, double *cand_dist, int32_t *cand_shift,
                               int32_t *cand_offset, double *pose_out, roam_icp_stats *stats)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_query(ctx, db, n_query, query_index, max_index, k, max_distance));
    if (!db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db verify: db keeps no clouds (roam_loop_db_keep_clouds)"); return ROAM_E_STATE; }
    if (!cand_index || !cand_dist || !cand_shift || !pose_out || !stats) {
        ROAM_SET_ERR(ctx, "loop db query: %s is null", !cand_index ? "cand_index" : !cand_dist ? "cand_dist" : !cand_shift ? "cand_shift"
                                                       : !pose_out ? "pose_out" : "stats");
        return ROAM_E_ARG;
    }
    roam_icp_opts o;
    LOOP_TRY(roam_icp_resolve_opts(ctx, opts, &o));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    // queries per launch: the distance scratch, the pairs' scratch and the grids' extents
    const bool variants = db->n_off > 0;
    int64_t chunk = roam_chunk_limit(SC_CHUNK_ENV, SC_DB_BYTES) / (loop_query_bytes(db, variants) + (int64_t)k * sc_pair_bytes(db));
    if (chunk > ROAM_ICP_MAX_PAIRS / k) chunk = ROAM_ICP_MAX_PAIRS / k;
    if (variants && chunk > 65535 * SC_QB / db->n_off) chunk = 65535 * SC_QB / db->n_off;
    if (chunk < 1) chunk = 1;
    const std::vector<int32_t> qm = loop_query_clamp(db, n_query, max_index);
    for (int64_t q0 = 0; q0 < n_query; q0 += chunk) {
        const int nq = (int)(n_query - q0 < chunk ? n_query - q0 : chunk);
        const int np = nq * k;
        IcpStoreArgs A;
        LoopQueryBufs b;
        LOOP_TRY(sc_verify_scratch(ctx, db, np, o, &A));  // every take of the chunk comes before its first copy: a slot that grows waits for the stream
        LOOP_TRY(loop_query_stage(ctx, db, nq, k, query_index + q0, qm.data() + q0, &b, variants));
        LOOP_TRY(loop_query_enqueue(ctx, db, b, nq, k, max_distance, false));
        hipLaunchKernelGGL(loop_pairs_kernel, dim3((np + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, st, b.d_q, b.d_ci, b.d_cs, b.d_cv, db->off_m,
                           np, k, db->S,
                           (int32_t *)A.src_index, (int32_t *)A.dst_index, (double *)A.init);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, launch_icp2d_store(st, A, np));
        LOOP_TRY(loop_query_download(ctx, b, nq, k, cand_index + q0 * k, cand_dist + q0 * k, cand_shift + q0 * k));
        LOOP_TRY(sc_download_pairs(ctx, A, q0 * k, np, pose_out, stats));
        if (cand_offset && variants) HIP_TRY(ctx, hipMemcpyAsync(cand_offset + q0 * k, b.d_cv, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, st));
        if (cand_offset && !variants) memset(cand_offset + q0 * k, 0, sizeof(int32_t) * (size_t)np);
        HIP_TRY(ctx, hipStreamSynchronize(st));           // the one wait of the chunk
    }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_query_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                             int32_t k, double max_distance, const roam_icp_opts *opts, int32_t *cand_index, double *cand_dist,
                                             int32_t *cand_shift, double *pose_out, roam_icp_stats *stats)
{
    return sc_query_verify(ctx, db, n_query, query_index, max_index, k, max_distance, opts, cand_index, cand_dist, cand_shift, nullptr, pose_out, stats);
}

extern "C" int32_t roam_loop_db_query_verify_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index,
                                                     const int32_t *max_index, int32_t k, double max_distance, const roam_icp_opts *opts,
                                                     int32_t *cand_index, double *cand_dist, int32_t *cand_shift, int32_t *cand_offset,
                                                     double *pose_out, roam_icp_stats *stats)
{
    if (ctx && !cand_offset) { ROAM_SET_ERR(ctx, "loop db query: cand_offset is null"); return ROAM_E_ARG; }
    return sc_query_verify(ctx, db, n_query, query_index, max_index, k, max_distance, opts, cand_index, cand_dist, cand_shift, cand_offset, pose_out,
                           stats);
}
