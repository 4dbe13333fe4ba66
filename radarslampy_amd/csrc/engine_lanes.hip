// Lane set-up and read-back of the engine (engine.hip): a lane's first pyramid, pose and features (given, or detected on the device),
// what a lane holds now, and the pass-through entry points that run another unit's work on the scans resident in the pool.
#include "engine.h"
#include "loop.h"

// features -> keyframe locals: undistort(velocity, (pts - center) * m/px) (Mapping.py:59-66)
__global__ void lane_kf_reset_kernel(const float *__restrict__ feat, int K, const double *__restrict__ vel,
                                     double *__restrict__ kf_und)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= K) return;
    const double x = ((double)feat[2 * j] - CART_CENTER) * M_PER_PX, y = ((double)feat[2 * j + 1] - CART_CENTER) * M_PER_PX;
    const double dT = 0.25 * atan2(-y, -x) / TWO_PI;
    const double a = vel[2] * dT, ca = cos(a), sa = sin(a);
    kf_und[2 * j] = ca * x - sa * y + vel[0] * dT;
    kf_und[2 * j + 1] = sa * x + ca * y + vel[1] * dT;
}

extern "C" {

static int32_t set_features_impl(roam_ctx *ctx, Engine *e, int32_t lane, const float *pts, int32_t K, int32_t kf_scan)
{
    float *f = e->feat + (size_t)lane * KS * 2;
    // f1: the keyframe this call replaces goes to the lane's map ring first (device-side decision, see the kernel)
    if (e->map_cap > 0) ROAM_TRY(launch_map_freeze(ctx, e, lane));
    e->lane_k[lane] = K;
    if (K > 0) HIP_TRY(ctx, hipMemcpyAsync(f, pts, sizeof(float) * 2 * (size_t)K, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(e->feat_n + lane, &K, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    // the frame that triggers a retrack also adds a keyframe at the latest pose (RawROAMSystem.py:250-270):
    // kf pose = latest pose, kf locals = undistort(velocity, centred features)
    HIP_TRY(ctx, hipMemcpyAsync(e->kf_pose + 3 * (size_t)lane, e->pose + 3 * (size_t)lane, sizeof(double) * 3,
                                hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(e->kf_vel + 3 * (size_t)lane, e->vel + 3 * (size_t)lane, sizeof(double) * 3,
                                hipMemcpyDeviceToDevice, ctx->stream));
    const int32_t one = 1;
    HIP_TRY(ctx, hipMemcpyAsync(e->kf_live + lane, &one, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (kf_scan >= 0) HIP_TRY(ctx, hipMemcpyAsync(e->kf_scan + lane, &kf_scan, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (K > 0) {
        hipLaunchKernelGGL(lane_kf_reset_kernel, dim3((K + 255) / 256), dim3(256), 0, ctx->stream, f, K,
                           e->vel + 3 * (size_t)lane, e->kf_und + (size_t)lane * KS * 2);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

int32_t roam_engine_set_features(roam_ctx *ctx, int32_t lane, const float *pts, int32_t K)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B && K >= 0 && K <= KS && (K == 0 || pts));
    return set_features_impl(ctx, e, lane, pts, K, e->last_scan[lane]);
}

int32_t roam_engine_init_lane(roam_ctx *ctx, int32_t lane, int32_t pool_idx, const float *pts, int32_t K,
                              const double *pose3)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B && pool_idx >= 0 && pool_idx < e->cfg.pool_scans && pose3 && K >= 0 && K <= KS);
    if (e->uploads_pending) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_up, 0));     // asynchronous uploads land first
    // previous-image pyramid of this lane from the pool scan
    uint8_t *pyr = e->pyr[e->cur] + (size_t)lane * e->pd.lane_stride;
    WarpSrc ws = {e->pool + (size_t)pool_idx * e->rec_bytes, 0, (int64_t)e->cfg.stride, e->cfg.payload_off, 1, nullptr};
    HIP_TRY(ctx, launch_warp_gather(ctx->stream, e->warp_map, ws, 1, e->cfg.rows, e->cfg.clip, pyr, e->pd.lane_stride, e->warp_dark_zero));
    HIP_TRY(ctx, launch_build_pyramid(ctx->stream, pyr, e->pd, 1, e->pyr_dark));
    double zero[3] = {0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(e->pose + 3 * (size_t)lane, pose3, sizeof(double) * 3, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(e->vel + 3 * (size_t)lane, zero, sizeof(double) * 3, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    e->prev_scan[lane] = pool_idx; e->lane_seen[lane] = e->slot_writes[(size_t)pool_idx];
    return set_features_impl(ctx, e, lane, pts, K, pool_idx);
}

int32_t roam_engine_init_lane_detect(roam_ctx *ctx, int32_t lane, int32_t pool_idx, const double *pose3)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B && pool_idx >= 0 && pool_idx < e->cfg.pool_scans && pose3);
    if (!e->rt_on) { ROAM_SET_ERR(ctx, "engine created without retrack_on_device"); return ROAM_E_STATE; }
    int32_t rc = roam_engine_init_lane(ctx, lane, pool_idx, nullptr, 0, pose3);      // pyramid, pose, zero velocity, empty keyframe
    if (rc != ROAM_OK) return rc;
    // first-frame appendNewFeatures(prevImgCart, empty) (RawROAMSystem.py:150): the retrack path for this one lane
    const int32_t one = 1;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(e->rt.rt_n, &one, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(e->rt.rt_lane, &lane, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(e->rt.rt_scan, &pool_idx, sizeof(int32_t), hipMemcpyHostToDevice, st));
    e->rt.res = nullptr;
    HIP_TRY(ctx, launch_retrack(st, e->rt, 1));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    e->lane_k[lane] = 320;
    return ROAM_OK;
}

// batched roam_engine_init_lane_detect for lanes lane0 .. lane0 + n - 1: one warp / pyramid launch over the n lanes and ONE
// detection pass (chunks of `retrack_slots`) instead of n single-lane passes of 2.4 ms each (4096 lanes: 10 s -> 0.3 s)
int32_t roam_engine_init_lanes_detect(roam_ctx *ctx, int32_t lane0, int32_t n, const int32_t *pool_idx, const double *poses3)
{
    ENGINE();
    ARG_CHECK(ctx, n >= 1 && lane0 >= 0 && lane0 + n <= e->B && pool_idx && poses3);
    if (!e->rt_on) { ROAM_SET_ERR(ctx, "engine created without retrack_on_device"); return ROAM_E_STATE; }
    for (int i = 0; i < n; i++) ARG_CHECK(ctx, pool_idx[i] >= 0 && pool_idx[i] < e->cfg.pool_scans);
    if (e->map_cap > 0) {                                   // the keyframe map freezes the replaced keyframes lane by lane
        for (int i = 0; i < n; i++) {
            const int32_t rc = roam_engine_init_lane_detect(ctx, lane0 + i, pool_idx[i], poses3 + 3 * (size_t)i);
            if (rc != ROAM_OK) return rc;
        }
        return ROAM_OK;
    }
    hipStream_t st = ctx->stream;
    if (e->uploads_pending) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_up, 0));
    std::vector<int32_t> lanes((size_t)n);
    for (int i = 0; i < n; i++) lanes[i] = lane0 + i;
    HIP_TRY(ctx, hipMemcpyAsync(e->rt.rt_n, &n, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(e->rt.rt_lane, lanes.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(e->rt.rt_scan, pool_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    // previous-image pyramids from the pool scans (lane i of the launch reads record rt_scan[i])
    uint8_t *pyr = e->pyr[e->cur] + (size_t)lane0 * e->pd.lane_stride;
    HIP_TRY(ctx, launch_warp_gather(st, e->warp_map, pool_warp_src(e, e->rt.rt_scan), n, e->cfg.rows, e->cfg.clip, pyr, e->pd.lane_stride, e->warp_dark_zero));
    HIP_TRY(ctx, launch_build_pyramid(st, pyr, e->pd, n, e->pyr_dark));
    // pose, zero velocity, empty feature set, keyframe at the pose created on the scan (set_features_impl with K = 0)
    HIP_TRY(ctx, hipMemcpyAsync(e->pose + 3 * (size_t)lane0, poses3, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(e->kf_pose + 3 * (size_t)lane0, poses3, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(e->vel + 3 * (size_t)lane0, 0, sizeof(double) * 3 * (size_t)n, st));
    HIP_TRY(ctx, hipMemsetAsync(e->kf_vel + 3 * (size_t)lane0, 0, sizeof(double) * 3 * (size_t)n, st));
    HIP_TRY(ctx, hipMemsetAsync(e->feat_n + lane0, 0, sizeof(int32_t) * (size_t)n, st));
    HIP_TRY(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(e->kf_live + lane0), 1, (size_t)n, st));
    HIP_TRY(ctx, hipMemcpyAsync(e->kf_scan + lane0, pool_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    // first-frame appendNewFeatures(prevImgCart, empty) (RawROAMSystem.py:150) for all n lanes
    e->rt.res = nullptr;
    HIP_TRY(ctx, launch_retrack(st, e->rt, n));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) {
        e->lane_k[lane0 + i] = 320;
        e->prev_scan[lane0 + i] = pool_idx[i]; e->lane_seen[lane0 + i] = e->slot_writes[(size_t)pool_idx[i]];
    }
    return ROAM_OK;
}

int32_t roam_engine_lane_features(roam_ctx *ctx, int32_t lane, float *pts, int32_t cap, int32_t *K)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B && pts && K && cap >= 0);
    int32_t n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, e->feat_n + lane, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *K = n;
    const int m = n < cap ? n : cap;
    if (m > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(pts, e->feat + (size_t)lane * KS * 2, sizeof(float) * 2 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return n > cap ? ROAM_E_CAPACITY : ROAM_OK;
}

int32_t roam_engine_lane_peaks(roam_ctx *ctx, int32_t lane, int32_t *out, int64_t cap, int64_t *n_out)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B && out && n_out && cap >= 0);
    int32_t n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, e->peaks_n[e->pk] + lane, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = n;
    int64_t m = n < cap ? n : cap;
    if (m > e->cfg.peaks_cap) m = e->cfg.peaks_cap;
    if (m > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(out, e->peaks_out[e->pk] + (size_t)lane * e->cfg.peaks_cap * 2, sizeof(int32_t) * 2 * (size_t)m,
                                    hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return (n > cap || n > e->cfg.peaks_cap) ? ROAM_E_CAPACITY : ROAM_OK;
}

int32_t roam_engine_doh_maxima(roam_ctx *ctx, int32_t pool_idx, const double *sigmas, int32_t num_sigma, double threshold,
                               int32_t *out_rcs, double *out_val, int32_t cap, int32_t *n_out)
{
    ENGINE();
    ARG_CHECK(ctx, pool_idx >= 0 && pool_idx < e->cfg.pool_scans);
    return roam_doh_maxima_record_device(ctx, e->pool + (size_t)pool_idx * e->rec_bytes, e->cfg.rows, e->cfg.stride,
                                         e->cfg.payload_off, e->cfg.clip, sigmas, num_sigma, threshold, out_rcs, out_val,
                                         cap, n_out);
}

int32_t roam_engine_fmt_rotation(roam_ctx *ctx, int32_t n, const int32_t *prev_pool_idx, const int32_t *curr_pool_idx, int32_t clip_px,
                                 int32_t downsample, double *out3)
{
    ENGINE();
    ARG_CHECK(ctx, n >= 1 && prev_pool_idx && curr_pool_idx && out3 && downsample >= 1 && e->cfg.rows >= 8);
    for (int i = 0; i < n; i++)
        ARG_CHECK(ctx, prev_pool_idx[i] >= 0 && prev_pool_idx[i] < e->cfg.pool_scans && curr_pool_idx[i] >= 0 && curr_pool_idx[i] < e->cfg.pool_scans);
    const int clip = (clip_px > 0 && clip_px < e->cfg.clip) ? clip_px : e->cfg.clip;
    const int R = clip / downsample;
    ARG_CHECK(ctx, R >= ROAM_FMT_MIN_R && R <= ROAM_FMT_MAX_R);
    // the pass runs on the compute stream, behind every step enqueued so far; asynchronous uploads land first (the newest upload's event
    // covers them all).  Nothing of the engine's bookkeeping changes: a later step still waits for its own uploads.
    if (e->uploads_pending) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_up, 0));
    FmtBatchIn in;
    in.pool = e->pool; in.rec_bytes = (int64_t)e->rec_bytes; in.rec_stride = e->cfg.stride; in.payload_off = e->cfg.payload_off;
    in.prev_idx = prev_pool_idx; in.curr_idx = curr_pool_idx;
    return roam_fmt_batch_run(ctx, in, n, e->cfg.rows, clip, R, out3, nullptr);
}

int32_t roam_engine_fmt_register(roam_ctx *ctx, int32_t n, const int32_t *prev_pool_idx, const int32_t *curr_pool_idx, int32_t clip_px,
                                 int32_t downsample, int32_t cart_downsample, double *out6)
{
    ENGINE();
    ARG_CHECK(ctx, n >= 1 && prev_pool_idx && curr_pool_idx && out6 && downsample >= 1 && cart_downsample >= 1 && e->cfg.rows >= 8);
    for (int i = 0; i < n; i++)
        ARG_CHECK(ctx, prev_pool_idx[i] >= 0 && prev_pool_idx[i] < e->cfg.pool_scans && curr_pool_idx[i] >= 0 && curr_pool_idx[i] < e->cfg.pool_scans);
    const int clip = (clip_px > 0 && clip_px < e->cfg.clip) ? clip_px : e->cfg.clip;
    const int R = clip / downsample, Rc = e->cfg.clip / cart_downsample;
    ARG_CHECK(ctx, R >= ROAM_FMT_MIN_R && R <= ROAM_FMT_MAX_R && Rc >= 1 && 2 * Rc <= 4096 && e->cfg.clip <= 16384);
    // as roam_engine_fmt_rotation: behind every step enqueued so far and the uploads of the pool, the engine's bookkeeping untouched
    if (e->uploads_pending) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_up, 0));
    FmtBatchIn in;
    in.pool = e->pool; in.rec_bytes = (int64_t)e->rec_bytes; in.rec_stride = e->cfg.stride; in.payload_off = e->cfg.payload_off;
    in.prev_idx = prev_pool_idx; in.curr_idx = curr_pool_idx;
    in.cols = e->cfg.clip;                                   // the Cartesian half reads the record's full clipped width
    return roam_fmt_register_run(ctx, in, n, e->cfg.rows, clip, R, Rc, out6, nullptr);
}

// the pool as the loop database's record entries read it.  As roam_engine_fmt_rotation: they run behind every step enqueued so far and
// the uploads of the pool, the engine's bookkeeping untouched
static LoopPool loop_pool(const roam_ctx *ctx, const Engine *e)
{
    return {e->pool, (int64_t)e->rec_bytes, e->cfg.stride, e->cfg.payload_off, e->cfg.rows, e->cfg.clip, e->uploads_pending ? ctx->ev_up : nullptr};
}

int32_t roam_engine_loop_db_add(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t clip_px, int32_t floor_code,
                                int32_t *first_index_out)
{
    return roam_engine_loop_db_add_motion(ctx, db, n, pool_idx, clip_px, floor_code, nullptr, 0.25, first_index_out);
}

int32_t roam_engine_loop_db_add_motion(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t clip_px, int32_t floor_code,
                                       const double *velocities, double period, int32_t *first_index_out)
{
    ENGINE();
    ARG_CHECK(ctx, db && n >= 1 && pool_idx);
    for (int i = 0; i < n; i++) ARG_CHECK(ctx, pool_idx[i] >= 0 && pool_idx[i] < e->cfg.pool_scans);
    return loop_records_append(ctx, db, loop_pool(ctx, e), n, pool_idx, clip_px, floor_code, first_index_out, velocities, period);
}

int32_t roam_engine_time_loop_describe(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t clip_px, int32_t floor_code,
                                       int32_t reps, float *ms_per_rep)
{
    ENGINE();
    ARG_CHECK(ctx, db && n >= 1 && pool_idx && ms_per_rep);
    for (int i = 0; i < n; i++) ARG_CHECK(ctx, pool_idx[i] >= 0 && pool_idx[i] < e->cfg.pool_scans);
    return loop_records_time_describe(ctx, db, loop_pool(ctx, e), n, pool_idx, clip_px, floor_code, reps, ms_per_rep);
}

int32_t roam_engine_time_loop_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t clip_px, int32_t floor_code,
                                      int32_t reps, float *ms_per_rep)
{
    ENGINE();
    ARG_CHECK(ctx, db && n >= 1 && pool_idx && ms_per_rep);
    for (int i = 0; i < n; i++) ARG_CHECK(ctx, pool_idx[i] >= 0 && pool_idx[i] < e->cfg.pool_scans);
    return loop_records_time_offsets(ctx, db, loop_pool(ctx, e), n, pool_idx, clip_px, floor_code, reps, ms_per_rep);
}

int32_t roam_engine_time_loop_cloud(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t reps, float *rows_ms,
                                    float *gather_ms)
{
    return roam_engine_time_loop_cloud_motion(ctx, db, n, pool_idx, nullptr, 0.25, reps, rows_ms, gather_ms);
}

int32_t roam_engine_time_loop_cloud_motion(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, const double *velocities,
                                           double period, int32_t reps, float *rows_ms, float *gather_ms)
{
    ENGINE();
    ARG_CHECK(ctx, db && n >= 1 && pool_idx && rows_ms && gather_ms);
    for (int i = 0; i < n; i++) ARG_CHECK(ctx, pool_idx[i] >= 0 && pool_idx[i] < e->cfg.pool_scans);
    float ms[2] = {0, 0};
    const int32_t rc = loop_records_time_cloud(ctx, db, loop_pool(ctx, e), n, pool_idx, reps, ms, velocities, period);
    *rows_ms = ms[0];
    *gather_ms = ms[1];
    return rc;
}

int32_t roam_engine_lane_image(roam_ctx *ctx, int32_t lane, int32_t level, uint8_t *out, int64_t cap)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B && level >= 0 && level < ROAM_PYR_LEVELS && out);
    const size_t n = (size_t)e->pd.w[level] * e->pd.h[level];
    ARG_CHECK(ctx, cap >= (int64_t)n);
    HIP_TRY(ctx, hipMemcpyAsync(out, e->pyr[e->cur] + (size_t)lane * e->pd.lane_stride + e->pd.off[level], n,
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

}  // extern "C"
