// Batched, device-resident scan-pair engine.
//
// B independent sequences ("lanes") live in HBM: the raw Oxford records (pool), a ring of
// four u8 pyramids per lane (previous / current / in the pyramid stage / being warped), the
// tracked feature set, the keyframe state (+ optionally every past keyframe, 8f-f1) and the
// poses.  One roam_engine_step() advances EVERY lane by one scan pair with ~15 kernel launches
// and no host round trip, in three pipelined stages (+ the peak kernel on a stream of its own):
//   P (depends only on the raw scan; joined before the result record):  ingest+peaks
//   A (depends only on the raw scan; issue-bound):                      warp+quantise
//   B (HBM-bound):                                                      pyramid
//   C: KLT -> (status & err<10) compaction -> consistency graph -> max clique ->
//      inlier compaction + keyframe pruning + p_w / p_jt -> Kabsch -> initial transform ->
//      motion-distortion LM (latency-bound) -> pose / keyframe bookkeeping
// so that when steps are enqueued back to back A(N+2), B(N+1) and C(N) share the GPU.
// It restates the body of RawROAMSystem.run's loop (reference RawROAMSystem.py:162-298)
// without the plotting, Tracker.track (Tracker.py:35-106) and the Keyframe bookkeeping
// (Mapping.py:37-66,97-125,149-174).  Scan pairs of different lanes are independent, so the
// batch dimension is what fills the 256 CUs; within a lane the chain is sequential.
#include "engine.h"
#include "kabsch_body.inc"
#include <new>

// ------------------------------------------------------------------------------ glue kernels
__device__ __forceinline__ int blk_excl_scan(int v, int *sh, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int n = __shfl_up(inc, d);
        if (lane >= d) inc += n;
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; i++) {
        int s = sh[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__global__ void new_sequence_kernel(int32_t *__restrict__ feat_n, const int32_t *__restrict__ flag, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && flag[b]) feat_n[b] = 0;
}

// G1: status &= err < ERR_THRESHOLD (getTransformKLT.py:365), ordered compaction of the good pairs
__global__ __launch_bounds__(256) void g1_good_kernel(const float *__restrict__ feat, const int32_t *__restrict__ feat_n,
                                                      const float *__restrict__ klt_next, uint8_t *__restrict__ status,
                                                      const float *__restrict__ err, float *__restrict__ good_old,
                                                      float *__restrict__ good_new, int32_t *__restrict__ good_idx,
                                                      int32_t *__restrict__ good_n, int kmax_launch)
{
    __shared__ int sh[8];
    const int b = blockIdx.x, t = threadIdx.x;
    const int K = min(feat_n[b], kmax_launch);          // (the tracker ran on kmax_launch features at most)
    const int items = (KS + 255) / 256;
    const int lo = t * items, hi = min(lo + items, K);
    int c = 0;
    for (int k = lo; k < hi; k++) {
        const int64_t i = (int64_t)b * KS + k;
        uint8_t s = status[i] & (uint8_t)(err[i] < ERR_THR);
        status[i] = s;
        c += s;
    }
    int total;
    int pos = blk_excl_scan(c, sh, &total);
    for (int k = lo; k < hi; k++) {
        const int64_t i = (int64_t)b * KS + k;
        if (status[i]) {
            const int64_t o = (int64_t)b * KS + pos;
            good_old[2 * o] = feat[2 * i]; good_old[2 * o + 1] = feat[2 * i + 1];
            good_new[2 * o] = klt_next[2 * i]; good_new[2 * o + 1] = klt_next[2 * i + 1];
            good_idx[o] = k;
            pos++;
        }
    }
    if (t == 0) good_n[b] = total;
}

__global__ void fill_mask_kernel(uint8_t *mask, const int32_t *good_n, int32_t *cq_n, int32_t *cq_flags)
{
    const int b = blockIdx.x;
    for (int k = threadIdx.x; k < KS; k += blockDim.x) mask[(int64_t)b * KS + k] = 1;
    if (threadIdx.x == 0) { cq_n[b] = good_n[b]; cq_flags[b] = 1; }
}

// G2: inlier compaction (Tracker.py:93-104), keyframe pruning (Mapping.py:118-125), Kabsch inputs,
//     p_w (Mapping.py:97-116), centered_new (RawROAMSystem.py:198-199), next feature set (:296)
__global__ __launch_bounds__(256) void g2_inliers_kernel(const float *__restrict__ good_old, const float *__restrict__ good_new,
                                                         const int32_t *__restrict__ good_idx, const int32_t *__restrict__ good_n,
                                                         const uint8_t *__restrict__ mask, const double *__restrict__ kf_pose,
                                                         const double *__restrict__ kf_und, double *__restrict__ kf_und_tmp,
                                                         double *__restrict__ kab_src, double *__restrict__ kab_tgt,
                                                         double *__restrict__ p_w, double *__restrict__ p_jt,
                                                         float *__restrict__ feat, int32_t *__restrict__ in_n,
                                                         double *__restrict__ kab_out, const double *__restrict__ pose,
                                                         double *__restrict__ T_wj0, double *__restrict__ T_init)
{
    __shared__ int sh[8];
    __shared__ double red[8];
    const int b = blockIdx.x, t = threadIdx.x;
    const int G = good_n[b];
    const int items = (KS + 255) / 256;
    const int lo = t * items, hi = min(lo + items, G);
    int c = 0;
    for (int g = lo; g < hi; g++) c += mask[(int64_t)b * KS + g] ? 1 : 0;
    int total;
    int pos = blk_excl_scan(c, sh, &total);
    const double kx = kf_pose[3 * b], ky = kf_pose[3 * b + 1], kth = kf_pose[3 * b + 2];
    const double ck = cos(kth), sk = sin(kth);
    for (int g = lo; g < hi; g++) {
        const int64_t i = (int64_t)b * KS + g;
        if (!mask[i]) continue;
        const int64_t o = (int64_t)b * KS + pos;
        const float ox = good_old[2 * i], oy = good_old[2 * i + 1];
        const float nx = good_new[2 * i], ny = good_new[2 * i + 1];
        kab_src[2 * o] = (double)ox; kab_src[2 * o + 1] = (double)oy;
        kab_tgt[2 * o] = (double)nx; kab_tgt[2 * o + 1] = (double)ny;
        const int64_t ki = (int64_t)b * KS + good_idx[i];
        const double ux = kf_und[2 * ki], uy = kf_und[2 * ki + 1];
        kf_und_tmp[2 * o] = ux; kf_und_tmp[2 * o + 1] = uy;
        p_w[2 * o] = ck * ux - sk * uy + kx;
        p_w[2 * o + 1] = sk * ux + ck * uy + ky;
        p_jt[2 * o] = ((double)nx - CART_CENTER) * M_PER_PX;
        p_jt[2 * o + 1] = ((double)ny - CART_CENTER) * M_PER_PX;
        pos++;
    }
    __syncthreads();
    // blobCoord = good_new.copy(): write after every read of good_* (distinct buffers, so no hazard)
    pos -= c;
    for (int g = lo; g < hi; g++) {
        const int64_t i = (int64_t)b * KS + g;
        if (!mask[i]) continue;
        const int64_t o = (int64_t)b * KS + pos;
        feat[2 * o] = good_new[2 * i]; feat[2 * o + 1] = good_new[2 * i + 1];
        pos++;
    }
    if (t == 0) in_n[b] = total;
    // The Kabsch fit of the lane's inliers (getTransformKLT.calculateTransformSVD) and, with motion distortion, the LM's two transforms
    // (G3) by the same workgroup: kernels of their own until round 6 - two launches less in the chain of a step (a single sequence's pair is
    // a chain of ~20 launches of 4-6 us each on the device and on the enqueuing thread)
    __threadfence_block();
    __syncthreads();
    double *ko = kab_out + 6 * (int64_t)b;
    kabsch_body(kab_src + (int64_t)b * KS * 2, kab_tgt + (int64_t)b * KS * 2, total, red, ko);
    if (T_wj0 && t == 0) {
        const double x = pose[3 * b], y = pose[3 * b + 1], th = pose[3 * b + 2];
        const double c = cos(th), s = sin(th);
        double *T0 = T_wj0 + 9 * (int64_t)b, *Ti = T_init + 9 * (int64_t)b;
        T0[0] = c; T0[1] = -s; T0[2] = x; T0[3] = s; T0[4] = c; T0[5] = y; T0[6] = 0; T0[7] = 0; T0[8] = 1;
        const double hx = ko[4] * M_PER_PX, hy = ko[5] * M_PER_PX;
        Ti[0] = c * ko[0] - s * ko[2]; Ti[1] = c * ko[1] - s * ko[3]; Ti[2] = c * hx - s * hy + x;
        Ti[3] = s * ko[0] + c * ko[2]; Ti[4] = s * ko[1] + c * ko[3]; Ti[5] = s * hx + c * hy + y;
        Ti[6] = 0; Ti[7] = 0; Ti[8] = 1;
    }
}

// (G3 - h *= 0.0864 (Tracker.py:124-125); T_wj = prev_pose @ [[R,h],[0,0,1]] (RawROAMSystem.py:201) - is the tail of g2_inliers_kernel)

// G4: pose / velocity update, keyframe criteria (Mapping.py:149-174, RawROAMSystem.py:250-271),
//     possible_kf.updateInfo undistortion (Mapping.py:65), result record
__global__ __launch_bounds__(256) void g4_update_kernel(roam_engine_cfg cfg, const double *__restrict__ lm_out,
                                                        const int32_t *__restrict__ lm_nfev, const int32_t *__restrict__ lm_info,
                                                        const double *__restrict__ kab_out, double *__restrict__ pose,
                                                        double *__restrict__ vel, double *__restrict__ kf_pose,
                                                        double *__restrict__ kf_und, const double *__restrict__ kf_und_tmp,
                                                        const double *__restrict__ p_jt, const int32_t *__restrict__ in_n,
                                                        const int32_t *__restrict__ good_n, int32_t *__restrict__ feat_n,
                                                        const int32_t *__restrict__ peaks_n, const int32_t *__restrict__ cq_flags,
                                                        roam_lane_result *__restrict__ res, const int32_t *__restrict__ scan_idx,
                                                        double *__restrict__ kf_vel, int32_t *__restrict__ kf_scan,
                                                        int32_t *__restrict__ kf_fresh, const int32_t *__restrict__ kf_live,
                                                        double *__restrict__ map_store, int32_t *__restrict__ map_n, int map_cap,
                                                        int collect, int32_t *__restrict__ rt_lane, int32_t *__restrict__ rt_scan,
                                                        int32_t *__restrict__ rt_n)
{
    __shared__ double np_[3], nv_[3];
    __shared__ int newkf;
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = in_n[b];
    if (t == 0) {
        double px = pose[3 * b], py = pose[3 * b + 1], pth = pose[3 * b + 2];
        double v0 = 0, v1 = 0, v2 = 0;
        const double *k = kab_out + 6 * (int64_t)b;
        if (n >= 2) {
            if (cfg.motion_distortion) {
                const double *s = lm_out + 6 * (int64_t)b;
                v0 = s[0]; v1 = s[1]; v2 = s[2]; px = s[3]; py = s[4]; pth = s[5];
            } else {
                // updateTrajectory: convertRandHtoDeltas + appendRelativeDeltas (utils.py:99-103, trajectoryPlotting.py:28-35)
                const double dx = k[4] * M_PER_PX, dy = k[5] * M_PER_PX, dth = atan2(k[2], k[0]);
                const double c = cos(pth), s = sin(pth);
                px += dx * c - dy * s; py += dx * s + dy * c; pth += dth;
            }
        }
        np_[0] = px; np_[1] = py; np_[2] = pth; nv_[0] = v0; nv_[1] = v1; nv_[2] = v2;
        const int retrack = n <= N_RETRACK;
        const double dth = fabs(kf_pose[3 * b + 2] - pth);
        const double ddx = kf_pose[3 * b] - px, ddy = kf_pose[3 * b + 1] - py;
        const int good = (dth >= cfg.keyframe_rot_rad) || (ddx * ddx + ddy * ddy >= cfg.keyframe_trans_m * cfg.keyframe_trans_m);
        newkf = retrack || good;
        roam_lane_result *r = res + b;
        r->pose[0] = px; r->pose[1] = py; r->pose[2] = pth;
        r->velocity[0] = v0; r->velocity[1] = v1; r->velocity[2] = v2;
        r->kabsch_R[0] = k[0]; r->kabsch_R[1] = k[1]; r->kabsch_R[2] = k[2]; r->kabsch_R[3] = k[3];
        r->kabsch_h[0] = k[4] * M_PER_PX; r->kabsch_h[1] = k[5] * M_PER_PX;
        r->n_tracked = feat_n[b]; r->n_good = good_n[b]; r->n_inliers = n; r->n_peaks = peaks_n[b];
        r->lm_nfev = (n >= 2 && cfg.motion_distortion) ? lm_nfev[b] : 0;
        r->lm_info = (n >= 2 && cfg.motion_distortion) ? lm_info[b] : 0;
        // (a device-scope atomic store: the last block of this kernel reads every lane's flags, possibly from another XCD - see below)
        __hip_atomic_store(&r->flags, (cq_flags[b] & 1) | (newkf ? 2 : 0) | (retrack ? 4 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        r->n_after_retrack = 0;
    }
    __syncthreads();
    const double v0 = nv_[0], v1 = nv_[1], v2 = nv_[2];
    // a keyframe that is replaced keeps its final state (pose, creation velocity, pruned locals) in the map
    const int mslot = (newkf && map_cap > 0 && kf_live[b]) ? map_n[b] : -1;
    if (mslot >= 0) map_freeze(map_store, map_n, map_cap, b, kf_pose + 3 * b, kf_vel + 3 * b, n, kf_scan[b], kf_und_tmp + (int64_t)b * KS * 2);
    for (int j = t; j < n; j += 256) {
        const int64_t o = (int64_t)b * KS + j;
        if (newkf) {
            const double x = p_jt[2 * o], y = p_jt[2 * o + 1];
            const double dT = 0.25 * atan2(-y, -x) / TWO_PI;
            const double a = v2 * dT, ca = cos(a), sa = sin(a);
            kf_und[2 * o] = ca * x - sa * y + v0 * dT;
            kf_und[2 * o + 1] = sa * x + ca * y + v1 * dT;
        } else {
            kf_und[2 * o] = kf_und_tmp[2 * o]; kf_und[2 * o + 1] = kf_und_tmp[2 * o + 1];
        }
    }
    __syncthreads();
    if (t == 0) {
        pose[3 * b] = np_[0]; pose[3 * b + 1] = np_[1]; pose[3 * b + 2] = np_[2];
        vel[3 * b] = v0; vel[3 * b + 1] = v1; vel[3 * b + 2] = v2;
        if (newkf) {
            kf_pose[3 * b] = np_[0]; kf_pose[3 * b + 1] = np_[1]; kf_pose[3 * b + 2] = np_[2];
            kf_vel[3 * b] = v0; kf_vel[3 * b + 1] = v1; kf_vel[3 * b + 2] = v2;
            kf_scan[b] = scan_idx[b];
            if (mslot >= 0 && mslot < map_cap) map_n[b] = mslot + 1;
        }
        kf_fresh[b] = newkf;
        feat_n[b] = n;
    }
    // The list of the lanes that re-detect (rt_collect_kernel's job: lane order, so one block) by the block that finishes LAST: one launch
    // less in the chain every step enqueues (a kernel that only returns costs ~4-6 us of a single sequence's 290 us pair).
    // collect: 0 none, 1 lanes with flag bit 2, 2 every lane; rt_n[1] counts the finished blocks and is left at zero
    if (collect) {
        __shared__ int last_s, sh[4], base_s;
        // (no __threadfence(): on this GPU it writes the XCD's whole L2 back; the flags travel as device-scope atomics, the counter after them)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "g4_update_kernel's hand-off to its last block relies on gfx94x/95x storing with write-through and counting stores in vmcnt: s_waitcnt vmcnt(0) + relaxed atomics, no release/acquire pair"
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) last_s = atomicAdd(rt_n + 1, 1) == (int)gridDim.x - 1;
        __syncthreads();
        if (!last_s) return;
        const int B = (int)gridDim.x;
        if (t == 0) base_s = 0;
        __syncthreads();
        for (int b0 = 0; b0 < B; b0 += 256) {
            const int bb = b0 + t;
            const int f = (bb < B && (collect == 2 || (__hip_atomic_load(&res[bb].flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 4))) ? 1 : 0;
            const int lane = t & 63, w = t >> 6;
            int inc = f;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int nn = __shfl_up(inc, d); if (lane >= d) inc += nn; }
            if (lane == 63) sh[w] = inc;
            __syncthreads();
            int off = base_s, tot = 0;
            for (int i = 0; i < 4; i++) { if (i < w) off += sh[i]; tot += sh[i]; }
            if (f) { rt_lane[off + inc - 1] = bb; rt_scan[off + inc - 1] = scan_idx[bb]; }
            __syncthreads();
            if (t == 0) base_s += tot;
            __syncthreads();
        }
        if (t == 0) { rt_n[0] = base_s; rt_n[1] = 0; }
    }
}

// f2 ingest: record i, rows 4 per workgroup (one wavefront per row): bytes [0, width) of every row from pinned host memory
// into the pool.  Source rows start at arbitrary alignment (stride 3779), so a lane loads 16 bytes at byte granularity
// through a packed unaligned vector type and stores them unaligned as well; the tail is copied byte-wise.
typedef uint32_t u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));
__global__ __launch_bounds__(256) void ingest_rows_kernel(const uint8_t *__restrict__ host, int64_t host_stride, uint8_t *__restrict__ pool,
                                                          int64_t rec_bytes, int rows, int stride, int width)
{
    const int rec = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const uint8_t *s = host + (int64_t)rec * host_stride + (int64_t)row * stride;
    uint8_t *d = pool + (int64_t)rec * rec_bytes + (int64_t)row * stride;
    const int nvec = width / 16;
    for (int v = lane; v < nvec; v += 64) *reinterpret_cast<u32x4_a1 *>(d + 16 * v) = *reinterpret_cast<const u32x4_a1 *>(s + 16 * v);
    for (int b = nvec * 16 + lane; b < width; b += 64) d[b] = s[b];
}

// ------------------------------------------------------------------------------ API
extern "C" {

// the in-step prior's resources; the caller has waited for the enqueued steps
static void auto_prior_release(Engine *e)
{
    if (e->ap_stream) { (void)hipStreamSynchronize(e->ap_stream); (void)hipStreamDestroy(e->ap_stream); e->ap_stream = nullptr; }
    if (e->ap_ev) { (void)hipEventDestroy(e->ap_ev); e->ap_ev = nullptr; }
    roam_fmt_auto_free(e->ap); e->ap = nullptr;
    if (e->ap_slab) { (void)hipFree(e->ap_slab); e->ap_slab = nullptr; }
    if (e->ap_rec_host) { (void)hipHostFree(e->ap_rec_host); e->ap_rec_host = nullptr; }
    e->ap_rec = nullptr;
    for (auto &st : e->ap_rec_step) st = -1;
}

int32_t roam_engine_destroy(roam_ctx *ctx)
{
    if (!ctx) return ROAM_E_ARG;
    Engine *e = ctx->engine;
    if (!e) return ROAM_OK;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    auto_prior_release(e);
    for (void *p : e->allocs) hipFree(p);
    if (e->scan_host) hipHostFree(e->scan_host);
    if (e->prior_host) hipHostFree(e->prior_host);
    if (e->results_host) hipHostFree(e->results_host);
    if (e->st_comm) { hipStreamSynchronize(e->st_comm); hipStreamDestroy(e->st_comm); }
    // (only events that were created are listed, so a creation that failed half way leaks nothing)
    for (hipEvent_t *ev : e->events) { hipEventDestroy(*ev); *ev = nullptr; }
    hipStreamSynchronize(ctx->stream2);
    hipStreamSynchronize(ctx->stream4);
    delete e;
    ctx->engine = nullptr;
    return ROAM_OK;
}

// everything of a new engine behind the empty struct: buffers, events, tables.  A failure returns with the error text set, and what exists
// by then is listed in the engine (allocs, events) or named by its members: roam_engine_destroy takes it all (roam_engine_create)
static int32_t engine_build(roam_ctx *ctx, Engine *e, const roam_engine_cfg *cfg)
{
    e->cfg = *cfg;
    if (!(e->cfg.keyframe_trans_m > 0.0)) e->cfg.keyframe_trans_m = 2.0;        // Mapping.py:14
    if (!(e->cfg.keyframe_rot_rad > 0.0)) e->cfg.keyframe_rot_rad = ROT_THR;      // Mapping.py:13
    const int B = e->B = cfg->lanes;
    e->lane_k.assign(B, 0);
    e->new_seq.assign(B, 0);
    e->last_scan.assign(B, -1);
    e->prev_scan.assign(B, -1);
    e->lane_seen.assign(B, 0);
    e->slot_writes.assign((size_t)cfg->pool_scans, 0);
    e->W = 2 * (cfg->clip / 2);
    e->stage_cap = (cfg->clip + 1) / 2;
    pyr_desc_init(&e->pd, e->W, e->W);
    e->rec_bytes = (size_t)cfg->rows * cfg->stride;
    const int nw = KS / 64;
    bool ok = true;
    ok = ok && dalloc(ctx, e, &e->pool, e->rec_bytes * cfg->pool_scans + 64);      // + slack: the warp stages its boxes with dword loads
    ok = ok && dalloc(ctx, e, &e->pyr[0], (size_t)e->pd.lane_stride * B);
    ok = ok && dalloc(ctx, e, &e->pyr[1], (size_t)e->pd.lane_stride * B);
    ok = ok && dalloc(ctx, e, &e->pyr[2], (size_t)e->pd.lane_stride * B);
    ok = ok && dalloc(ctx, e, &e->pyr[3], (size_t)e->pd.lane_stride * B);
    ok = ok && dalloc(ctx, e, &e->pyr_dark, pyr_dark_words(e->W));
    ok = ok && dalloc(ctx, e, &e->warp_map, (size_t)e->W * e->W);
    ok = ok && dalloc(ctx, e, &e->row_stage, (size_t)B * cfg->rows * e->stage_cap);
    ok = ok && dalloc(ctx, e, &e->row_count, (size_t)B * cfg->rows);
    for (int i = 0; i < 3; i++) {
        ok = ok && dalloc(ctx, e, &e->peaks_out[i], (size_t)B * cfg->peaks_cap * 2);
        ok = ok && dalloc(ctx, e, &e->peaks_n[i], (size_t)B);
        ok = ok && dalloc(ctx, e, &e->scan_idx[i], 2 * (size_t)B);     // [0, B): pool scan of each lane; [B, 2B): 1 = the lane starts a new sequence
    }
    if (ok && hipHostMalloc(reinterpret_cast<void **>(&e->scan_host), sizeof(int32_t) * 6 * (size_t)B, hipHostMallocDefault) != hipSuccess) {
        ROAM_SET_ERR(ctx, "engine: hipHostMalloc failed"); ok = false;
    }
    e->prior_bytes = ((size_t)B * 25 + 15) & ~(size_t)15;
    if (ok && hipHostMalloc(reinterpret_cast<void **>(&e->prior_host), 4 * e->prior_bytes, hipHostMallocDefault) != hipSuccess) {
        ROAM_SET_ERR(ctx, "engine: hipHostMalloc failed"); ok = false;
    }
    ok = ok && dalloc(ctx, e, &e->prior_dev, 4 * e->prior_bytes);
    ok = ok && dalloc(ctx, e, &e->feat, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->feat_n, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->klt_next, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->klt_err, (size_t)B * KS);
    ok = ok && dalloc(ctx, e, &e->klt_status, (size_t)B * KS);
    ok = ok && dalloc(ctx, e, &e->good_old, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->good_new, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->good_idx, (size_t)B * KS);
    ok = ok && dalloc(ctx, e, &e->good_n, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->adj, (size_t)B * KS * nw);
    ok = ok && dalloc(ctx, e, &e->cq_stack, (size_t)B * (KS + 2) * 2 * nw);
    ok = ok && dalloc(ctx, e, &e->cq_order, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->cq_mask, (size_t)B * KS);
    ok = ok && dalloc(ctx, e, &e->cq_n, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->cq_flags, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->kab_src, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->kab_tgt, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->kab_out, (size_t)B * 6);
    ok = ok && dalloc(ctx, e, &e->in_n, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->kf_pose, (size_t)B * 3);
    ok = ok && dalloc(ctx, e, &e->kf_vel, (size_t)B * 3) && dalloc(ctx, e, &e->kf_scan, (size_t)B) && dalloc(ctx, e, &e->kf_fresh, (size_t)B) &&
         dalloc(ctx, e, &e->kf_live, (size_t)B) && dalloc(ctx, e, &e->map_n, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->kf_und, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->kf_und_tmp, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->pose, (size_t)B * 3);
    ok = ok && dalloc(ctx, e, &e->vel, (size_t)B * 3);
    ok = ok && dalloc(ctx, e, &e->T_wj0, (size_t)B * 9);
    ok = ok && dalloc(ctx, e, &e->T_init, (size_t)B * 9);
    ok = ok && dalloc(ctx, e, &e->p_w, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->p_jt, (size_t)B * KS * 2);
    ok = ok && dalloc(ctx, e, &e->lm_work, (size_t)B * ((size_t)(2 * KS + 3) * 9 + KS));
    ok = ok && dalloc(ctx, e, &e->lm_out, (size_t)B * 6);
    ok = ok && dalloc(ctx, e, &e->lm_nfev, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->lm_big, (size_t)2 * (1 + B));
    ok = ok && dalloc(ctx, e, &e->lm_info, (size_t)B);
    ok = ok && dalloc(ctx, e, &e->results, (size_t)B * RES_RING);
    if (ok && hipHostMalloc(reinterpret_cast<void **>(&e->results_host), sizeof(roam_lane_result) * (size_t)B * RES_RING, hipHostMallocDefault) != hipSuccess) {
        ROAM_SET_ERR(ctx, "engine: hipHostMalloc failed"); ok = false;
    }
    { const char *se = getenv("ROAM_STAGE_EVENTS"); e->stage_ev = !(se && se[0] == '0'); e->stage_ev_forced = se && (se[0] == '0' || se[0] == '1'); }
    e->rt_on = cfg->retrack_on_device != 0;
    if (ok && e->rt_on) {
        // device-side feature (re)detection: DEFAULT_FEATURE_PARAMS of getFeatures.py:13-18, i.e. sigma = linspace(0.01, 10, 3)
        RtArgs &r = e->rt;
        memset(&r, 0, sizeof(r));
        const double step = (10.0 - 0.01) / 2.0;                         // numpy.linspace: arange(num) * step + start, last = stop
        r.sigma1 = 1.0 * step + 0.01; r.sigma2 = 10.0; r.threshold = 0.0005;
        r.size1 = (int)(3 * r.sigma1); r.size2 = (int)(3 * r.sigma2);
        r.W = e->W; r.rows = cfg->rows; r.cols = cfg->clip; r.stride = cfg->stride; r.payload_off = cfg->payload_off;
        r.rec_bytes = (int64_t)e->rec_bytes;
        const int R = r.slots = std::max(1, std::min(B, cfg->retrack_slots > 0 ? cfg->retrack_slots : 2048));      // (round 6: 512 -> 2048, +2.5 % on the default workload)
        const size_t npx = (size_t)e->W * e->W;
        if (e->W > 2048) { ROAM_SET_ERR(ctx, "engine: device retrack needs a Cartesian image of at most 2048 x 2048"); return ROAM_E_ARG; }
        ok = ok && dalloc(ctx, e, &r.rt_n, 2) && dalloc(ctx, e, &r.rt_lane, (size_t)B) && dalloc(ctx, e, &r.rt_scan, (size_t)B);
        // rows of the integral image start on 128-byte lines: a wave's 512-byte store then fills four whole lines (with the natural
        // pitch of 2024 doubles HBM saw 1.44 x the bytes written)
        r.SP = (e->W + 15) & ~15;
        ok = ok && dalloc(ctx, e, &r.S, (size_t)r.SP * e->W * R);
        ok = ok && dalloc(ctx, e, const_cast<uint32_t **>(&r.boxtab), retrack_boxtab_words(e->W));
        ok = ok && dalloc(ctx, e, const_cast<uint32_t **>(&r.darktab), retrack_darktab_words(e->W));
        ok = ok && dalloc(ctx, e, const_cast<uint32_t **>(&r.phlist), retrack_phase_words(e->W));
        ok = ok && dalloc(ctx, e, &r.colT, (size_t)std::min(R, RT_TWO_PASS_SLOTS) * ((e->W + 63) / 64) * e->W);
        ok = ok && dalloc(ctx, e, &r.col_done, (size_t)std::min(R, RT_TWO_PASS_SLOTS) * 64);
        // the fused detection kernel (retrack_fused.inc: integral image + determinants + maxima without the float64 image in HBM) serves
        // chunks of >= RT_TWO_PASS_SLOTS detections when ROAM_FUSED_DETECT=1 asks for it.  It is bit-identical to the two-kernel form
        // (tests/test_gpu_fused_detect.py) and MEASURED SLOWER - 27 ms against 12.6 ms per 512 detections, DESIGN.md section 6e: the path is
        // bound by instruction issue, not by HBM - so the two-kernel form stays the default.  Its tables: transposed sampling map,
        // footprints and dark steps per band; per slot: two hand-off buffers + the column totals
        {
            // (its buffers - 1 MB of hand-off scratch per slot, 0.55 GB at 512 slots, and three tables - exist only when the variant is
            // asked for: by the environment here, by roam_engine_debug_detect / roam_engine_time_kernel("doh_fused") on first use)
            const char *fv = getenv("ROAM_FUSED_DETECT");
            r.fused = (fv && fv[0] == '1') ? 1 : 0;
            // the determinants of a chunk of 1 024 detections beside the next chunk's integral images (launch_retrack; +1.7 %); needs both
            // halves of a 2 048-slot scratch.  ROAM_DET_SIDE=0: one launch of each kernel per chunk of `slots`, as until late round 6
            e->det_side.chunk = getenv("ROAM_DET_SIDE") ? atoi(getenv("ROAM_DET_SIDE")) : ((B >= 2048 && r.slots >= 2048) ? 1024 : 0);
            r.fd_halo_words = (int64_t)retrack_fused_halo_words(e->W);
        }
        // candidate lists and bookkeeping tables per DETECTION (0.9 MB each): K4-K7 run once per step over all of them
        const size_t D = (size_t)B;
        ok = ok && dalloc(ctx, e, &r.cand_rc, D * BP_MAX_PTS) && dalloc(ctx, e, &r.cand_val, D * BP_MAX_PTS) && dalloc(ctx, e, &r.cand_n, D);
        ok = ok && dalloc(ctx, e, &r.tasks, D * BP_MAX_TASKS) && dalloc(ctx, e, &r.pairs, D * (BP_MAX_PAIRS + 1));
        ok = ok && dalloc(ctx, e, &r.order, D * (BP_MAX_PAIRS + 1)) && dalloc(ctx, e, &r.ovbits, D * ((BP_MAX_PAIRS + 31) / 32 + 1));
        ok = ok && dalloc(ctx, e, &r.bigtab, D * 2 * 131072);
        ok = ok && dalloc(ctx, e, &r.kp, D * BP_MAX_PTS * 3) && dalloc(ctx, e, &r.kp_n, D) && dalloc(ctx, e, &r.slot_flags, D);
        ok = ok && dalloc(ctx, e, &r.ssc_work, D * 4 * BP_MAX_PTS) && dalloc(ctx, e, &r.sel, D * BP_MAX_PTS) && dalloc(ctx, e, &r.sel_n, D) && dalloc(ctx, e, &r.blob_order_buf, D);
    }
    if (!ok) return ROAM_E_HIP;
    if (e->rt_on) {
        if (hipError_t er = retrack_init(); er != hipSuccess) {
            ROAM_SET_ERR(ctx, "retrack_init failed: %s", hipGetErrorString(er));
            return ROAM_E_HIP;
        }
        RtArgs &r = e->rt;
        r.pool = e->pool; r.map = e->warp_map; r.feat = e->feat; r.feat_n = e->feat_n; r.vel = e->vel; r.kf_und = e->kf_und; r.res = nullptr;
    }
    for (auto &ev : e->ev_res) ok = ok && new_event(ctx, e, &ev, hipEventDisableTiming);
    e->slot_seq.assign((size_t)cfg->pool_scans, 0);
    for (auto &ev : e->ev_up_ring) ok = ok && new_event(ctx, e, &ev, hipEventDisableTiming);
    ok = ok && new_event(ctx, e, &e->ev_pool, hipEventDisableTiming);
    for (auto &ev : e->ev) ok = ok && new_event(ctx, e, &ev, hipEventDefault);
    ok = ok && new_event(ctx, e, &e->ev_join, hipEventDefault) && new_event(ctx, e, &e->ev_pk0, hipEventDefault) && new_event(ctx, e, &e->ev_pk1, hipEventDefault);
    ok = ok && new_event(ctx, e, &e->ev_warp, hipEventDisableTiming) && new_event(ctx, e, &e->ev_idx, hipEventDisableTiming) && new_event(ctx, e, &e->ev_peaks, hipEventDisableTiming);
    for (int i = 0; i < 4; i++) ok = ok && new_event(ctx, e, &e->ev_klt[i], hipEventDisableTiming) && new_event(ctx, e, &e->ev_g4[i], hipEventDisableTiming);
    if (!ok) return ROAM_E_HIP;
    // (the 64 x (6 + 3 x RT_TRACE_CHUNKS) timestamp events of the per-step traces are created by the first step that records into a slot:
    // creating all of them here was ~5 ms of the 13.6 ms a single sequence's engine cost to set up and tear down, recorded or not)
    HIP_TRY(ctx, launch_warp_map(ctx->stream, cfg->rows, cfg->clip, e->warp_map));
    HIP_TRY(ctx, launch_pyr_dark(ctx->stream, e->warp_map, e->W, e->W, cfg->clip, e->pyr_dark));
    if (e->rt_on) HIP_TRY(ctx, launch_retrack_boxtab(ctx->stream, e->warp_map, e->W, cfg->clip, const_cast<uint32_t *>(e->rt.boxtab)));
    if (e->rt_on) HIP_TRY(ctx, launch_retrack_darktab(ctx->stream, e->warp_map, e->W, cfg->clip, const_cast<uint32_t *>(e->rt.darktab)));
    if (e->rt_on && e->rt.fused) ROAM_TRY(fused_tables(ctx, e));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    e->rt_image_px = (int64_t)e->W * e->W;
    if (e->rt_on && e->W <= 2048 && B >= RT_TWO_PASS_SLOTS) {
        e->rt_image_px = 0;
        // (an engine of fewer lanes never launches the one-sweep kernel: a single sequence's engine skips these ~5 ms of its set-up)
        // the phases the one-sweep integral kernel walks: from the sampling map and the dark-step table just made (host code, once)
        // (through PINNED staging: a pageable hipMemcpy of this size leaves the runtime in a state in which the small device-to-device
        // copy of the keyframe exchange costs 80 us more per step - measured, round 6)
        const size_t npx = (size_t)e->W * e->W, ndt = retrack_darktab_words(e->W), nph = retrack_phase_words(e->W);
        uint32_t *stage = nullptr;
        HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&stage), (npx + ndt + nph) * 4, hipHostMallocDefault));
        uint32_t *mh = stage, *dh = stage + npx;
        std::vector<uint32_t> ph(nph, 0u);
        hipError_t ec = hipMemcpyAsync(mh, e->warp_map, npx * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (ec == hipSuccess) ec = hipMemcpyAsync(dh, e->rt.darktab, ndt * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (ec == hipSuccess) ec = hipStreamSynchronize(ctx->stream);
        bool okp = ec == hipSuccess && retrack_build_phases(mh, dh, e->W, cfg->clip, ph.data());
        if (okp) {
            memcpy(stage + npx + ndt, ph.data(), nph * 4);
            ec = hipMemcpyAsync(const_cast<uint32_t *>(e->rt.phlist), stage + npx + ndt, nph * 4, hipMemcpyHostToDevice, ctx->stream);
            if (ec == hipSuccess) ec = hipStreamSynchronize(ctx->stream);
        }
        (void)hipHostFree(stage);
        if (!okp || ec != hipSuccess) { ROAM_SET_ERR(ctx, "retrack: phase list (%s)", ec != hipSuccess ? hipGetErrorString(ec) : "image too large"); return ec != hipSuccess ? ROAM_E_HIP : ROAM_E_ARG; }
        e->rt_image_px = retrack_phase_pixels(ph.data(), e->W);
    }
    return ROAM_OK;
}

int32_t roam_engine_create(roam_ctx *ctx, const roam_engine_cfg *cfg)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // rows >= 2: the sampling map reaches iy == rows + 1 (a tap row of weight zero) and the warp and the re-detection's integral wrap a
    // staged polar row ONCE, to row 1 - with one azimuth that is the next record, or past the pool (docs/KERNELS.md, warp_gather_kernel)
    ARG_CHECK(ctx, cfg && cfg->lanes >= 1 && cfg->rows >= 2 && cfg->rows <= 1020 && cfg->clip >= 32 && cfg->clip <= 4094 && (cfg->clip / 2) % 2 == 0 &&
                       (int64_t)cfg->rows * cfg->stride < (1ll << 30) &&
                       cfg->payload_off >= 0 && cfg->stride >= cfg->payload_off + cfg->clip && cfg->pool_scans >= 1 &&
                       cfg->peaks_cap >= 1);
    roam_engine_destroy(ctx);
    Engine *e = new (std::nothrow) Engine();
    if (!e) return ROAM_E_HIP;
    ctx->engine = e;
    // one failure exit: whatever engine_build had made by then goes with the engine, and the context is left without one
    const int32_t rc = engine_build(ctx, e, cfg);
    if (rc != ROAM_OK) roam_engine_destroy(ctx);
    return rc;
}

int32_t roam_engine_upload_scan(roam_ctx *ctx, int32_t pool_idx, const uint8_t *rec)
{
    ENGINE();
    ARG_CHECK(ctx, rec && pool_idx >= 0 && pool_idx < e->cfg.pool_scans);
    e->slot_writes[(size_t)pool_idx]++;
    HIP_TRY(ctx, hipMemcpyAsync(e->pool + (size_t)pool_idx * e->rec_bytes, rec, e->rec_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

// f2 (raw-record ingest): records stream from PINNED host memory on the copy stream while the main
// stream computes.  Protocol for a double-buffered pool (halves A/B):
//   roam_engine_upload_scans_async(half B)   - copy stream; starts after the last roam_engine_fence()
//   roam_engine_step(scans of half A)        - main stream; first waits for the uploads of the slots it reads
//   roam_engine_fence()                      - uploads enqueued from now on wait for the steps enqueued so far
int32_t roam_engine_upload_scans_async(roam_ctx *ctx, int32_t pool_idx0, int32_t n, const uint8_t *host_records, int64_t host_stride)
{
    ENGINE();
    ARG_CHECK(ctx, host_records && n >= 1 && pool_idx0 >= 0 && pool_idx0 + n <= e->cfg.pool_scans && (host_stride == 0 || host_stride >= (int64_t)e->rec_bytes));
    // the copy kernel dereferences the records on the GPU: they must live in pinned (or registered) host memory - a pageable
    // buffer would fault on the device and abort the process, so it is refused here
    hipPointerAttribute_t at;
    const hipError_t pa = hipPointerGetAttributes(&at, host_records);
    if (pa != hipSuccess || (at.type != hipMemoryTypeHost && at.type != hipMemoryTypeManaged && at.type != hipMemoryTypeDevice)) {
        (void)hipGetLastError();
        ROAM_SET_ERR(ctx, "upload_scans_async: host_records is not pinned host memory (hipHostMalloc / hipHostRegister / roam_host_alloc)");
        return ROAM_E_ARG;
    }
    const uint8_t *dev_alias = at.devicePointer ? static_cast<const uint8_t *>(at.devicePointer) : host_records;
    // only the bytes the path reads cross PCIe: metadata + the clipped payload of every row (2 036 of 3 779 bytes for the
    // Oxford record at the 87.5 m clip).  A copy KERNEL on the copy stream reads the pinned host memory directly (it is
    // device-visible) with 16-byte loads - hipMemcpy2DAsync moves such rows one by one (270 scan pairs/s measured)
    const int width = e->cfg.payload_off + e->cfg.clip;
    hipLaunchKernelGGL(ingest_rows_kernel, dim3((e->cfg.rows + 3) / 4, n), dim3(256), 0, ctx->stream3, dev_alias, host_stride,
                       e->pool + (size_t)pool_idx0 * e->rec_bytes, (int64_t)e->rec_bytes, e->cfg.rows, e->cfg.stride, width);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev_up, ctx->stream3));
    e->up_seq++;
    for (int i = 0; i < n; i++) { e->slot_seq[(size_t)pool_idx0 + i] = e->up_seq; e->slot_writes[(size_t)pool_idx0 + i]++; }
    HIP_TRY(ctx, hipEventRecord(e->ev_up_ring[e->up_seq & 15], ctx->stream3));
    e->uploads_pending = true;
    return ROAM_OK;
}

int32_t roam_engine_fence(roam_ctx *ctx)
{
    ENGINE();
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fence, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream3, ctx->ev_fence, 0));
    return ROAM_OK;
}

int32_t roam_engine_copy_scan(roam_ctx *ctx, int32_t dst_idx, int32_t src_idx)
{
    ENGINE();
    ARG_CHECK(ctx, dst_idx >= 0 && dst_idx < e->cfg.pool_scans && src_idx >= 0 && src_idx < e->cfg.pool_scans);
    if (dst_idx != src_idx)
    {
        HIP_TRY(ctx, hipMemcpyAsync(e->pool + (size_t)dst_idx * e->rec_bytes, e->pool + (size_t)src_idx * e->rec_bytes,
                                    e->rec_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(e->ev_pool, ctx->stream));         // the front-end streams of the next step wait for it
        e->pool_dirty = true;
        e->ap_pool_dirty = true;
        e->slot_writes[(size_t)dst_idx]++;
    }
    return ROAM_OK;
}

int32_t roam_engine_set_motion_prior(roam_ctx *ctx, const float *affine, const uint8_t *use)
{
    ENGINE();
    if (!affine) { e->prior_set = false; return ROAM_OK; }
    const int B = e->B;
    for (int b = 0; b < B; b++)
        for (int i = 0; i < 6; i++) {
            const float lim = (i % 3 == 2) ? ROAM_KLT_MAX_GUESS : ROAM_PRIOR_MAX_LINEAR;
            if (!(fabsf(affine[6 * b + i]) <= lim)) {                   // (NaN fails it too)
                ROAM_SET_ERR(ctx, "set_motion_prior: lane %d, entry %d = %g: finite, linear part within %g, translation within %g px",
                             b, i, (double)affine[6 * b + i], (double)ROAM_PRIOR_MAX_LINEAR, (double)ROAM_KLT_MAX_GUESS);
                return ROAM_E_ARG;
            }
        }
    const int k4 = (int)(e->nstep & 3);
    // the slot's last upload was enqueued ahead of the tracker of step nstep - 4; roam_engine_step has waited for that step's end
    // since (it lets the host run three steps ahead), so this returns at once - it states the guard, as for scan_host
    if (e->nstep >= 4) HIP_TRY(ctx, hipEventSynchronize(e->ev_klt[k4]));
    uint8_t *slot = e->prior_host + (size_t)k4 * e->prior_bytes;
    memcpy(slot, affine, sizeof(float) * 6 * (size_t)B);
    if (use) for (int b = 0; b < B; b++) slot[24 * (size_t)B + b] = use[b] ? 1 : 0;
    else memset(slot + 24 * (size_t)B, 1, (size_t)B);
    e->prior_set = true;
    return ROAM_OK;
}

int32_t roam_engine_set_auto_prior(roam_ctx *ctx, const roam_auto_prior_cfg *cfg)
{
    if (!ctx) return ROAM_E_ARG;
    Engine *e = ctx->engine;
    if (!e) { ROAM_SET_ERR(ctx, "engine not created"); return ROAM_E_STATE; }
    FmtAutoCfg ac = {};
    FmtAutoPlan plan = {};
    if (cfg) {
        // what roam_engine_fmt_register refuses, before any device call
        const bool dflt = cfg->clip_px == 0 && cfg->downsample == 0 && cfg->cart_downsample == 0;
        const int clip_px = dflt ? 1012 : cfg->clip_px, ds = dflt ? 10 : cfg->downsample, cds = dflt ? 20 : cfg->cart_downsample;
        ARG_CHECK(ctx, ds >= 1 && cds >= 1 && e->cfg.rows >= 8);
        const int clip = (clip_px > 0 && clip_px < e->cfg.clip) ? clip_px : e->cfg.clip;
        ac.rows = e->cfg.rows; ac.cols = e->cfg.clip; ac.clip = clip; ac.R = clip / ds; ac.Rc = e->cfg.clip / cds; ac.lanes = e->B;
        ac.min_rot = cfg->min_rot_response; ac.min_trans = cfg->min_trans_response;
        ROAM_TRY(roam_fmt_auto_plan(ctx, ac, &plan));
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the one blocking part: the enqueued steps finish first (every stream a step uses)
    for (hipStream_t s : {ctx->stream, ctx->stream2, ctx->stream4, ctx->stream5}) HIP_TRY(ctx, hipStreamSynchronize(s));
    auto_prior_release(e);
    if (!cfg) return ROAM_OK;
    const size_t B = (size_t)e->B, rec_bytes = sizeof(FmtPriorRec) * B * RES_RING;
    hipError_t er = hipMalloc(reinterpret_cast<void **>(&e->ap_slab), plan.slab_bytes + rec_bytes);
    if (er == hipSuccess) er = hipMemsetAsync(e->ap_slab, 0, plan.slab_bytes + rec_bytes, ctx->stream);
    if (er == hipSuccess) er = hipHostMalloc(reinterpret_cast<void **>(&e->ap_rec_host), rec_bytes, hipHostMallocDefault);
    // a stream of its own: every stream of the context carries a stage of the step or the uploads
    if (er == hipSuccess) er = hipStreamCreateWithFlags(&e->ap_stream, hipStreamNonBlocking);
    if (er == hipSuccess) er = hipEventCreateWithFlags(&e->ap_ev, hipEventDisableTiming);
    int32_t rc = ROAM_OK;
    if (er != hipSuccess) {
        (void)hipGetLastError();
        ROAM_SET_ERR(ctx, "auto prior: %zu bytes of device memory for chunks of %zu pairs: %s", plan.slab_bytes + rec_bytes, plan.chunk, hipGetErrorString(er));
        rc = ROAM_E_HIP;
    } else {
        e->ap_rec = reinterpret_cast<FmtPriorRec *>(e->ap_slab + plan.slab_bytes);
        rc = roam_fmt_auto_init(ctx, ac, plan, e->ap_slab, &e->ap);          // (synchronises ctx->stream: the memset has landed)
    }
    if (rc != ROAM_OK) { auto_prior_release(e); return rc; }
    e->ap_plan = plan;
    e->ap_up_waited = 0;
    e->ap_pool_dirty = e->pool_dirty;
    return ROAM_OK;
}

int32_t roam_engine_step_prior(roam_ctx *ctx, int64_t step, double *out6, float *affine, uint8_t *source, int32_t n)
{
    ENGINE();
    ARG_CHECK(ctx, n >= 1 && n <= e->B);
    if (step < 0 || step >= e->nstep || step < e->nstep - RES_RING) {
        ROAM_SET_ERR(ctx, "step %lld is not in the result ring (steps %lld..%lld)", (long long)step,
                     (long long)std::max<int64_t>(0, e->nstep - RES_RING), (long long)e->nstep - 1);
        return ROAM_E_STATE;
    }
    const int rs = (int)(step % RES_RING);
    if (!e->ap || e->ap_rec_step[rs] != step) {
        ROAM_SET_ERR(ctx, "step %lld has no prior records: roam_engine_set_auto_prior was off when it was enqueued or has been since", (long long)step);
        return ROAM_E_STATE;
    }
    HIP_TRY(ctx, hipEventSynchronize(e->ev_res[rs]));      // that step's records only
    const FmtPriorRec *r = e->ap_rec_host + (size_t)rs * e->B;
    for (int i = 0; i < n; i++) {
        if (out6) {
            double *q = out6 + 6 * (size_t)i;
            q[0] = r[i].v[3]; q[1] = roam_fmt_scale(e->ap_plan.log_base, r[i].v[0]); q[2] = r[i].v[2];
            q[3] = r[i].v[4]; q[4] = r[i].v[5]; q[5] = r[i].v[6];
        }
        if (affine) memcpy(affine + 6 * (size_t)i, r[i].affine, sizeof(float) * 6);
        if (source) source[i] = r[i].source;
    }
    return ROAM_OK;
}

// ------------------------------------------------------------------------------ one step, part by part (in the order roam_engine_step calls them)
// what a step works out once, before it enqueues anything
struct Step {
    bool manual, ap_run;        // who seeds the tracker: the caller's prior (roam_engine_set_motion_prior) | else, in that mode, the in-step registration
    bool any_new;               // a lane starts a new sequence
    int rs, pb, k4, w4;         // ring slot of the result records | of the peak / scan-index buffers | event slot of this step | of step N-3
    int KM, ap_pairs;           // host-known bound of the feature counts (they only shrink between (re)seeds) | pairs the in-step prior registers
    roam_lane_result *res_slot;
    uint8_t *prev, *next;       // pyramids: the previous image | the one this step makes
    uint8_t *prior_slot;        // the step's slot of prior_dev: B x 6 f32 affine rows, then B use bytes
};

// the checks: arguments (the caller's indices are decoded here: e->new_seq now, e->last_scan once nothing can refuse the step for its
// slots), the auto prior's stale-slot refusal, the new-sequence precondition.  No runtime call
static int32_t step_check(roam_ctx *ctx, Engine *e, const int32_t *scan_idx, Step &s)
{
    ARG_CHECK(ctx, scan_idx);
    const int B = e->B;
    for (int b = 0; b < B; b++) {
        ARG_CHECK(ctx, scan_idx[b] >= 0 && (scan_idx[b] & ~ROAM_STEP_NEW_SEQUENCE) < e->cfg.pool_scans);
        e->new_seq[b] = (scan_idx[b] & ROAM_STEP_NEW_SEQUENCE) ? 1 : 0;
    }
    s.manual = e->prior_set;
    s.ap_run = e->ap && !e->prior_set;
    if (s.ap_run) {
        int bad = -1;
        for (int b = B - 1; b >= 0; b--) {
            const int ps = e->prev_scan[b];
            if (ps < 0 || e->new_seq[b] || e->lane_seen[b] == UINT64_MAX || e->slot_writes[(size_t)ps] == e->lane_seen[b]) continue;
            e->lane_seen[b] = UINT64_MAX;        // said once: the caller restores the record and steps again, and that step trusts the slot
            bad = b;
        }
        if (bad >= 0) {
            ROAM_SET_ERR(ctx, "auto prior: pool slot %d, the previous scan of lane %d, was written after the lane consumed it", e->prev_scan[bad], bad);
            return ROAM_E_STATE;
        }
    }
    s.any_new = false;
    for (int b = 0; b < B; b++) { e->last_scan[b] = scan_idx[b] & ~ROAM_STEP_NEW_SEQUENCE; s.any_new = s.any_new || e->new_seq[b]; }
    if (s.any_new && !(e->rt_on && e->rt_mode)) { ROAM_SET_ERR(ctx, "ROAM_STEP_NEW_SEQUENCE needs device-side detection (retrack_on_device, mode >= 1)"); return ROAM_E_STATE; }
    return ROAM_OK;
}

// `st` waits for asynchronous upload number `need` - the latest that wrote a pool slot the stream's next kernels read - unless it has
// waited for it or a later one before: *waited advances
static int32_t wait_upload(roam_ctx *ctx, Engine *e, hipStream_t st, uint64_t need, uint64_t *waited)
{
    if (need <= *waited) return ROAM_OK;
    if (e->up_seq - need < 16) HIP_TRY(ctx, hipStreamWaitEvent(st, e->ev_up_ring[need & 15], 0));
    else { HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_up, 0)); need = e->up_seq; }      // (its event has been reused: the newest covers it)
    *waited = need;
    return ROAM_OK;
}

// the in-step prior, first half: the pairs of this step, and what stage A waits for in step_indices, for the previous and the current slots
// alike, on the pass's stream
static int32_t auto_prior_pairs(roam_ctx *ctx, Engine *e, Step &s)
{
    const int B = e->B;
    e->ap_prev.resize((size_t)B); e->ap_curr.resize((size_t)B); e->ap_pair.resize((size_t)B);
    uint64_t need = 0;
    s.ap_pairs = 0;
    for (int b = 0; b < B; b++) {
        const int ps = e->prev_scan[b], cs = e->last_scan[b];
        e->ap_pair[b] = -1;
        if (ps < 0 || e->new_seq[b]) continue;
        e->ap_pair[b] = s.ap_pairs; e->ap_prev[s.ap_pairs] = ps; e->ap_curr[s.ap_pairs] = cs; s.ap_pairs++;
        need = std::max(need, std::max(e->slot_seq[(size_t)ps], e->slot_seq[(size_t)cs]));
    }
    ROAM_TRY(wait_upload(ctx, e, e->ap_stream, need, &e->ap_up_waited));
    if (e->ap_pool_dirty) { HIP_TRY(ctx, hipStreamWaitEvent(e->ap_stream, e->ev_pool, 0)); e->ap_pool_dirty = false; }
    return ROAM_OK;
}

// what stage A waits for before it reads the pool, then the step's scan indices and new-sequence flags on its stream
// (lane initialisation, retracks and synchronous uploads finish on the host before a step is enqueued)
static int32_t step_indices(roam_ctx *ctx, Engine *e, const Step &s)
{
    const int B = e->B;
    hipStream_t sA = ctx->stream2;
    if (e->uploads_pending) {
        uint64_t need = 0;
        for (int b = 0; b < B; b++) need = std::max(need, e->slot_seq[(size_t)e->last_scan[b]]);
        ROAM_TRY(wait_upload(ctx, e, sA, need, &e->up_waited));
        if (e->up_waited == e->up_seq) e->uploads_pending = false;
    }
    if (e->pool_dirty) { HIP_TRY(ctx, hipStreamWaitEvent(sA, e->ev_pool, 0)); e->pool_dirty = false; }   // device-to-device record copies
    int32_t *hs = e->scan_host + (size_t)s.pb * 2 * B;
    if (e->nstep >= 3) HIP_TRY(ctx, hipEventSynchronize(e->ev_g4[s.w4]));   // the staging slot's last copy has long been consumed
    for (int b = 0; b < B; b++) { hs[b] = e->last_scan[b]; hs[B + b] = e->new_seq[b]; }
    HIP_TRY(ctx, hipMemcpyAsync(e->scan_idx[s.pb], hs, sizeof(int32_t) * 2 * (size_t)B, hipMemcpyHostToDevice, sA));
    return ROAM_OK;
}

// the in-step prior, second half (every step of an engine in that mode, whoever seeds it): the pass and the step's prior records
static int32_t auto_prior_enqueue(roam_ctx *ctx, Engine *e, const Step &s)
{
    const int B = e->B;
    if (s.ap_run) {
        // The registration of this step: it reads raw pool records only, like stage A, and runs beside it.  Its index copy is its own
        // stream's first command; it writes the step's slot of prior_dev (last read by the tracker of four steps ago) and of the record
        // ring (whose copy of eight steps ago the host has waited for); its staging slot was consumed four steps ago (the wait
        // for g4 of step N - 3 in step_indices covers it).  The chunks of a pass, and the passes of consecutive steps, share buffers and run
        // in order on the one stream; the pass of step N + 1 may run while step N tracks
        FmtBatchIn in;
        in.pool = e->pool; in.rec_bytes = (int64_t)e->rec_bytes; in.rec_stride = e->cfg.stride; in.payload_off = e->cfg.payload_off;
        ROAM_TRY(roam_fmt_auto_enqueue(ctx, e->ap, e->ap_stream, in, s.k4, s.ap_pairs, e->ap_prev.data(), e->ap_curr.data(), e->ap_pair.data(),
                                       s.prior_slot, e->ap_rec + (size_t)s.rs * B));
        HIP_TRY(ctx, hipEventRecord(e->ap_ev, e->ap_stream));
    }
    e->ap_rec_step[s.rs] = e->nstep;
    if (s.manual) {                  // the caller's prior: no registration, the records say so (the ring slot is the host's: roam_engine_step waited)
        const uint8_t *hp = e->prior_host + (size_t)s.k4 * e->prior_bytes;
        FmtPriorRec *hr = e->ap_rec_host + (size_t)s.rs * B;
        for (int b = 0; b < B; b++) {
            for (double &v : hr[b].v) v = NAN;
            memcpy(hr[b].affine, hp + 24 * (size_t)b, 24);
            hr[b].source = hp[24 * (size_t)B + b] ? 2 : 0;
        }
    }
    return ROAM_OK;
}

// The front end.  Three-stage pipeline across steps:
//   stage A (stream2): warp (+ polar peaks on stream5) - depend only on the raw scan; issue-bound (VALU / LDS)
//   stage B (stream4): pyramid of the warped image - HBM-bound, little arithmetic
//   stage C (stream):  KLT ... LM, g4              - needs stage B of its own step and stage C of the previous one
// When steps are enqueued back to back, A(N+2), B(N+1) and C(N) run concurrently: the HBM-bound pyramid and the
// latency-bound LM solve fill the gaps of the issue-bound kernels.  Four pyramid buffers (previous / current /
// in stage B / in stage A) and three peak / scan-index buffers keep the stages apart:
//   A(N) waits for KLT(N-3)  - the pyramid it overwrites was that tracker's "previous" image
//   A(N) waits for g4(N-3)   - that kernel reads the peak counts / scan indices of the same ring slot
//   B(N) waits for A(N), KLT(N) waits for B(N)
// (the two waits of A: roam_engine_step; the scan indices are on stage A's stream: step_indices)
static int32_t step_front_end(roam_ctx *ctx, Engine *e, const Step &s)
{
    const int B = e->B, pb = s.pb;
    const roam_engine_cfg &c = e->cfg;
    hipStream_t sA = ctx->stream2, sB = ctx->stream4;
    hipEvent_t *tr = e->tr_ev[e->nstep & 63];
    if (e->stage_ev) {
        for (auto &ev : e->tr_ev[e->nstep & 63]) if (!ev && !new_event(ctx, e, &ev, hipEventDefault)) return ROAM_E_HIP;
        if (e->rt_on) for (auto &ev : e->rt_ev[e->nstep & 63]) if (!ev && !new_event(ctx, e, &ev, hipEventDefault)) return ROAM_E_HIP;
    }
    e->tr_ev_ok[e->nstep & 63] = e->stage_ev;       // (the switch may be flipped between steps: every step remembers what it recorded)
    if (e->stage_ev) e->stage_ev_step = e->nstep;
    // the peak kernel gets its own stream: it only needs the scan indices (event ev_idx) and is joined before g4
    hipStream_t sP = ctx->stream5;
    HIP_TRY(ctx, hipEventRecord(e->ev_idx, sA));
    HIP_TRY(ctx, hipStreamWaitEvent(sP, e->ev_idx, 0));
    // Batches (>= 256 lanes): the polar peaks (needed by this step's keyframe glue only) and the pyramid wait for the first bookkeeping
    // kernels of the previous step's detection.  Left alone the pyramid starts when its warp ends - beside the integral images of that
    // step, the one pairing on this path that is WORSE than running the two one after the other (integral 31 ms + pyramid 15.5 ms
    // in-step against 25 + 6.3 alone) - and, launched at the determinants' end itself, the 130 000 workgroups of the two kept whichever
    // bookkeeping kernel came first waiting ~3.8 ms for slots.  +2 % +2 % +0.8 % on the default workload (profiles/ROUNDS.md, round 6).
    // Not for a single sequence: it lives on the overlap of its front end with the previous pair's back end.
    if (e->ev_emit) HIP_TRY(ctx, hipStreamWaitEvent(sP, e->ev_emit, 0));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_PEAKS], sP));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev_pk0, sP));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(tr[0], sP));
    PeakSrc ps = {e->pool, (int64_t)e->rec_bytes, (int64_t)c.stride, c.payload_off, 1, e->scan_idx[pb]};
    HIP_TRY(ctx, launch_peaks(sP, ps, B, c.rows, c.clip, e->row_stage, e->stage_cap, e->row_count, e->peaks_out[pb], c.peaks_cap, e->peaks_n[pb]));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev_pk1, sP));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(tr[5], sP));
    HIP_TRY(ctx, hipEventRecord(e->ev_peaks, sP));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(tr[1], sA));
    HIP_TRY(ctx, launch_warp_gather(sA, e->warp_map, pool_warp_src(e, e->scan_idx[pb]), B, c.rows, c.clip, s.next, e->pd.lane_stride, e->warp_dark_zero));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(tr[2], sA));
    HIP_TRY(ctx, hipEventRecord(e->ev_warp, sA));                         // end of stage A
    HIP_TRY(ctx, hipStreamWaitEvent(sB, e->ev_warp, 0));
    if (e->ev_emit) HIP_TRY(ctx, hipStreamWaitEvent(sB, e->ev_emit, 0));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(tr[3], sB));
    HIP_TRY(ctx, launch_build_pyramid(sB, s.next, e->pd, B, e->pyr_dark));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(tr[4], sB));
    HIP_TRY(ctx, hipEventRecord(e->ev_join, sB));                         // end of stage B
    return ROAM_OK;
}

// the back end (stage C, on the compute stream behind stage B): KLT through g4, then the retrack, then the result copies
static int32_t step_back_end(roam_ctx *ctx, Engine *e, const Step &s)
{
    const int B = e->B, pb = s.pb, KM = s.KM;
    const roam_engine_cfg &c = e->cfg;
    const int nw = KS / 64;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipStreamWaitEvent(st, e->ev_join, 0));
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_KLT], st));
    if (s.any_new) {
        // lanes that start a NEW sequence on this scan drop their features: nothing is tracked, the pose stays, and the retrack
        // branch detects the sequence's first features on this scan (appendNewFeatures(prevImgCart, empty), RawROAMSystem.py:150)
        hipLaunchKernelGGL(new_sequence_kernel, dim3((B + 255) / 256), dim3(256), 0, st, e->feat_n, e->scan_idx[pb] + B, B);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (s.ap_run) HIP_TRY(ctx, hipStreamWaitEvent(st, e->ap_ev, 0));      // the affines of the in-step registration
    const bool seeded = s.manual || s.ap_run;
    HIP_TRY(ctx, launch_klt(st, s.prev, s.next, e->pd, e->feat, e->feat_n, KM, KS, B, e->klt_next, e->klt_status, e->klt_err, nullptr,
                            seeded ? reinterpret_cast<const float *>(s.prior_slot) : nullptr, seeded ? s.prior_slot + 24 * (size_t)B : nullptr));
    HIP_TRY(ctx, hipEventRecord(e->ev_klt[s.k4], st));
    hipLaunchKernelGGL(g1_good_kernel, dim3(B), dim3(256), 0, st, e->feat, e->feat_n, e->klt_next, e->klt_status, e->klt_err,
                       e->good_old, e->good_new, e->good_idx, e->good_n, KM);
    HIP_TRY(ctx, hipGetLastError());
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_GRAPH], st));
    if (c.reject_outliers) {
        HIP_TRY(ctx, launch_consistency_graph(st, e->good_old, e->good_new, e->good_n, KM, KS, B, 0.5 / M_PER_PX, e->adj, nw));
        if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_CLIQUE], st));
        HIP_TRY(ctx, launch_max_clique(st, e->adj, e->good_n, KM, KS, nw, B, c.clique_node_limit, e->cq_stack, e->cq_mask, e->cq_n, e->cq_flags, e->cq_order));
    } else {
        if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_CLIQUE], st));
        hipLaunchKernelGGL(fill_mask_kernel, dim3(B), dim3(256), 0, st, e->cq_mask, e->good_n, e->cq_n, e->cq_flags);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_KABSCH], st));
    hipLaunchKernelGGL(g2_inliers_kernel, dim3(B), dim3(256), 0, st, e->good_old, e->good_new, e->good_idx, e->good_n, e->cq_mask,
                       e->kf_pose, e->kf_und, e->kf_und_tmp, e->kab_src, e->kab_tgt, e->p_w, e->p_jt, e->feat, e->in_n, e->kab_out, e->pose,
                       c.motion_distortion ? e->T_wj0 : nullptr, e->T_init);                 // (T_wj0 / T_init feed the LM solve only)
    HIP_TRY(ctx, hipGetLastError());
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_LM], st));
    if (c.motion_distortion) {
        MdsProblemDesc P;
        P.T_wj0 = e->T_wj0; P.T_init = e->T_init; P.p_w = e->p_w; P.p_jt = e->p_jt; P.count = e->in_n;
        P.N = KM; P.nstride = KS; P.nmax = KM; P.B = B; P.period = 0.25;
        for (int i = 0; i < 5; i++) P.sigma5[i] = c.sigma5[i];
        P.big = e->lm_big; P.big_slot = e->lm_big_slot; e->lm_big_slot ^= 1;
        HIP_TRY(ctx, launch_mds_solve(st, P, e->lm_work, e->lm_out, e->lm_nfev, e->lm_info, nullptr, nullptr));
    }
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_GLUE], st));
    HIP_TRY(ctx, hipStreamWaitEvent(st, e->ev_peaks, 0));
    hipLaunchKernelGGL(g4_update_kernel, dim3(B), dim3(256), 0, st, c, e->lm_out, e->lm_nfev, e->lm_info, e->kab_out, e->pose,
                       e->vel, e->kf_pose, e->kf_und, e->kf_und_tmp, e->p_jt, e->in_n, e->good_n, e->feat_n, e->peaks_n[pb],
                       e->cq_flags, s.res_slot, e->scan_idx[pb], e->kf_vel, e->kf_scan, e->kf_fresh, e->kf_live, e->map_store, e->map_n,
                       e->map_cap, (e->rt_on && e->rt_mode) ? (e->rt_mode == 2 ? 2 : 1) : 0, e->rt.rt_lane, e->rt.rt_scan, e->rt.rt_n);
    HIP_TRY(ctx, hipGetLastError());
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_RETRACK], st));
    if (e->rt_on && e->rt_mode) {
        // lanes that ran out of features (flag bit 2; listed by g4_update_kernel's last block): appendNewFeatures on the current scan +
        // keyframe refresh, on the device
        e->rt.res = s.res_slot;
        if (B >= 256 && !e->ev_emit && !new_event(ctx, e, &e->ev_emit, hipEventDisableTiming)) return ROAM_E_HIP;
        if (e->det_side.chunk > 0 && !e->det_side.ev_i[0]) {
            e->det_side.st = ctx->stream4;
            for (int i = 0; i < 4; i++)
                if (!new_event(ctx, e, &e->det_side.ev_i[i], hipEventDisableTiming) || !new_event(ctx, e, &e->det_side.ev_d[i], hipEventDisableTiming)) return ROAM_E_HIP;
        }
        HIP_TRY(ctx, launch_retrack(st, e->rt, B, e->stage_ev ? e->rt_ev[e->nstep & 63] : nullptr, RT_TRACE_CHUNKS, e->ev_emit,
                                    e->det_side.chunk > 0 ? &e->det_side : nullptr));
        if (e->rt_mode == 2) e->rt_floor = std::min(KS, e->kmax() + 256);
    }
    e->rt_ev_ok[e->nstep & 63] = e->rt_on && e->rt_mode && e->stage_ev;
    if (e->stage_ev) HIP_TRY(ctx, hipEventRecord(e->ev[ST_COUNT], st));
    HIP_TRY(ctx, hipEventRecord(e->ev_g4[s.k4], st));
    // per-step result record -> pinned host ring: roam_engine_step_results(step) waits for THIS copy only
    // (on the compute stream itself: a side stream waiting on an event here cost 11 % of the step rate - the extra stream
    // shares a hardware queue with one of the pipeline's streams and serialises it; the 0.5 MB copy takes ~20 us)
    HIP_TRY(ctx, hipMemcpyAsync(e->results_host + (size_t)s.rs * B, s.res_slot, sizeof(roam_lane_result) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (s.ap_run) HIP_TRY(ctx, hipMemcpyAsync(e->ap_rec_host + (size_t)s.rs * B, e->ap_rec + (size_t)s.rs * B, sizeof(FmtPriorRec) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipEventRecord(e->ev_res[s.rs], st));
    return ROAM_OK;
}

// the ring bookkeeping: the step is enqueued, the lanes have consumed their scans
static void step_advance(Engine *e, const Step &s)
{
    for (int b = 0; b < e->B; b++) { e->prev_scan[b] = e->last_scan[b]; e->lane_seen[b] = e->slot_writes[(size_t)e->last_scan[b]]; }
    e->cur = (e->cur + 1) & 3;
    e->pk = s.pb;
    e->nstep++;
    e->stepped = true;
}

int32_t roam_engine_step(roam_ctx *ctx, const int32_t *scan_idx)
{
    ENGINE();
    Step s = {};
    ROAM_TRY(step_check(ctx, e, scan_idx, s));
    const int B = e->B;
    hipStream_t st = ctx->stream, sA = ctx->stream2;
    s.KM = e->kmax();
    s.rs = (int)(e->nstep % RES_RING);
    s.pb = (int)(e->nstep % 3);
    s.k4 = (int)(e->nstep & 3); s.w4 = (int)((e->nstep + 1) & 3);
    s.res_slot = e->results + (size_t)s.rs * B;
    s.prev = e->pyr[e->cur]; s.next = e->pyr[(e->cur + 1) & 3];
    s.prior_slot = e->prior_dev + (size_t)s.k4 * e->prior_bytes;
    if (e->kfx_calls) {
        // a keyframe exchange reads the previous step's keyframe state (the compute stream overwrites it: wait for the latest PACK) and the peak
        // list of ITS ring slot, which the peak stream overwrites three steps later: stream5 waits for the pack that read the slot it is about
        // to fill - not for the latest one, which would take the peak kernel out of the stage overlap
        HIP_TRY(ctx, hipStreamWaitEvent(st, e->ev_kfx[e->kfx_last], 0));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream5, e->ev_kfx[s.pb], 0));
    }
    if (e->nstep >= RES_RING) HIP_TRY(ctx, hipEventSynchronize(e->ev_res[s.rs]));   // the ring slot's previous copy (8 steps ago) has long landed
    // the motion prior of this step, if one was set: one small copy on the compute stream, behind the previous step's back end (which
    // no longer reads the slot: its tracker ran four steps ago) and long before this step's tracker is released by its pyramid
    if (s.manual) {
        HIP_TRY(ctx, hipMemcpyAsync(s.prior_slot, e->prior_host + (size_t)s.k4 * e->prior_bytes, 25 * (size_t)B, hipMemcpyHostToDevice, st));
        e->prior_set = false;
    }
    HIP_TRY(ctx, hipStreamWaitEvent(sA, e->ev_klt[s.w4], 0));
    HIP_TRY(ctx, hipStreamWaitEvent(sA, e->ev_g4[s.w4], 0));
    if (s.ap_run) ROAM_TRY(auto_prior_pairs(ctx, e, s));
    ROAM_TRY(step_indices(ctx, e, s));
    if (e->ap) ROAM_TRY(auto_prior_enqueue(ctx, e, s));
    else e->ap_rec_step[s.rs] = -1;
    ROAM_TRY(step_front_end(ctx, e, s));
    ROAM_TRY(step_back_end(ctx, e, s));
    step_advance(e, s);
    return ROAM_OK;
}

int32_t roam_engine_results(roam_ctx *ctx, roam_lane_result *out, int32_t n)
{
    ENGINE();
    ARG_CHECK(ctx, out && n >= 1 && n <= e->B);
    if (e->nstep == 0) { ROAM_SET_ERR(ctx, "no step enqueued"); return ROAM_E_STATE; }
    return roam_engine_step_results(ctx, e->nstep - 1, out, n);
}

int32_t roam_engine_step_results(roam_ctx *ctx, int64_t step, roam_lane_result *out, int32_t n)
{
    ENGINE();
    ARG_CHECK(ctx, out && n >= 1 && n <= e->B);
    if (step < 0 || step >= e->nstep || step < e->nstep - RES_RING) {
        ROAM_SET_ERR(ctx, "step %lld is not in the result ring (steps %lld..%lld)", (long long)step,
                     (long long)std::max<int64_t>(0, e->nstep - RES_RING), (long long)e->nstep - 1);
        return ROAM_E_STATE;
    }
    const int rs = (int)(step % RES_RING);
    HIP_TRY(ctx, hipEventSynchronize(e->ev_res[rs]));      // waits for that step's records only; later steps keep running
    memcpy(out, e->results_host + (size_t)rs * e->B, sizeof(roam_lane_result) * (size_t)n);
    if (e->rt_on && e->rt_floor > 320 && step == e->nstep - 1 && e->rt_mode != 2) {
        // a forced (mode 2) step inflated the launch width of every later KLT / graph launch; the records of the LATEST step say
        // what every lane really holds, and lanes only shrink (or re-detect to <= 60 + 256) from here on
        const roam_lane_result *r = e->results_host + (size_t)rs * e->B;
        int m = 320;
        for (int b = 0; b < e->B; b++) m = std::max(m, (int)((r[b].flags & 8) ? r[b].n_after_retrack : r[b].n_inliers));
        e->rt_floor = std::min(e->rt_floor, (m + 63) & ~63);
    }
    return ROAM_OK;
}

int32_t roam_engine_set_retrack(roam_ctx *ctx, int32_t mode)
{
    ENGINE();
    ARG_CHECK(ctx, mode >= 0 && mode <= 2);
    if (!e->rt_on) { ROAM_SET_ERR(ctx, "engine created without retrack_on_device"); return ROAM_E_STATE; }
    e->rt_mode = mode;
    return ROAM_OK;
}

int32_t roam_engine_steps_enqueued(roam_ctx *ctx, int64_t *nstep)
{
    ENGINE();
    ARG_CHECK(ctx, nstep);
    *nstep = e->nstep;
    return ROAM_OK;
}

}  // extern "C"
