// engine.h - what the translation units of the scan-pair engine share (engine.hip: the step, creation and teardown; engine_map.hip: the
// keyframe maps and their exchange; engine_lanes.hip: lane set-up and read-back; engine_measure.hip: timing and diagnostics); internal,
// the other units of the library see the forward declaration of roam_internal.h.  Overview: engine.hip.
#pragma once
#include "roam_internal.h"
#include "fmt.h"
#include "retrack.h"
#include <algorithm>

#define KS ROAM_MAX_FEATURES
#define CART_CENTER 1012.0
#define M_PER_PX 0.0864
#define N_RETRACK 60             // getFeatures.py:57 (import-time binding used by RawROAMSystem.py:7,251)
#define ROT_THR 0.2              // Mapping.py:13
#define ERR_THR 10.0f            // getTransformKLT.py:84
#define TWO_PI 6.283185307179586476925286766559

#define RES_RING 8
enum { ST_PEAKS = 0, ST_WARP, ST_PYR, ST_KLT, ST_GRAPH, ST_CLIQUE, ST_KABSCH, ST_LM, ST_GLUE, ST_RETRACK, ST_COUNT };

struct Engine {
    roam_engine_cfg cfg;
    int B = 0, W = 0, stage_cap = 0;
    PyrDesc pd;
    size_t rec_bytes = 0;
    uint8_t *pool = nullptr;
    uint8_t *pyr[4] = {nullptr, nullptr, nullptr, nullptr};   // ring: previous / current / in the pyramid stage / being warped
    uint32_t *warp_map = nullptr;       // W x W sampling map (geometry only)
    int cur = 0;                        // pyr[cur] = previous image pyramids
    uint16_t *row_stage = nullptr;
    int32_t *row_count = nullptr;
    int32_t *peaks_out[3] = {nullptr, nullptr, nullptr}, *peaks_n[3] = {nullptr, nullptr, nullptr};   // ring of 3 (stage A runs 2 steps ahead of g4)
    int32_t *scan_idx[3] = {nullptr, nullptr, nullptr};
    int32_t *scan_host = nullptr;       // pinned staging of the scan indices + new-sequence flags (3 x 2B)
    int pk = 0;                         // ring slot of the latest step (valid peak / scan-index buffers)
    // motion prior of the next step (roam_engine_set_motion_prior): per slot B x 6 f32 affine rows, then B use bytes.  Four slots, indexed
    // like ev_klt: the host slot is rewritten and the device slot overwritten only after the tracker of four steps ago
    uint8_t *prior_host = nullptr, *prior_dev = nullptr;
    size_t prior_bytes = 0;             // of one slot
    bool prior_set = false;             // prior_host's slot of the next step holds a prior that no step has consumed
    int64_t nstep = 0;
    // the prior as a mode (roam_engine_set_auto_prior): fmt.hip's in-step registration on ap_stream writes the step's slot of prior_dev and
    // one record per lane into ap_rec (ring of RES_RING x B, behind the pass's buffers in ap_slab), mirrored to pinned memory behind the step
    FmtAuto *ap = nullptr;
    FmtAutoPlan ap_plan = {};
    uint8_t *ap_slab = nullptr;
    FmtPriorRec *ap_rec = nullptr, *ap_rec_host = nullptr;
    int64_t ap_rec_step[RES_RING] = {-1, -1, -1, -1, -1, -1, -1, -1};      // the step whose prior records a ring slot holds
    hipStream_t ap_stream = nullptr;
    hipEvent_t ap_ev = nullptr;         // end of the latest pass (the tracker of its step waits for it)
    uint64_t ap_up_waited = 0;          // as up_waited, for ap_stream
    bool ap_pool_dirty = false;         // as pool_dirty, for ap_stream
    std::vector<int32_t> prev_scan;     // host: the scan each lane's previous pyramid was made from (init_lane*, every step), -1: none
    std::vector<uint64_t> slot_writes;  // host: writes to each pool slot so far (upload_scan, upload_scans_async, copy_scan)
    std::vector<uint64_t> lane_seen;    // host: slot_writes of prev_scan when the lane consumed it; UINT64_MAX: whatever it holds (after a refusal)
    std::vector<int32_t> ap_prev, ap_curr, ap_pair;
    float *feat = nullptr;              // B x KS x 2
    int32_t *feat_n = nullptr;
    float *klt_next = nullptr, *klt_err = nullptr;
    uint8_t *klt_status = nullptr;
    float *good_old = nullptr, *good_new = nullptr;
    int32_t *good_idx = nullptr, *good_n = nullptr;
    uint64_t *adj = nullptr, *cq_stack = nullptr;
    int32_t *cq_order = nullptr;     // B: the step's clique problems, largest first (launch_max_clique)
    uint8_t *cq_mask = nullptr;
    int32_t *cq_n = nullptr, *cq_flags = nullptr;
    double *kab_src = nullptr, *kab_tgt = nullptr, *kab_out = nullptr;
    int32_t *in_n = nullptr;
    double *kf_pose = nullptr, *kf_und = nullptr, *kf_und_tmp = nullptr;   // B x 3, B x KS x 2
    // f1: device-resident keyframe map (Mapping.Map.keyframes): the live keyframe's creation velocity / scan,
    // and a per-lane ring of frozen keyframes {pose, velocity, n, scan | n x 2 undistorted locals}
    double *kf_vel = nullptr;                                              // B x 3
    int32_t *kf_scan = nullptr, *kf_fresh = nullptr, *kf_live = nullptr;   // B
    double *map_store = nullptr;                                           // B x map_cap x MAP_SLOT
    int32_t *map_n = nullptr;                                              // B
    int map_cap = 0;
    std::vector<int32_t> last_scan;                                        // host: scan of each lane's latest step
    double *pose = nullptr, *vel = nullptr;                                // B x 3
    double *T_wj0 = nullptr, *T_init = nullptr, *p_w = nullptr, *p_jt = nullptr;
    double *lm_work = nullptr, *lm_out = nullptr;
    int32_t *lm_nfev = nullptr, *lm_info = nullptr;
    int32_t *lm_big = nullptr;           // MdsProblemDesc::big: the solves left to the workgroup form, two alternating lists
    int lm_big_slot = 0;
    roam_lane_result *results = nullptr;           // ring of RES_RING per-step records (RES_RING x B)
    roam_lane_result *results_host = nullptr;      // pinned mirror, filled asynchronously after every step
    hipEvent_t ev_res[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_pool = nullptr;
    bool pool_dirty = false;
    RtArgs rt;                                      // device-side retrack (retrack.hip)
    bool rt_on = false;
    int rt_mode = 1;                                // 0 = suspended, 1 = lanes that ran out of features, 2 = every lane (measurement)
    uint8_t *kfb = nullptr;                         // 8e: packed keyframe payload (RCCL broadcast buffer)
    // 8e consumer: the global map of Mapping.Map.addKeyframe on EVERY rank - a ring of received keyframe payloads in HBM
    uint8_t *rmap = nullptr;
    int rmap_cap = 0;
    int64_t rmap_n = 0;                             // keyframes received so far (slot = index % rmap_cap)
    int64_t rmap_n_bcast = 0;                       // ... of which through roam_bcast_keyframe (host-side appends; never mixed with the exchange)
    std::vector<int32_t> rmap_root;                 // sending rank of each slot
    // per-step keyframe exchange (roam_keyframe_exchange): fixed-size records, one all-gather per step on its own stream, the
    // received keyframes appended on the device - the host never waits
    uint8_t *kfx_send = nullptr, *kfx_recv = nullptr;
    size_t kfx_rec = 0;                             // bytes of one record
    int kfx_peaks = 0;                              // peaks carried per record
    int kfx_world = 0;                              // ranks the receive buffer was sized for
    int64_t *rmap_n_dev = nullptr;                  // keyframes appended by the exchange (device-side count)
    int32_t *rmap_root_dev = nullptr;               // their sending ranks, per slot
    int64_t kfx_calls = 0;
    bool kfx_ready = false;                         // every resource of the exchange exists (set last: a failed set-up is retried, never half used)
    hipStream_t st_comm = nullptr;
    hipEvent_t ev_kfx[3] = {};                      // the PACK kernel of the exchange that read peak-ring slot i (the streams that overwrite its inputs wait for it)
    int kfx_last = -1;                              // slot of the latest pack
    hipEvent_t ev[ST_COUNT + 1] = {};
    bool stage_ev_forced = false;                   // ... the environment said so
    bool stage_ev = true;                           // record them (roam_engine_stage_times); ROAM_STAGE_EVENTS=0: ten timestamp packets fewer in the back end's chain
    hipEvent_t ev_join = nullptr, ev_pk0 = nullptr, ev_pk1 = nullptr;            // end of the front end (the back end waits for it) + the peak kernel's timing pair
    hipEvent_t ev_klt[4] = {}, ev_g4[4] = {};                // back-end milestones stage A of step N+3 waits for
    hipEvent_t ev_warp = nullptr;                            // end of stage A (stage B waits for it)
    hipEvent_t ev_idx = nullptr, ev_peaks = nullptr;                   // scan indices uploaded / peak kernel done
    // per-step boundaries of the three front-end kernels (before peaks | peaks/warp | warp/pyramid | after pyramid),
    // kept for the last TRACE_RING steps so that a caller can average a kernel's launch time over a timed
    // region without synchronising inside it (roam_engine_kernel_avg)
    hipEvent_t tr_ev[64][6] = {};
    hipEvent_t rt_ev[64][3 * RT_TRACE_CHUNKS] = {};                    // every detection chunk of a step (the first RT_TRACE_CHUNKS): before | integral image | determinants
    bool rt_ev_ok[64] = {};
    hipEvent_t ev_emit = nullptr;                   // batches of >= 256 lanes: after the first bookkeeping kernels behind a step's determinants (made by the
                                                    // first step that detects; the peaks and the pyramid of every later step wait for it)
    RtSide det_side = {};                           // determinants of a chunk beside the next chunk's integral images (ROAM_DET_SIDE=chunk, 0: off)
    int det_chunk() const { return (det_side.chunk > 0 && retrack_sided(rt, B, &det_side)) ? det_side.chunk : rt.slots; }     // detections per launch of a detection kernel
    int64_t rt_image_px = 0;                        // pixels of the integral image that are written and read (the needed tiles of the phase list)
    bool tr_ev_ok[64] = {};                          // the step recorded its front-end event pairs (stage events were on when it was enqueued)
    int64_t stage_ev_step = -1;                     // the step whose ev[] (back-end stage events) are valid, -1: none
    unsigned long long *pyr_dark = nullptr;        // lanes of the 2024 -> 1012 pyramid kernel that see nothing but pixels beyond the maximum range
    static constexpr bool warp_dark_zero = true;   // the pyramids are zero-filled at creation and level 0 is written by the warp only:
                                                    // its tiles beyond the maximum range are never stored (0.6 ms of 11.4 per 4096 scans)
    bool stepped = false, uploads_pending = false;
    // asynchronous uploads are numbered; a step waits for the upload that last wrote one of ITS scans, not for the newest one - the
    // newest waits (roam_engine_fence) for the steps before it, and a front end that waited for it ran after the previous step's back end
    // instead of beside it (the single-sequence driver: ~170 us of every pair)
    uint64_t up_seq = 0, up_waited = 0;
    std::vector<uint64_t> slot_seq;
    hipEvent_t ev_up_ring[16] = {};
    std::vector<int> lane_k;            // host-side upper bound of each lane's feature count
    // device-side retracks (mode 1) grow a lane to at most 60 + 256 features without the host knowing which lane; a step in
    // mode 2 re-detects on EVERY lane, whatever it holds: the bound of every lane then grows by the 256 the append may add
    int rt_floor = 320;
    int kmax() const { int m = rt_on ? rt_floor : 64; for (int k : lane_k) m = k > m ? k : m; m = (m + 63) & ~63; return m > KS ? KS : m; }
    std::vector<void *> allocs;         // every device allocation (dalloc): freed by roam_engine_destroy
    std::vector<hipEvent_t *> events;   // every event above that exists (new_event): destroyed and nulled by roam_engine_destroy; ap_ev alone
                                        // goes with the in-step prior's resources, which may be released and made again (auto_prior_release)
    std::vector<int32_t> new_seq;       // host: the lane starts a new sequence on the step being enqueued (ROAM_STEP_NEW_SEQUENCE)
};

#define ENGINE()                                  \
    if (!ctx) return ROAM_E_ARG;                  \
    Engine *e = ctx->engine;                      \
    if (!e) { ROAM_SET_ERR(ctx, "engine not created"); return ROAM_E_STATE; } \
    HIP_TRY(ctx, hipSetDevice(ctx->device))
#define ROAM_TRY(call) do { const int32_t rc_ = (call); if (rc_ != ROAM_OK) return rc_; } while (0)      // as HIP_TRY, for the library's own codes

// the engine's device memory has one owner: zero-filled on the context stream, freed with the engine
template <typename T>
static bool dalloc(roam_ctx *ctx, Engine *e, T **p, size_t count)
{
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = 16;
    hipError_t err = hipMalloc(&q, bytes);
    if (err != hipSuccess) {
        ROAM_SET_ERR(ctx, "engine: hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
        return false;
    }
    hipMemsetAsync(q, 0, bytes, ctx->stream);
    e->allocs.push_back(q);
    *p = (T *)q;
    return true;
}

// ... and so have its events: *slot (a member of *e, null so far) is created with `flags` (hipEventDefault: timed) and destroyed with the engine
static bool new_event(roam_ctx *ctx, Engine *e, hipEvent_t *slot, unsigned flags)
{
    if (hipEventCreateWithFlags(slot, flags) != hipSuccess) { *slot = nullptr; ROAM_SET_ERR(ctx, "hipEventCreate failed"); return false; }
    e->events.push_back(slot);
    return true;
}

// the pool as the warp reads it: lane b of a launch takes record lane_index[b]
static WarpSrc pool_warp_src(Engine *e, const int32_t *lane_index)
{
    WarpSrc s = {e->pool, (int64_t)e->rec_bytes, (int64_t)e->cfg.stride, e->cfg.payload_off, 1, lane_index};
    return s;
}

// f1 keyframe map: one slot = 8-double header {pose[3], velocity[3], n, scan} + KS x 2 undistorted locals
#define MAP_SLOT (8 + 2 * KS)
// copy a keyframe that is about to be replaced into the lane's ring (whole block; returns through *ok)
__device__ __forceinline__ void map_freeze(double *__restrict__ map_store, int32_t *__restrict__ map_n, int map_cap, int b,
                                           const double *__restrict__ kfp, const double *__restrict__ kfv, int n,
                                           int scan, const double *__restrict__ locals)
{
    const int slot = map_n[b];
    if (slot >= map_cap) return;                          // ring full: the keyframe is dropped, count stays at cap
    double *d = map_store + ((size_t)b * map_cap + slot) * MAP_SLOT;
    for (int j = threadIdx.x; j < 2 * n; j += blockDim.x) d[8 + j] = locals[j];
    if (threadIdx.x == 0) {
        d[0] = kfp[0]; d[1] = kfp[1]; d[2] = kfp[2];
        d[3] = kfv[0]; d[4] = kfv[1]; d[5] = kfv[2];
        d[6] = (double)n; d[7] = (double)scan;
    }
}

// ---- host functions that cross a unit (kept out of the library's symbol table)
#define ENGINE_UNIT __attribute__((visibility("hidden")))
// engine_map.hip: the live keyframe of `lane` goes to the lane's map ring unless the latest step made it (map_freeze_kernel, on ctx->stream)
ENGINE_UNIT int32_t launch_map_freeze(roam_ctx *ctx, Engine *e, int lane);
// engine_measure.hip: the fused detection variant's tables and per-slot scratch, made on first use (creation under ROAM_FUSED_DETECT=1)
ENGINE_UNIT int32_t fused_tables(roam_ctx *ctx, Engine *e);
