// The engine's keyframe maps (the engine: engine.hip): the per-lane device map of Mapping.Map.keyframes (f1), the keyframe broadcast
// (8e) and the per-step keyframe exchange between ranks with the remote map it fills.
#include "engine.h"

// host-initiated keyframe replacement (roam_engine_set_features): freeze the live keyframe unless the step that
// has just run created it (then g4 already froze its predecessor and the caller is amending the new one)
__global__ __launch_bounds__(256) void map_freeze_kernel(double *__restrict__ map_store, int32_t *__restrict__ map_n, int map_cap,
                                                         int b, const double *__restrict__ kf_pose,
                                                         const double *__restrict__ kf_vel, const int32_t *__restrict__ feat_n,
                                                         const int32_t *__restrict__ kf_scan, const double *__restrict__ kf_und,
                                                         const int32_t *__restrict__ kf_live, const int32_t *__restrict__ kf_fresh)
{
    if (!kf_live[b] || kf_fresh[b]) return;
    const int slot = map_n[b];
    map_freeze(map_store, map_n, map_cap, b, kf_pose + 3 * b, kf_vel + 3 * b, feat_n[b], kf_scan[b], kf_und + (size_t)b * KS * 2);
    __syncthreads();
    if (threadIdx.x == 0 && slot < map_cap) map_n[b] = slot + 1;
}

// 8e: keyframe payload of one lane for the RCCL broadcast, packed on the device:
//   [0..63]   roam_keyframe_hdr (pose, velocity, n_features, n_peaks, scan, lane)
//   [64.. ]   KS x 2 f64 prunedUndistortedLocals
//   [64 + KS*16 ..]  peaks_cap x 2 i32 polar peaks of the lane's latest scan
#define KFB_HDR 64
#define KFB_LOCALS_OFF KFB_HDR
#define KFB_PEAKS_OFF (KFB_HDR + KS * 16)
__global__ __launch_bounds__(256) void kf_pack_kernel(uint8_t *__restrict__ buf, int lane, const double *__restrict__ kf_pose,
                                                      const double *__restrict__ kf_vel, const int32_t *__restrict__ feat_n,
                                                      const int32_t *__restrict__ kf_scan, const double *__restrict__ kf_und,
                                                      const int32_t *__restrict__ peaks_n, const int32_t *__restrict__ peaks,
                                                      int peaks_cap)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    int n = feat_n[lane], P = peaks_n[lane];
    if (n > KS) n = KS;
    if (P > peaks_cap) P = peaks_cap;
    if (t == 0) {
        roam_keyframe_hdr *h = reinterpret_cast<roam_keyframe_hdr *>(buf);
        for (int i = 0; i < 3; i++) { h->pose[i] = kf_pose[3 * lane + i]; h->velocity[i] = kf_vel[3 * lane + i]; }
        h->n_features = n; h->n_peaks = P; h->scan = kf_scan[lane]; h->lane = lane;
    }
    double *loc = reinterpret_cast<double *>(buf + KFB_LOCALS_OFF);
    const double *src = kf_und + (size_t)lane * KS * 2;
    for (int j = t; j < 2 * n; j += nt) loc[j] = src[j];
    int32_t *pk = reinterpret_cast<int32_t *>(buf + KFB_PEAKS_OFF);
    const int32_t *ps = peaks + (size_t)lane * peaks_cap * 2;
    for (int j = t; j < 2 * P; j += nt) pk[j] = ps[j];
}

// per-step exchange: this rank's record = the live keyframe of `lane` if the step just made it one (result flag bit 1), else an
// empty record (n_features = -1); peaks are capped at `pk_cap` (n_peaks says how many travelled)
__global__ __launch_bounds__(256) void kfx_pack_kernel(uint8_t *__restrict__ buf, int lane, const roam_lane_result *__restrict__ res,
                                                       const double *__restrict__ kf_pose, const double *__restrict__ kf_vel,
                                                       const int32_t *__restrict__ feat_n, const int32_t *__restrict__ kf_scan,
                                                       const double *__restrict__ kf_und, const int32_t *__restrict__ peaks_n,
                                                       const int32_t *__restrict__ peaks, int peaks_cap, int pk_cap)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    const bool valid = (res[lane].flags & 2) != 0;
    int n = feat_n[lane], P = peaks_n[lane];
    if (n > KS) n = KS;
    if (P > pk_cap) P = pk_cap;
    if (t == 0) {
        roam_keyframe_hdr *h = reinterpret_cast<roam_keyframe_hdr *>(buf);
        for (int i = 0; i < 3; i++) { h->pose[i] = kf_pose[3 * lane + i]; h->velocity[i] = kf_vel[3 * lane + i]; }
        h->n_features = valid ? n : -1; h->n_peaks = valid ? P : 0; h->scan = kf_scan[lane]; h->lane = lane;
    }
    if (!valid) return;
    double *loc = reinterpret_cast<double *>(buf + KFB_LOCALS_OFF);
    const double *src = kf_und + (size_t)lane * KS * 2;
    for (int j = t; j < 2 * n; j += nt) loc[j] = src[j];
    int32_t *pk = reinterpret_cast<int32_t *>(buf + KFB_PEAKS_OFF);
    const int32_t *ps = peaks + (size_t)lane * peaks_cap * 2;
    for (int j = t; j < 2 * P; j += nt) pk[j] = ps[j];
}

// Map.addKeyframe on this rank for every non-empty record of the gathered buffer, in rank order (one workgroup: the slot of
// record r depends on the valid records before it)
__global__ __launch_bounds__(256) void kfx_append_kernel(const uint8_t *__restrict__ recv, int world, size_t rec_bytes,
                                                         uint8_t *__restrict__ rmap, size_t slot_bytes, int cap,
                                                         int64_t *__restrict__ n_dev, int32_t *__restrict__ root_dev, int max_feat, int max_peaks)
{
    __shared__ int64_t base;
    if (threadIdx.x == 0) base = *n_dev;
    __syncthreads();
    int64_t cnt = base;
    for (int r = 0; r < world; r++) {
        const uint8_t *src = recv + (size_t)r * rec_bytes;
        const roam_keyframe_hdr *h = reinterpret_cast<const roam_keyframe_hdr *>(src);
        const int n = h->n_features, P = h->n_peaks;
        if (n < 0) continue;                                                 // the rank made no keyframe in this step
        if (n > max_feat || P < 0 || P > max_peaks) continue;               // (a record no pack kernel writes: never copied past a slot)
        uint8_t *dst = rmap + (size_t)(cnt % cap) * slot_bytes;
        const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src);
        uint32_t *d4 = reinterpret_cast<uint32_t *>(dst);
        const size_t w_hdr = (KFB_HDR + (size_t)n * 16) / 4, w_pk0 = KFB_PEAKS_OFF / 4, w_pk = (size_t)P * 2;
        for (size_t j = threadIdx.x; j < w_hdr; j += blockDim.x) d4[j] = s4[j];
        for (size_t j = threadIdx.x; j < w_pk; j += blockDim.x) d4[w_pk0 + j] = s4[w_pk0 + j];
        if (threadIdx.x == 0) root_dev[cnt % cap] = r;
        cnt++;
    }
    __syncthreads();
    if (threadIdx.x == 0) *n_dev = cnt;
}

int32_t launch_map_freeze(roam_ctx *ctx, Engine *e, int lane)
{
    hipLaunchKernelGGL(map_freeze_kernel, dim3(1), dim3(256), 0, ctx->stream, e->map_store, e->map_n, e->map_cap, lane,
                       e->kf_pose, e->kf_vel, e->feat_n, e->kf_scan, e->kf_und, e->kf_live, e->kf_fresh);
    HIP_TRY(ctx, hipGetLastError());
    return ROAM_OK;
}

extern "C" {

int32_t roam_engine_map_reserve(roam_ctx *ctx, int32_t keyframes_per_lane)
{
    ENGINE();
    ARG_CHECK(ctx, keyframes_per_lane > 0 && keyframes_per_lane <= 4096);
    if (e->map_cap > 0) { ROAM_SET_ERR(ctx, "engine: the keyframe map is already reserved (%d per lane)", e->map_cap); return ROAM_E_STATE; }
    if (!dalloc(ctx, e, &e->map_store, (size_t)e->B * keyframes_per_lane * MAP_SLOT)) return ROAM_E_HIP;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    e->map_cap = keyframes_per_lane;
    return ROAM_OK;
}

int32_t roam_engine_map_count(roam_ctx *ctx, int32_t lane, int32_t *count)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B && count);
    int32_t v[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&v[0], e->map_n + lane, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&v[1], e->kf_live + lane, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *count = v[0] + (v[1] ? 1 : 0);                 // frozen keyframes + the live one
    return ROAM_OK;
}

int32_t roam_engine_map_get(roam_ctx *ctx, int32_t lane, int32_t index, double *pose3, double *vel3, double *locals_xy,
                            int32_t cap_pts, int32_t *n_out, int32_t *scan_out)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B && index >= 0 && pose3 && vel3 && n_out && scan_out && cap_pts >= 0 && (cap_pts == 0 || locals_xy));
    int32_t v[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&v[0], e->map_n + lane, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&v[1], e->kf_live + lane, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int frozen = v[0];
    if (index < frozen) {
        const double *src = e->map_store + ((size_t)lane * e->map_cap + index) * MAP_SLOT;
        double hdr[8];
        HIP_TRY(ctx, hipMemcpyAsync(hdr, src, sizeof(hdr), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const int n = (int)hdr[6];
        for (int i = 0; i < 3; i++) { pose3[i] = hdr[i]; vel3[i] = hdr[3 + i]; }
        *n_out = n; *scan_out = (int32_t)hdr[7];
        if (n > cap_pts) { ROAM_SET_ERR(ctx, "map_get: keyframe has %d points, capacity %d", n, cap_pts); return ROAM_E_CAPACITY; }
        if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(locals_xy, src + 8, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    } else if (index == frozen && v[1]) {           // the live keyframe
        int32_t n = 0, sc = -1;
        HIP_TRY(ctx, hipMemcpyAsync(pose3, e->kf_pose + 3 * (size_t)lane, sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(vel3, e->kf_vel + 3 * (size_t)lane, sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&n, e->feat_n + lane, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&sc, e->kf_scan + lane, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        *n_out = n; *scan_out = sc;
        if (n > cap_pts) { ROAM_SET_ERR(ctx, "map_get: keyframe has %d points, capacity %d", n, cap_pts); return ROAM_E_CAPACITY; }
        if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(locals_xy, e->kf_und + (size_t)lane * KS * 2, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        ROAM_SET_ERR(ctx, "map_get: lane %d holds %d keyframes, index %d", lane, frozen + (v[1] ? 1 : 0), index);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

int32_t roam_bcast_keyframe(roam_ctx *ctx, int32_t root, int32_t lane, roam_keyframe_hdr *hdr_out, double *locals_xy,
                            int32_t cap_pts, int32_t *peaks, int64_t peaks_cap)
{
    ENGINE();
    // (every rank validates the lane BEFORE the collective: a root that bailed out alone would leave the others in ncclBroadcast)
    ARG_CHECK(ctx, hdr_out && lane >= 0 && lane < e->B && cap_pts >= 0 && peaks_cap >= 0);
    static_assert(sizeof(roam_keyframe_hdr) == KFB_HDR, "header layout");
    const size_t total = KFB_PEAKS_OFF + (size_t)e->cfg.peaks_cap * 8;
    if (!e->kfb && !dalloc(ctx, e, &e->kfb, total)) return ROAM_E_HIP;
    hipStream_t st = ctx->stream;
    if (roam_comm_rank(ctx) == root) {
        hipLaunchKernelGGL(kf_pack_kernel, dim3(16), dim3(256), 0, st, e->kfb, lane, e->kf_pose, e->kf_vel, e->feat_n, e->kf_scan,
                           e->kf_und, e->peaks_n[e->pk], e->peaks_out[e->pk], e->cfg.peaks_cap);
        HIP_TRY(ctx, hipGetLastError());
    }
    // header + features (fixed 16.4 KB), then the peak list sized by the header: two latency-bound broadcasts
    int32_t rc = roam_comm_bcast_bytes(ctx, e->kfb, KFB_PEAKS_OFF, root);
    if (rc != ROAM_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(hdr_out, e->kfb, sizeof(roam_keyframe_hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const int n = hdr_out->n_features, P = hdr_out->n_peaks;
    if (n < 0 || n > KS || P < 0 || P > e->cfg.peaks_cap) { ROAM_SET_ERR(ctx, "bcast_keyframe: corrupt header (n=%d, P=%d)", n, P); return ROAM_E_STATE; }
    if (P > 0) {
        rc = roam_comm_bcast_bytes(ctx, e->kfb + KFB_PEAKS_OFF, (size_t)P * 8, root);
        if (rc != ROAM_OK) return rc;
    }
    if (e->rmap_cap > 0) {
        // (refused BEFORE anything is written: the exchange owns the ring slots and their count once it has run)
        if (e->kfx_calls) { ROAM_SET_ERR(ctx, "remote map: roam_bcast_keyframe and roam_keyframe_exchange were mixed on one engine"); return ROAM_E_STATE; }
        // Map.addKeyframe on this rank: the payload stays in HBM (device-to-device), header + features, then the peaks
        const size_t slot_bytes = KFB_PEAKS_OFF + (size_t)e->cfg.peaks_cap * 8;
        uint8_t *dst = e->rmap + (size_t)(e->rmap_n % e->rmap_cap) * slot_bytes;
        HIP_TRY(ctx, hipMemcpyAsync(dst, e->kfb, KFB_HDR + sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToDevice, st));
        if (P > 0) HIP_TRY(ctx, hipMemcpyAsync(dst + KFB_PEAKS_OFF, e->kfb + KFB_PEAKS_OFF, (size_t)P * 8, hipMemcpyDeviceToDevice, st));
        e->rmap_root[e->rmap_n % e->rmap_cap] = root;
        e->rmap_n++;
        e->rmap_n_bcast++;
    }
    if (locals_xy) {
        if (n > cap_pts) { ROAM_SET_ERR(ctx, "bcast_keyframe: %d features, capacity %d", n, cap_pts); return ROAM_E_CAPACITY; }
        if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(locals_xy, e->kfb + KFB_LOCALS_OFF, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    if (peaks) {
        if (P > peaks_cap) { ROAM_SET_ERR(ctx, "bcast_keyframe: %d peaks, capacity %lld", P, (long long)peaks_cap); return ROAM_E_CAPACITY; }
        if (P > 0) HIP_TRY(ctx, hipMemcpyAsync(peaks, e->kfb + KFB_PEAKS_OFF, sizeof(int32_t) * 2 * (size_t)P, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return ROAM_OK;
}

// the exchange's resources, made once for `world` ranks (a failed set-up is retried, never half used)
static int32_t kfx_setup(roam_ctx *ctx, Engine *e, int world)
{
    if (e->kfx_ready) {
        if (world > e->kfx_world) { ROAM_SET_ERR(ctx, "keyframe exchange: set up for %d ranks, asked for %d", e->kfx_world, world); return ROAM_E_STATE; }
        return ROAM_OK;
    }
    e->kfx_peaks = std::min(e->cfg.peaks_cap, 32768);
    e->kfx_rec = KFB_PEAKS_OFF + (size_t)e->kfx_peaks * 8;
    if (!e->st_comm) HIP_TRY(ctx, hipStreamCreateWithFlags(&e->st_comm, hipStreamNonBlocking));
    for (auto &ev : e->ev_kfx) if (!ev && !new_event(ctx, e, &ev, hipEventDisableTiming)) return ROAM_E_HIP;
    if (!e->kfx_send && !dalloc(ctx, e, &e->kfx_send, e->kfx_rec)) return ROAM_E_HIP;
    if (!e->kfx_recv && !dalloc(ctx, e, &e->kfx_recv, e->kfx_rec * (size_t)world)) return ROAM_E_HIP;
    if (!e->rmap_n_dev && !dalloc(ctx, e, &e->rmap_n_dev, 1)) return ROAM_E_HIP;
    if (!e->rmap_root_dev && !dalloc(ctx, e, &e->rmap_root_dev, (size_t)e->rmap_cap)) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemsetAsync(e->rmap_n_dev, 0, sizeof(int64_t), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    e->kfx_world = world;
    e->kfx_ready = true;
    return ROAM_OK;
}

// test / debug: the RECEIVE half of roam_keyframe_exchange on one GPU.  `recv` (host) holds `world` records as the ncclAllGather of a
// `world`-rank job leaves them in every rank's receive buffer - record r = rank r's, *rec_bytes apart (header at 0, locals at
// *locals_off, peaks at *peaks_off) - and goes through the SAME kfx_append_kernel, on the exchange stream, into this rank's remote map.
// With recv == NULL only the layout is returned.  No communicator is needed; the map must be reserved with at least `world` slots.
int32_t roam_debug_keyframe_append(roam_ctx *ctx, const uint8_t *recv, int32_t world, int64_t *rec_bytes, int32_t *locals_off,
                                   int32_t *peaks_off, int32_t *max_peaks)
{
    ENGINE();
    ARG_CHECK(ctx, world >= 1 && world <= 4096);
    if (e->rmap_cap <= 0) { ROAM_SET_ERR(ctx, "debug_keyframe_append: reserve the remote map first"); return ROAM_E_STATE; }
    if (e->rmap_cap < world) { ROAM_SET_ERR(ctx, "debug_keyframe_append: remote map of %d slots for %d ranks", e->rmap_cap, world); return ROAM_E_CAPACITY; }
    if (e->rmap_n_bcast) { ROAM_SET_ERR(ctx, "remote map: roam_bcast_keyframe and roam_keyframe_exchange were mixed on one engine"); return ROAM_E_STATE; }
    ROAM_TRY(kfx_setup(ctx, e, world));
    if (rec_bytes) *rec_bytes = (int64_t)e->kfx_rec;
    if (locals_off) *locals_off = KFB_LOCALS_OFF;
    if (peaks_off) *peaks_off = KFB_PEAKS_OFF;
    if (max_peaks) *max_peaks = e->kfx_peaks;
    if (!recv) return ROAM_OK;
    hipStream_t st = e->st_comm;
    HIP_TRY(ctx, hipMemcpyAsync(e->kfx_recv, recv, e->kfx_rec * (size_t)world, hipMemcpyHostToDevice, st));
    const size_t slot_bytes = KFB_PEAKS_OFF + (size_t)e->cfg.peaks_cap * 8;
    hipLaunchKernelGGL(kfx_append_kernel, dim3(1), dim3(256), 0, st, e->kfx_recv, world, e->kfx_rec, e->rmap, slot_bytes, e->rmap_cap,
                       e->rmap_n_dev, e->rmap_root_dev, KS, e->kfx_peaks);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));                            // (the host buffer is the caller's again)
    e->kfx_calls++;
    return ROAM_OK;
}

// collective, NON-BLOCKING: every rank calls it once after each roam_engine_step with its own lane.  The rank's record (the lane's
// new keyframe if the step made one, else empty) is packed on the device, one ncclAllGather of the fixed-size records runs on the
// exchange stream behind the step's last kernel, and every non-empty record is appended to this rank's remote map on the device.
// No host synchronisation: the step pipeline keeps running; roam_remote_map_count / _get wait for the exchange stream.
int32_t roam_keyframe_exchange(roam_ctx *ctx, int32_t lane)
{
    ENGINE();
    ARG_CHECK(ctx, lane >= 0 && lane < e->B);
    if (!ctx->comm) { ROAM_SET_ERR(ctx, "keyframe_exchange: communicator not initialised"); return ROAM_E_STATE; }
    if (e->rmap_cap <= 0) { ROAM_SET_ERR(ctx, "keyframe_exchange: reserve the remote map first"); return ROAM_E_STATE; }
    if (e->nstep == 0) { ROAM_SET_ERR(ctx, "keyframe_exchange: no step enqueued"); return ROAM_E_STATE; }
    const int world = roam_comm_world(ctx);
    // (the append kernel writes the records of one gather into consecutive ring slots: fewer slots than ranks would tear them)
    if (e->rmap_cap < world) { ROAM_SET_ERR(ctx, "keyframe_exchange: remote map of %d slots for %d ranks", e->rmap_cap, world); return ROAM_E_CAPACITY; }
    if (e->rmap_n_bcast) { ROAM_SET_ERR(ctx, "remote map: roam_bcast_keyframe and roam_keyframe_exchange were mixed on one engine"); return ROAM_E_STATE; }
    ROAM_TRY(kfx_setup(ctx, e, world));
    hipStream_t st = e->st_comm;
    const int rs = (int)((e->nstep - 1) % RES_RING);
    HIP_TRY(ctx, hipStreamWaitEvent(st, e->ev_res[rs], 0));            // the step's records (and with them its keyframe state) are final
    hipLaunchKernelGGL(kfx_pack_kernel, dim3(16), dim3(256), 0, st, e->kfx_send, lane, e->results + (size_t)rs * e->B, e->kf_pose, e->kf_vel,
                       e->feat_n, e->kf_scan, e->kf_und, e->peaks_n[e->pk], e->peaks_out[e->pk], e->cfg.peaks_cap, e->kfx_peaks);
    HIP_TRY(ctx, hipGetLastError());
    // the following steps overwrite what the pack kernel reads (keyframe state: the compute stream; the peak list of this ring slot:
    // the peak stream, three steps on): their streams wait for the PACK, not for the collective
    HIP_TRY(ctx, hipEventRecord(e->ev_kfx[e->pk], st));
    e->kfx_last = e->pk;
    int32_t rc = roam_comm_allgather_bytes(ctx, e->kfx_send, e->kfx_recv, e->kfx_rec, st);
    if (rc != ROAM_OK) return rc;
    const size_t slot_bytes = KFB_PEAKS_OFF + (size_t)e->cfg.peaks_cap * 8;
    hipLaunchKernelGGL(kfx_append_kernel, dim3(1), dim3(256), 0, st, e->kfx_recv, world, e->kfx_rec, e->rmap, slot_bytes, e->rmap_cap,
                       e->rmap_n_dev, e->rmap_root_dev, KS, e->kfx_peaks);
    HIP_TRY(ctx, hipGetLastError());
    e->kfx_calls++;
    return ROAM_OK;
}

// the exchange stream has drained: pull the device-side count and senders over to the host's bookkeeping
static int32_t kfx_settle(roam_ctx *ctx, Engine *e)
{
    if (!e->kfx_ready) return ROAM_OK;
    HIP_TRY(ctx, hipStreamSynchronize(e->st_comm));
    int64_t n = 0;
    HIP_TRY(ctx, hipMemcpy(&n, e->rmap_n_dev, sizeof(n), hipMemcpyDeviceToHost));
    // (the map may be polled while the loop runs: the device-side count only grows; the two producers refuse each other at call time)
    if (n > 0) {
        e->rmap_n = n;
        HIP_TRY(ctx, hipMemcpy(e->rmap_root.data(), e->rmap_root_dev, sizeof(int32_t) * (size_t)e->rmap_cap, hipMemcpyDeviceToHost));
    }
    return ROAM_OK;
}

int32_t roam_remote_map_reserve(roam_ctx *ctx, int32_t keyframes)
{
    ENGINE();
    ARG_CHECK(ctx, keyframes > 0 && keyframes <= 65536);
    if (e->rmap_cap > 0) { ROAM_SET_ERR(ctx, "engine: the remote map is already reserved (%d keyframes)", e->rmap_cap); return ROAM_E_STATE; }
    const size_t slot_bytes = KFB_PEAKS_OFF + (size_t)e->cfg.peaks_cap * 8;
    if (!dalloc(ctx, e, &e->rmap, slot_bytes * (size_t)keyframes)) return ROAM_E_HIP;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    e->rmap_root.assign((size_t)keyframes, -1);
    e->rmap_cap = keyframes;
    return ROAM_OK;
}

int32_t roam_remote_map_count(roam_ctx *ctx, int64_t *received, int32_t *resident)
{
    ENGINE();
    ARG_CHECK(ctx, received && resident);
    ROAM_TRY(kfx_settle(ctx, e));
    *received = e->rmap_n;
    *resident = (int32_t)std::min<int64_t>(e->rmap_n, e->rmap_cap);
    return ROAM_OK;
}

int32_t roam_remote_map_get(roam_ctx *ctx, int32_t index, roam_keyframe_hdr *hdr_out, int32_t *root_out, double *locals_xy,
                            int32_t cap_pts, int32_t *peaks, int64_t peaks_cap)
{
    ENGINE();
    ROAM_TRY(kfx_settle(ctx, e));
    const int resident = (int)std::min<int64_t>(e->rmap_n, e->rmap_cap);
    ARG_CHECK(ctx, hdr_out && index >= 0 && index < resident && cap_pts >= 0 && peaks_cap >= 0);
    // index 0 = the oldest keyframe still resident
    const int64_t abs_i = e->rmap_n - resident + index;
    const size_t slot_bytes = KFB_PEAKS_OFF + (size_t)e->cfg.peaks_cap * 8;
    const uint8_t *src = e->rmap + (size_t)(abs_i % e->rmap_cap) * slot_bytes;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(hdr_out, src, sizeof(roam_keyframe_hdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (root_out) *root_out = e->rmap_root[abs_i % e->rmap_cap];
    const int n = hdr_out->n_features, P = hdr_out->n_peaks;
    if (locals_xy) {
        if (n > cap_pts) { ROAM_SET_ERR(ctx, "remote_map_get: %d features, capacity %d", n, cap_pts); return ROAM_E_CAPACITY; }
        if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(locals_xy, src + KFB_LOCALS_OFF, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    if (peaks) {
        if (P > peaks_cap) { ROAM_SET_ERR(ctx, "remote_map_get: %d peaks, capacity %lld", P, (long long)peaks_cap); return ROAM_E_CAPACITY; }
        if (P > 0) HIP_TRY(ctx, hipMemcpyAsync(peaks, src + KFB_PEAKS_OFF, sizeof(int32_t) * 2 * (size_t)P, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return ROAM_OK;
}

}  // extern "C"
