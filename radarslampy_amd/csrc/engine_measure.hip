// The engine's measurement and diagnostics surface (the engine: engine.hip): the stage and kernel timings a step records into its event
// rings, re-launches of single kernels for the roofline, and the detection kernels' candidate lists for the parity tests.
#include "engine.h"

static const char *kStageNames[ST_COUNT] = {"ingest_peaks", "warp_quantise", "pyramid", "klt", "consistency_graph",
                                            "max_clique", "kabsch", "mds_lm", "glue", "retrack"};

// the kernels a caller may name: the three of the front end by their stage's name (= their ST_ index), then the detection's image-scale
// kernels; "doh_fused[:<d>]": the fused variant [with diagnostics word d - ablations of retrack_fused.inc, measurement only]
enum { KN_INTEGRAL = ST_PYR + 1, KN_DET, KN_FUSED, KN_UNKNOWN };
static int kernel_of(const char *name)
{
    for (int i = 0; i <= ST_PYR; i++) if (!strcmp(name, kStageNames[i])) return i;
    if (!strcmp(name, "doh_integral")) return KN_INTEGRAL;
    if (!strcmp(name, "doh_det_maxima")) return KN_DET;
    return strncmp(name, "doh_fused", 9) ? KN_UNKNOWN : KN_FUSED;
}

// the detection kernels outside a step: scratch slot i works on the scan lane i % lanes saw last, P slots
static int32_t detect_slots(roam_ctx *ctx, Engine *e, int P)
{
    std::vector<int32_t> sc(P);
    for (int i = 0; i < P; i++) sc[i] = e->last_scan[i % e->B] >= 0 ? e->last_scan[i % e->B] : 0;
    HIP_TRY(ctx, hipMemcpy(e->rt.rt_scan, sc.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(e->rt.rt_n, &P, sizeof(int32_t), hipMemcpyHostToDevice));
    return ROAM_OK;
}

// the fused detection variant's tables and per-slot scratch, made when first needed (dead weight otherwise)
int32_t fused_tables(roam_ctx *ctx, Engine *e)
{
    RtArgs &r = e->rt;
    if (r.fd_mapT) return ROAM_OK;
    const size_t npx = (size_t)e->W * e->W, R = (size_t)r.slots;
    uint32_t *mapT = nullptr, *boxtab = nullptr, *darktab = nullptr;
    bool ok = dalloc(ctx, e, &mapT, npx) && dalloc(ctx, e, &boxtab, retrack_fused_boxtab_words(e->W)) && dalloc(ctx, e, &darktab, retrack_darktab_words(e->W));
    ok = ok && dalloc(ctx, e, &r.fd_halo, R * 2 * (size_t)r.fd_halo_words) && dalloc(ctx, e, &r.fd_cc, R * 2048);
    if (!ok) return ROAM_E_HIP;
    HIP_TRY(ctx, launch_retrack_fused_tables(ctx->stream, e->warp_map, e->W, e->cfg.clip, mapT, boxtab, darktab));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    r.fd_boxtab = boxtab; r.fd_darktab = darktab;
    r.fd_mapT = mapT;                                   // (set last: the null check of launch_retrack_part is the "ready" test)
    return ROAM_OK;
}

extern "C" {

int32_t roam_engine_set_stage_events(roam_ctx *ctx, int32_t on)
{
    ENGINE();
    if (!e->stage_ev_forced) e->stage_ev = on != 0;
    return ROAM_OK;
}

int32_t roam_engine_stage_times(roam_ctx *ctx, float *ms_out, const char **names_out, int32_t cap, int32_t *n)
{
    ENGINE();
    ARG_CHECK(ctx, ms_out && n && cap >= ST_COUNT);
    if (!e->stepped) { ROAM_SET_ERR(ctx, "no step recorded"); return ROAM_E_STATE; }
    if (!e->stage_ev) { ROAM_SET_ERR(ctx, "stage events are off (roam_engine_set_stage_events)"); return ROAM_E_STATE; }
    if (e->stage_ev_step != e->nstep - 1) { ROAM_SET_ERR(ctx, "the last step was enqueued with stage events off: run a step first"); return ROAM_E_STATE; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < ST_COUNT; i++) {
        float ms = 0;
        hipEvent_t *tl = e->tr_ev[(e->nstep - 1) & 63];                                     // stage A / B boundaries of the last step
        if (i == ST_PEAKS) HIP_TRY(ctx, hipEventElapsedTime(&ms, tl[0], tl[5]));
        else if (i == ST_WARP) HIP_TRY(ctx, hipEventElapsedTime(&ms, tl[1], tl[2]));
        else if (i == ST_PYR) HIP_TRY(ctx, hipEventElapsedTime(&ms, tl[3], tl[4]));
        else HIP_TRY(ctx, hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]));
        ms_out[i] = ms;
        if (names_out) names_out[i] = kStageNames[i];
    }
    *n = ST_COUNT;
    return ROAM_OK;
}

// average launch time of one front-end kernel over the last `last_steps` steps (at most 64), from the event
// pairs recorded on the stream the kernel ran on - the live, in-step duration (other kernels may share the GPU)
int32_t roam_engine_kernel_avg(roam_ctx *ctx, const char *name, int32_t last_steps, float *avg_ms, int32_t *n_used)
{
    ENGINE();
    ARG_CHECK(ctx, name && last_steps >= 1 && avg_ms && n_used);
    if (!e->stage_ev) { ROAM_SET_ERR(ctx, "stage events are off (roam_engine_set_stage_events)"); return ROAM_E_STATE; }
    const int k = kernel_of(name);
    // the two image-scale kernels of the detection: the FIRST chunk of every step (min(retrack_slots, lanes flagged in that step)
    // detections; steps without device-side detection do not count) - roam_engine_kernel_chunk_ms has every chunk
    const bool det = k == KN_INTEGRAL || k == KN_DET;
    if (k > KN_DET) { ROAM_SET_ERR(ctx, "unknown kernel '%s'", name); return ROAM_E_ARG; }
    if (det && !e->rt_on) { ROAM_SET_ERR(ctx, "engine created without retrack_on_device"); return ROAM_E_STATE; }
    if (!e->stepped) { ROAM_SET_ERR(ctx, "run a step first"); return ROAM_E_STATE; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t n = std::min<int64_t>(std::min<int64_t>(last_steps, e->nstep), 64);
    // the ring the kernel's pairs are in, and the pair: peaks and pyramid have their own streams' pairs
    hipEvent_t *ring = det ? &e->rt_ev[0][0] : &e->tr_ev[0][0];
    const int pitch = det ? 3 * RT_TRACE_CHUNKS : 6;
    const bool *ok = det ? e->rt_ev_ok : e->tr_ev_ok;                       // (a step enqueued while the events were switched off has none)
    const int a0 = det ? k - KN_INTEGRAL : (k == ST_PYR ? 3 : (k == ST_WARP ? 1 : 0));
    const int a1 = det ? a0 + 1 : (k == ST_PYR ? 4 : (k == ST_WARP ? 2 : 5));
    double sum = 0;
    int64_t used = 0;
    for (int64_t i = e->nstep - n; i < e->nstep; i++) {
        if (!ok[i & 63]) continue;
        float ms = 0;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ring[(i & 63) * pitch + a0], ring[(i & 63) * pitch + a1]));
        sum += ms; used++;
    }
    *avg_ms = used ? (float)(sum / (double)used) : 0.f;
    *n_used = (int32_t)used;
    return ROAM_OK;
}

// detections per launch of a detection kernel inside a step (retrack_slots, or the chunk of the two-stream form)
int32_t roam_engine_detect_chunk(roam_ctx *ctx, int32_t *chunk)
{
    ENGINE();
    ARG_CHECK(ctx, chunk);
    if (!e->rt_on) { ROAM_SET_ERR(ctx, "engine created without retrack_on_device"); return ROAM_E_STATE; }
    *chunk = e->det_chunk();
    return ROAM_OK;
}

// launch durations of a detection kernel, chunk by chunk: ms_out[s * chunks + c] = chunk c of the s-th of the last `steps_out`
// steps (oldest first; -1 for a step without device-side detection).  A step launches `chunks` = ceil(lanes / retrack_slots) chunks
// (at most RT_TRACE_CHUNKS are traced) whatever the number of lanes that re-detect - only the device knows it - and chunk c holds
// clamp(n - c * retrack_slots, 0, retrack_slots) of the step's n detections: the caller has n in the step's result records
int32_t roam_engine_kernel_chunk_ms(roam_ctx *ctx, const char *name, int32_t last_steps, float *ms_out, int32_t cap, int32_t *chunks,
                                    int32_t *steps_out)
{
    ENGINE();
    ARG_CHECK(ctx, name && last_steps >= 1 && ms_out && chunks && steps_out);
    const int kd = kernel_of(name) - KN_INTEGRAL;
    if (kd < 0 || kd > 1) { ROAM_SET_ERR(ctx, "unknown kernel '%s'", name); return ROAM_E_ARG; }
    if (!e->rt_on) { ROAM_SET_ERR(ctx, "engine created without retrack_on_device"); return ROAM_E_STATE; }
    if (!e->stepped) { ROAM_SET_ERR(ctx, "run a step first"); return ROAM_E_STATE; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t n = std::min<int64_t>(std::min<int64_t>(last_steps, e->nstep), 64);
    const int nchunk = std::min((e->B + e->det_chunk() - 1) / e->det_chunk(), RT_TRACE_CHUNKS);
    ARG_CHECK(ctx, (int64_t)cap >= n * nchunk);
    for (int64_t i = e->nstep - n, s = 0; i < e->nstep; i++, s++)
        for (int c = 0; c < nchunk; c++) {
            float ms = -1.f;
            if (e->rt_ev_ok[i & 63]) HIP_TRY(ctx, hipEventElapsedTime(&ms, e->rt_ev[i & 63][3 * c + kd], e->rt_ev[i & 63][3 * c + kd + 1]));
            ms_out[s * nchunk + c] = ms;
        }
    *chunks = nchunk;
    *steps_out = (int32_t)n;
    return ROAM_OK;
}

// re-launch one streaming kernel of the step `reps` times over all lanes (inputs resident, outputs
// overwritten in the scratch "next" pyramid / peak buffers) and time it with HIP events on the
// context stream.  algo_bytes = algorithmic HBM bytes per launch.
int32_t roam_engine_time_kernel(roam_ctx *ctx, const char *name, int32_t reps, float *avg_ms, double *algo_bytes)
{
    ENGINE();
    ARG_CHECK(ctx, name && reps >= 1 && avg_ms);
    if (!e->stepped) { ROAM_SET_ERR(ctx, "run a step first"); return ROAM_E_STATE; }
    const int k = kernel_of(name);
    if (k == KN_UNKNOWN) { ROAM_SET_ERR(ctx, "unknown kernel '%s'", name); return ROAM_E_ARG; }
    if (k >= KN_INTEGRAL && !e->rt_on) { ROAM_SET_ERR(ctx, "engine created without retrack_on_device"); return ROAM_E_STATE; }
    hipStream_t st = ctx->stream;
    const roam_engine_cfg &c = e->cfg;
    const int B = e->B;
    uint8_t *next = e->pyr[(e->cur + 1) & 3];       // not the live "previous" pyramid
    double bytes = 0;
    hipEvent_t a, b;
    HIP_TRY(ctx, hipEventCreate(&a));
    HIP_TRY(ctx, hipEventCreate(&b));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipEventRecord(a, st));
    for (int r = 0; r < reps; r++) {
        if (k == ST_WARP) {
            HIP_TRY(ctx, launch_warp_gather(st, e->warp_map, pool_warp_src(e, e->scan_idx[e->pk]), B, c.rows, c.clip, next, e->pd.lane_stride, e->warp_dark_zero));
            bytes = (double)B * ((double)c.rows * c.clip + (double)e->W * e->W);
        } else if (k == ST_PEAKS) {
            PeakSrc ps = {e->pool, (int64_t)e->rec_bytes, (int64_t)c.stride, c.payload_off, 1, e->scan_idx[e->pk]};
            hipError_t er = launch_peaks(st, ps, B, c.rows, c.clip, e->row_stage, e->stage_cap, e->row_count, e->peaks_out[(e->pk + 1) % 3], c.peaks_cap, e->peaks_n[(e->pk + 1) % 3]);
            HIP_TRY(ctx, er);
            bytes = (double)B * ((double)c.rows * c.clip);
        } else if (k == ST_PYR) {
            HIP_TRY(ctx, launch_build_pyramid(st, next, e->pd, B, e->pyr_dark));
            double rd = 0, wr = 0;
            for (int l = 0; l + 1 < ROAM_PYR_LEVELS; l++) { rd += (double)e->pd.w[l] * e->pd.h[l]; wr += (double)e->pd.w[l + 1] * e->pd.h[l + 1]; }
            bytes = (double)B * (rd + wr);
        } else {
            // the image-scale kernels of the device-side retrack over all scratch slots (per launch: `slots` detections)
            const int P = e->rt.slots, which = k < KN_FUSED ? k - KN_INTEGRAL : 2 + (name[9] == ':' ? atoi(name + 10) : 0);
            if (which >= 2) ROAM_TRY(fused_tables(ctx, e));       // (made on first use)
            if (r == 0) {
                ROAM_TRY(detect_slots(ctx, e, P));
                if (which == 1) HIP_TRY(ctx, launch_retrack_part(st, e->rt, P, 0));      // valid integral images to work on
                HIP_TRY(ctx, hipStreamSynchronize(st));
                HIP_TRY(ctx, hipEventRecord(a, st));
            }
            HIP_TRY(ctx, launch_retrack_part(st, e->rt, P, which));
            if (which >= 1) HIP_TRY(ctx, hipMemsetAsync(e->rt.cand_n, 0, sizeof(int32_t) * (size_t)P, st));   // (no bookkeeping follows that would clear the counts)
            const double npx = (double)e->W * e->W;
            // algorithmic bytes per detection (strict): integral image = polar payload read + float64 image written once
            // (the 4-byte sampling-map word per pixel it also reads is the same geometry table for every detection and mostly comes
            // out of L2: not input data, not counted since round 4); determinants + maxima = float64 image read once (the
            // candidates it writes are a few KB)
            // the fused kernel: the polar payload is all a detection reads; the float64 image never leaves the CU
            // round 6: the part of the image that exists - the tiles the determinant kernel reads, the only ones the integral kernel
            // writes (retrack_build_phases): 87.7 % of a 2024 x 2024 image; rounds 2-5 counted the whole image for both kernels
            const double ipx = e->rt_image_px > 0 ? (double)e->rt_image_px : npx;
            bytes = (double)P * (which == 0 ? ((double)c.rows * c.clip + ipx * 8.0) : (which == 1 ? ipx * 8.0 : (double)c.rows * c.clip));
        }
    }
    HIP_TRY(ctx, hipEventRecord(b, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, a, b));
    hipEventDestroy(a); hipEventDestroy(b);
    *avg_ms = ms / reps;
    if (algo_bytes) *algo_bytes = bytes;
    return ROAM_OK;
}

// diagnostics: the image-scale detection kernels of `n_slots` detections (scratch slot i works on the scan lane i % lanes saw last) in the
// two-kernel form (fused = 0: rt_integral_kernel + rt_det_strip_kernel) or as rt_fused_kernel (fused = 1), candidates sorted into
// (row, column, layer) order.  Out: per slot the count (cand_n, may exceed cap_per_slot) and the first cap_per_slot candidates; S_out
// (optional, W x W doubles): the integral image of slot `s_slot` as that form computed it.  The parity tests hold the two forms equal.
int32_t roam_engine_debug_detect(roam_ctx *ctx, int32_t fused, int32_t n_slots, int32_t cap_per_slot, uint32_t *rc_out, double *val_out,
                                 int32_t *n_out, int32_t s_slot, double *S_out)
{
    ENGINE();
    ARG_CHECK(ctx, n_slots >= 1 && cap_per_slot >= 0 && n_out);
    if (!e->rt_on || !e->stepped) { ROAM_SET_ERR(ctx, "debug_detect: needs retrack_on_device and one step"); return ROAM_E_STATE; }
    ARG_CHECK(ctx, n_slots <= e->rt.slots && n_slots <= e->B && (!S_out || (s_slot >= 0 && s_slot < n_slots)));
    hipStream_t st = ctx->stream;
    const int P = n_slots;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ROAM_TRY(detect_slots(ctx, e, P));
    HIP_TRY(ctx, hipMemsetAsync(e->rt.cand_n, 0, sizeof(int32_t) * (size_t)P, st));
    if (fused) ROAM_TRY(fused_tables(ctx, e));
    if (fused) HIP_TRY(ctx, launch_retrack_part(st, e->rt, P, S_out ? 3 : 2));
    else { HIP_TRY(ctx, launch_retrack_part(st, e->rt, P, 0)); HIP_TRY(ctx, launch_retrack_part(st, e->rt, P, 1)); }
    HIP_TRY(ctx, launch_retrack_emit(st, e->rt, P));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipMemcpy(n_out, e->rt.cand_n, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost));
    const int keep = std::min(cap_per_slot, BP_MAX_PTS);
    for (int i = 0; i < P && keep > 0; i++) {
        if (rc_out) HIP_TRY(ctx, hipMemcpy(rc_out + (size_t)i * cap_per_slot, e->rt.cand_rc + (size_t)i * BP_MAX_PTS, sizeof(uint32_t) * (size_t)keep, hipMemcpyDeviceToHost));
        if (val_out) HIP_TRY(ctx, hipMemcpy(val_out + (size_t)i * cap_per_slot, e->rt.cand_val + (size_t)i * BP_MAX_PTS, sizeof(double) * (size_t)keep, hipMemcpyDeviceToHost));
    }
    if (S_out)
        HIP_TRY(ctx, hipMemcpy2D(S_out, sizeof(double) * (size_t)e->W, e->rt.S + (size_t)s_slot * e->rt.SP * e->W, sizeof(double) * (size_t)e->rt.SP,
                                 sizeof(double) * (size_t)e->W, (size_t)e->W, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemset(e->rt.cand_n, 0, sizeof(int32_t) * (size_t)P));     // the lists are clean for the next detection
    return ROAM_OK;
}

// test entry: the blob bookkeeping alone (K4-K6: candidate order, _prune_blobs with its pair order, sigma argsort, SSC) on the caller's
// candidate lists, through the engine's own per-detection scratch and the ONE call a step makes - launch_retrack_bookkeeping(st, rt, P,
// nullptr) with the device count rt_n = P - so P picks the launch form (rt_book_kernel below 256, emit + small + full class from 256,
// longest list first from 512).  cand_rc / cand_val: P lists of `rows_given` rows each (rc = row << 16 | col << 2 | layer, any order,
// keys distinct); cand_n[p] is the count the determinant kernel would have left: it may exceed rows_given only beyond BP_MAX_PTS
// (then rows_given = BP_MAX_PTS).  Outputs (kp_out P x BP_MAX_PTS x 3, sel_out P x BP_MAX_PTS, the others P) are what the kernels left in
// scratch prefilled with 0xff bytes (kp: NaN) / 0x7f bytes (the int32 arrays).  pairs_out (optional, P x (BP_MAX_PAIRS + 1)): the pair
// scratch as the kernels left it - the candidate pairs i << 16 | j (i < j, response-order indices) in query_pairs' EMISSION order
// from entry 0 on (the caller knows how many there are); meaningless after a tree / task overflow.
int32_t roam_engine_debug_blobs(roam_ctx *ctx, int32_t P, int32_t rows_given, const uint32_t *cand_rc, const double *cand_val,
                                const int32_t *cand_n, int32_t *kp_n_out, double *kp_out, int32_t *flags_out, int32_t *sel_n_out,
                                int32_t *sel_out, uint32_t *pairs_out)
{
    ENGINE();
    if (!e->rt_on) { ROAM_SET_ERR(ctx, "debug_blobs: needs retrack_on_device"); return ROAM_E_STATE; }
    ARG_CHECK(ctx, P >= 1 && P <= e->B && rows_given >= 0 && rows_given <= BP_MAX_PTS && cand_n && kp_n_out && kp_out && flags_out && sel_n_out && sel_out);
    ARG_CHECK(ctx, rows_given == 0 || (cand_rc && cand_val));
    std::vector<uint32_t> keys;
    for (int p = 0; p < P; p++) {
        ARG_CHECK(ctx, cand_n[p] >= 0 && std::min(cand_n[p], BP_MAX_PTS) <= rows_given);
        const int n = std::min(cand_n[p], BP_MAX_PTS);
        keys.assign(cand_rc + (size_t)p * rows_given, cand_rc + (size_t)p * rows_given + n);
        for (uint32_t k : keys) {
            const int layer = (int)(k & 3u);
            ARG_CHECK(ctx, (int)(k >> 16) < e->W && (int)((k >> 2) & 0x3fffu) < e->W && (layer == 1 || layer == 2));
        }
        std::sort(keys.begin(), keys.end());
        ARG_CHECK(ctx, std::adjacent_find(keys.begin(), keys.end()) == keys.end());     // K4 ranks by key: a repeated key leaves a row unwritten
    }
    hipStream_t st = ctx->stream;
    RtArgs &r = e->rt;
    const size_t D = (size_t)P;
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (rows_given > 0) {
        HIP_TRY(ctx, hipMemcpy2DAsync(r.cand_rc, sizeof(uint32_t) * BP_MAX_PTS, cand_rc, sizeof(uint32_t) * (size_t)rows_given,
                                      sizeof(uint32_t) * (size_t)rows_given, D, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpy2DAsync(r.cand_val, sizeof(double) * BP_MAX_PTS, cand_val, sizeof(double) * (size_t)rows_given,
                                      sizeof(double) * (size_t)rows_given, D, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx, hipMemcpyAsync(r.cand_n, cand_n, sizeof(int32_t) * D, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(r.rt_n, &P, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(r.kp, 0xff, sizeof(double) * D * BP_MAX_PTS * 3, st));
    HIP_TRY(ctx, hipMemsetAsync(r.sel, 0x7f, sizeof(int32_t) * D * BP_MAX_PTS, st));
    for (int32_t *q : {r.kp_n, r.slot_flags, r.sel_n}) HIP_TRY(ctx, hipMemsetAsync(q, 0x7f, sizeof(int32_t) * D, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                                          // (the host arrays above are pageable)
    HIP_TRY(ctx, launch_retrack_bookkeeping(st, r, P, nullptr));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipMemcpy(kp_out, r.kp, sizeof(double) * D * BP_MAX_PTS * 3, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(sel_out, r.sel, sizeof(int32_t) * D * BP_MAX_PTS, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(kp_n_out, r.kp_n, sizeof(int32_t) * D, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(flags_out, r.slot_flags, sizeof(int32_t) * D, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(sel_n_out, r.sel_n, sizeof(int32_t) * D, hipMemcpyDeviceToHost));
    if (pairs_out) HIP_TRY(ctx, hipMemcpy(pairs_out, r.pairs, sizeof(uint32_t) * D * (BP_MAX_PAIRS + 1), hipMemcpyDeviceToHost));
    // the scratch as a detection expects it: empty lists (rt_append_kernel clears them in a step), no count left at RT_BLOBS_REDO
    for (int32_t *q : {r.cand_n, r.kp_n, r.slot_flags, r.sel_n}) HIP_TRY(ctx, hipMemset(q, 0, sizeof(int32_t) * D));
    const int32_t zero = 0;
    HIP_TRY(ctx, hipMemcpy(r.rt_n, &zero, sizeof(int32_t), hipMemcpyHostToDevice));
    return ROAM_OK;
}

}  // extern "C"
