// Device-side feature (re)detection of the engine: appendNewFeatures(currImgCart, good_new) of the reference's loop
// (RawROAMSystem.py:250-271, getFeatures.py:74-118) for every lane whose step ran out of features, inside
// roam_engine_step, without a host round trip.  Per flagged lane ("slot" = one detection):
//   K1+K2 rt_integral    the float64 integral image in ONE sweep: float32 Cartesian pixel from the polar record through the engine's
//                        sampling map (the arithmetic of warp.hip, never written to memory; the polar footprint of a wave's patch
//                        staged in LDS), phases of 64 rows x 64 columns: column cumsum by four stacked waves of 16 rows each (exact
//                        in float64 in any order), row cumsum by a fifth wave through double-buffered LDS tiles in NumPy's
//                        sequential order, image written once.  Chunks of fewer than RT_TWO_PASS_SLOTS detections (and a lane's
//                        first detection) take rt_integ_cols + rt_integ_rows instead: thousands of threads per detection
//   K3 rt_det_strip      box-filter Hessian determinants of both live layers (sigma 5.005 / 10, sizes 15 / 30; the sigma 0.01 layer
//                        is all-NaN in scikit-image and ignored): workgroups march down 62-column strips of the integral image with
//                        its rows in an LDS ring (each byte fetched ~1.4 times), over the steps of the strip that lie inside the
//                        maximum range (a table, geometry only); dxy boxes only where dxx*dyy can pass the threshold; 3x3x3 maxima above the threshold are appended to the detection's candidate list
//   K4 rt_emit           the candidates sorted into C (row, col, layer) order
//   K5 rt_blobs          one wavefront per lane: response order, scikit-image's _prune_blobs in ITS pair order (blobprune.h:
//                        cKDTree emission order + CPython set order; the tree is built level by level with one lane per node, the
//                        traversal and the set order run on lane 0 out of LDS), NumPy-1.22 argsort of the sigmas -> keypoints in
//                        adaptiveNMS's priority order
//   K6 ssc_batch         ANMS.ssc (ssc.hip)
//   K7 rt_append         [x, y] flip, vstack + drop exact duplicates keeping the first (getFeatures.py:109-112), keyframe
//                        refresh (Mapping.py:59-66 with the frame's velocity), feature count
// The image-scale kernels (K1-K3) run in chunks of `slots` detections (scratch: a 33 MB integral image per slot); K3 appends to
// per-DETECTION candidate lists, and K4-K7 run once over all detections of the step.  Every kernel exits at once for
// detections beyond the number of flagged lanes, which only the device knows.
// One translation unit per part (shared: retrack_geom.h): K0, K7, schedule here; K1 / K2 retrack_integral.hip; K3, fused K1-K3 retrack_det.hip; K4-K6 retrack_blobs.hip
#include "retrack_geom.h"

#define KS ROAM_MAX_FEATURES
#define CART_CENTER 1012.0
#define M_PER_PX 0.0864
#define TWO_PI 6.283185307179586476925286766559

// ------------------------------------------------------------------------------------------------ K0: flagged lanes
__global__ __launch_bounds__(256) void rt_collect_kernel(const roam_lane_result *__restrict__ res, const int32_t *__restrict__ scan_idx,
                                                         int B, int force_all, int32_t *__restrict__ rt_lane,
                                                         int32_t *__restrict__ rt_scan, int32_t *__restrict__ rt_n)
{
    __shared__ int sh[8];
    __shared__ int base_s;
    const int t = threadIdx.x;
    if (t == 0) base_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + t;
        const int f = (b < B && (force_all || (res[b].flags & 4))) ? 1 : 0;
        // block exclusive scan
        const int lane = t & 63, w = t >> 6;
        int inc = f;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { int n = __shfl_up(inc, d); if (lane >= d) inc += n; }
        if (lane == 63) sh[w] = inc;
        __syncthreads();
        int off = base_s, tot = 0;
        for (int i = 0; i < 4; i++) { if (i < w) off += sh[i]; tot += sh[i]; }
        if (f) { rt_lane[off + inc - 1] = b; rt_scan[off + inc - 1] = scan_idx[b]; }
        __syncthreads();
        if (t == 0) base_s += tot;
        __syncthreads();
    }
    if (t == 0) *rt_n = base_s;
}

// ------------------------------------------------------------------------------------------------ K7: append + keyframe refresh
__global__ __launch_bounds__(256) void rt_append_kernel(RtArgs a, int first)
{
    __shared__ float nx[KS + 256], ny[KS + 256];
    __shared__ uint8_t keep[KS + 256];
    __shared__ int sh[8];
    const int ls = blockIdx.x, slot = first + ls;
    if (slot >= *a.rt_n) return;
    const int b = a.rt_lane[slot], t = threadIdx.x;
    if (t == 0) a.cand_n[ls] = 0;                                             // the last reader of the list is done: clean for the next detection
    float *feat = a.feat + (int64_t)b * KS * 2;
    const int n_old = min(a.feat_n[b], KS);
    const int n_sel = min(a.sel_n[ls], 256);                                  // (ANMS returns at most 220; more would be dropped: flagged below)
    const double *kp = a.kp + (int64_t)ls * BP_MAX_PTS * 3;
    const int32_t *sel = a.sel + (int64_t)ls * BP_MAX_PTS;
    // vstack((old, fliplr(new[:, :2])))  (getFeatures.py:101-109)
    for (int i = t; i < n_old; i += 256) { nx[i] = feat[2 * i]; ny[i] = feat[2 * i + 1]; }
    for (int i = t; i < n_sel; i += 256) { const int q = sel[i]; nx[n_old + i] = (float)kp[3 * q + 1]; ny[n_old + i] = (float)kp[3 * q]; }
    __syncthreads();
    const int tot = n_old + n_sel;
    // np.unique(axis=0, return_index) + sort(idx): drop a row when an earlier row is identical
    for (int i = t; i < tot; i += 256) {
        bool dup = false;
        for (int j = 0; j < i && !dup; j++) dup = nx[j] == nx[i] && ny[j] == ny[i];
        keep[i] = dup ? 0 : 1;
    }
    __syncthreads();
    // ordered compaction (tot <= KS + 256 -> 5 items per thread)
    const int items = (KS + 256 + 255) / 256, lo = t * items, hi = min(lo + items, tot);
    int c = 0;
    for (int i = lo; i < hi; i++) c += keep[i];
    const int lane = t & 63, w = t >> 6;
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { int n = __shfl_up(inc, d); if (lane >= d) inc += n; }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int pos = inc - c, total = 0;
    for (int i = 0; i < 4; i++) { if (i < w) pos += sh[i]; total += sh[i]; }
    const int m = min(total, KS);
    const double v0 = a.vel[3 * b], v1 = a.vel[3 * b + 1], v2 = a.vel[3 * b + 2];
    double *und = a.kf_und + (int64_t)b * KS * 2;
    for (int i = lo; i < hi; i++)
        if (keep[i]) {
            if (pos < KS) {
                feat[2 * pos] = nx[i]; feat[2 * pos + 1] = ny[i];
                // possible_kf.updateInfo(latestPose, centered_new, ..., velocity): undistort (Mapping.py:59-66)
                const double x = ((double)nx[i] - CART_CENTER) * M_PER_PX, y = ((double)ny[i] - CART_CENTER) * M_PER_PX;
                const double dT = 0.25 * atan2(-y, -x) / TWO_PI;
                const double ang = v2 * dT, ca = cos(ang), sa = sin(ang);
                und[2 * pos] = ca * x - sa * y + v0 * dT;
                und[2 * pos + 1] = sa * x + ca * y + v1 * dT;
            }
            pos++;
        }
    if (t == 0) {
        a.feat_n[b] = m;
        if (a.res) {
            a.res[b].flags |= 8 | (a.slot_flags[ls] << 8) | ((total > KS || a.sel_n[ls] > 256) ? (RT_F_FEAT_OVERFLOW << 8) : 0);
            a.res[b].n_after_retrack = m;
        }
    }
}

// ------------------------------------------------------------------------------------------------ launcher
hipError_t retrack_init() { const hipError_t e = retrack_det_init(); return e != hipSuccess ? e : retrack_integral_init(); }

bool retrack_sided(const RtArgs &a, int B, const RtSide *side) { return side && side->chunk > 0 && !a.fused && a.slots >= 2 * side->chunk && B > side->chunk; }

hipError_t launch_retrack(hipStream_t st, const RtArgs &a, int B, hipEvent_t *trace, int ntrace, hipEvent_t after_order, const RtSide *side)
{
    if (a.W > 2048) return hipErrorInvalidValue;                           // (roam_engine_create refuses such an engine)
    // image-scale kernels chunk by chunk (the float64 integral images of `slots` detections are resident at once); the candidate lists are
    // per DETECTION, so the lane-serial bookkeeping runs once over all of them afterwards (round 2 ran it per chunk: 1.4-2.7 ms of a near-idle
    // GPU each time).  (The candidate counts are zero on entry: rt_append_kernel, the last kernel of this chain, clears what a detection used.)
    // Sided: the determinants of chunk c on a second stream BESIDE the integral images of chunk c + 1 (round 6, late): chunks of side->chunk
    // detections, their integral images alternating between the two halves of the scratch.  The two kernels are latency-bound chains
    // at 10 % VALU / LDS utilisation each, and one workgroup of each per CU (80 + 74 KB of LDS) is a better pairing than two of a kind:
    // 70.3-70.7 -> 69.2-69.3 ms per step with chunks of 1 024 (768: nothing, 640: worse); same candidates (profiles/det_side_check.py).
    const bool sided = retrack_sided(a, B, side);
    const int C = sided ? side->chunk : a.slots;
    const hipStream_t dst = sided ? side->st : st;                         // the determinants' stream
    hipError_t e = hipSuccess;
    int nc = 0;
    for (int first = 0; first < B; first += C, nc++) {
        const int P = min(C, B - first);
        const bool tr = trace && nc < ntrace, big = B - first >= RT_TWO_PASS_SLOTS;      // (not big: fewer lanes left than the one-sweep kernel takes - it would return at once)
        hipEvent_t *tev = trace + 3 * nc;
        RtArgs ac = a;
        if (sided) ac.S = a.S + (size_t)(nc & 1) * C * a.SP * a.W;
        if (sided && nc >= 2 && (e = hipStreamWaitEvent(st, side->ev_d[(nc - 2) & 3], 0)) != hipSuccess) return e;      // this bank's determinants are done
        if (tr && (e = hipEventRecord(tev[0], st)) != hipSuccess) return e;
        if (big && a.fused && (e = launch_retrack_fused(st, ac, first, P, 0)) != hipSuccess) return e;       // (in place of the one-sweep kernel)
        if ((e = launch_retrack_integral(st, ac, first, P, big && !a.fused)) != hipSuccess) return e;
        if (tr && (e = hipEventRecord(tev[1], st)) != hipSuccess) return e;
        if (sided && (e = hipEventRecord(side->ev_i[nc & 3], st)) != hipSuccess) return e;
        if (sided && (e = hipStreamWaitEvent(dst, side->ev_i[nc & 3], 0)) != hipSuccess) return e;
        if ((e = launch_det(dst, ac, first, P)) != hipSuccess) return e;
        if (tr && (e = hipEventRecord(tev[2], dst)) != hipSuccess) return e;      // (sided: tev[1] .. tev[2] = the determinants, from the moment they could start)
        if (sided && (e = hipEventRecord(side->ev_d[nc & 3], dst)) != hipSuccess) return e;
    }
    for (int k = max(0, nc - 2); sided && k < nc; k++)
        if ((e = hipStreamWaitEvent(st, side->ev_d[k & 3], 0)) != hipSuccess) return e;
    if ((e = launch_retrack_bookkeeping(st, a, B, after_order)) != hipSuccess) return e;
    hipLaunchKernelGGL(rt_append_kernel, dim3(B), dim3(256), 0, st, a, 0);
    return hipGetLastError();
}

hipError_t launch_retrack_collect(hipStream_t st, const roam_lane_result *res, const int32_t *scan_idx, int B, int force_all, const RtArgs &a)
{
    hipLaunchKernelGGL(rt_collect_kernel, dim3(1), dim3(256), 0, st, res, scan_idx, B, force_all, a.rt_lane, a.rt_scan, a.rt_n);
    return hipGetLastError();
}

// measurement: the image-scale kernels again for the first `P` scratch slots (rt_n is set by the caller); which: retrack.h
hipError_t launch_retrack_part(hipStream_t st, const RtArgs &a_in, int P, int which)
{
    if (a_in.W > 2048) return hipErrorInvalidValue;
    RtArgs a = a_in;
    a.fused = which >= 2 ? 1 : 0;                                          // 0 / 1 time and check the two-kernel form whatever the engine runs
    if (which >= 2) return a.fd_mapT ? launch_retrack_fused(st, a, 0, P, which - 2) : hipErrorInvalidValue;
    if (which == 0) return launch_retrack_integral(st, a, 0, P, true);
    return launch_det(st, a, 0, P);                                         // (the caller clears the candidate counts: no bookkeeping follows that would)
}
