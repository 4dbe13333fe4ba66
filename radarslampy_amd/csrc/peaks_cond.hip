// polar peak extraction WITH scipy.signal.find_peaks' distance / prominence conditions (a2 with its two tuning knobs).
//
// getPointCloud.getPointCloudPolarInd(polarImage, peakDistance, peakProminence) (reference getPointCloud.py:11-54) hands both
// arguments to find_peaks(row, distance=..., prominence=...).  Per azimuth row, in find_peaks' order:
//   candidates  _local_maxima_1d: strict rise, strict fall, a plateau once at its midpoint (l + r) / 2, end samples never
//   distance    _select_by_peak_distance with d = ceil(distance): the candidates in the order of np.argsort(heights) - NumPy 1.22.3's
//               unstable introsort, which the reference pins and which decides between equal heights (u8-derived rows are full of
//               them) - walked from the highest priority down; a kept peak suppresses every other within |position difference| < d
//   prominence  _peak_prominences with wlen=None on the distance survivors, in float64 on the widened samples as find_peaks computes
//               it, then pmin <= prom <= pmax (either bound optional)
//   threshold   the reference's own h >= mean(h) + std(h) in float32, NumPy pairwise summation order (peaks_common.h)
// One wavefront per azimuth row (grid = rows x lanes), cols <= ROAM_MAX_COLS: the row stays in LDS in its source type (u8 codes:
// k -> k/255 is strictly increasing, so the codes order, compare and bound exactly like the decoded values); the sort is
// rb_aquicksort_wave (npsort_wave.h) on the candidate heights; the greedy walk is wave-uniform over the priority order with the lanes
// clearing the contiguous index range around a kept peak; prominence is a lane per surviving peak that walks its own 64-sample block
// and then skips whole blocks by their max / min summaries (a search of <= 3 x 64 samples instead of up to a whole row).  Survivors go
// to the same per-row staging layout as peaks.hip, and peaks.hip's gather kernel emits the (P, 2) list.
#include "roam_internal.h"
#include "peaks_common.h"
#include "npsort_wave.h"
#include <math.h>
#include <type_traits>

#define PKC_MAXC ROAM_MAX_COLS
#define PKC_MAXP (PKC_MAXC / 2)          // candidates of a row: at most (cols - 1) / 2 (two are never adjacent)
#define PKC_BLK 64                        // samples per block summary of the prominence search

__device__ __forceinline__ float pkc_val(uint8_t k) { return code_to_f32_pk(k); }
__device__ __forceinline__ float pkc_val(float v) { return v; }

template <typename K>
struct PkcLds {
    K xs[PKC_MAXC];                       // the row in its source type
    K ck[PKC_MAXP];                       // candidate heights, range order
    uint16_t pm[PKC_MAXP];                // candidate positions
    int16_t ts[PKC_MAXP];                 // priority order (argsort of ck); afterwards the positions of the survivors
    uint8_t keep[PKC_MAXP];
    K bmax[PKC_MAXC / PKC_BLK], bmin[PKC_MAXC / PKC_BLK];
    float leaf_sum[64];
    union {
        struct { uint16_t Lp[PKC_MAXP], Rp[PKC_MAXP]; int work[3 * 256]; } s;      // the sort's scratch
        struct { float h[PKC_MAXP], sq[PKC_MAXP]; } f;                              // the threshold's
    } u;
};

template <bool U8>
__global__ __launch_bounds__(64) void peaks_cond_rows_kernel(PeakSrc src, int rows, int cols, PeakCond cond,
                                                             uint16_t *__restrict__ row_stage, int stage_cap,
                                                             int32_t *__restrict__ row_count)
{
    typedef typename std::conditional<U8, uint8_t, float>::type K;
    __shared__ __align__(16) PkcLds<K> L;
    const int lane = threadIdx.x, b = blockIdx.y, r = blockIdx.x;
    int32_t *cnt_out = row_count + (int64_t)b * rows + r;
    const int64_t lane_sel = src.lane_index ? (int64_t)src.lane_index[b] : (int64_t)b;
    if (U8) {
        const uint8_t *p = reinterpret_cast<const uint8_t *>(src.base) + lane_sel * src.lane_stride + (int64_t)r * src.row_stride +
                           src.payload_off;
        for (int i = lane; i < cols; i += 64) L.xs[i] = (K)p[i];
    } else {
        const float *p = reinterpret_cast<const float *>(src.base) + lane_sel * src.lane_stride + (int64_t)r * src.row_stride;
        for (int i = lane; i < cols; i += 64) L.xs[i] = (K)p[i];
    }
    __syncthreads();

    // ---- candidates (plateau rule), a contiguous chunk of bins per lane keeps range order
    const int items = (cols + 63) / 64;
    const int lo = lane * items, hi = min(lo + items, cols), imax = cols - 1;
    int cnt = 0;
    for (int i = max(lo, 1); i < hi && i < imax; i++) {
        const K v = L.xs[i];
        if (L.xs[i - 1] < v) {
            int ia = i + 1;
            while (ia < imax && L.xs[ia] == v) ia++;
            if (L.xs[ia] < v) cnt++;
        }
    }
    int M;
    int pos = wave_excl_scan(cnt, lane, &M);
    for (int i = max(lo, 1); i < hi && i < imax; i++) {
        const K v = L.xs[i];
        if (L.xs[i - 1] < v) {
            int ia = i + 1;
            while (ia < imax && L.xs[ia] == v) ia++;
            if (L.xs[ia] < v) {
                L.ck[pos] = v;
                L.pm[pos] = (uint16_t)((i + ia - 1) >> 1);
                pos++;
            }
        }
    }
    for (int k = lane; k < M; k += 64) L.keep[k] = 1;
    __syncthreads();
    if (M == 0) {
        if (lane == 0) *cnt_out = 0;
        return;
    }

    // ---- distance: NumPy 1.22.3 argsort of the heights, then the greedy walk from the highest priority down
    if (cond.dist > 0) {
        rb_aquicksort_wave(L.ck, M, L.ts, lane, L.u.s.work, L.u.s.Lp, L.u.s.Rp);
        const int d = cond.dist;
        for (int i = M - 1; i >= 0; i--) {
            const int j = __builtin_amdgcn_readfirstlane(L.ts[i]);
            if (!__builtin_amdgcn_readfirstlane(L.keep[j])) continue;
            const int pj = __builtin_amdgcn_readfirstlane(L.pm[j]);
            for (int k0 = j - 1; k0 >= 0; k0 -= 64) {                // positions ascend: the suppressed peaks are contiguous
                const int k = k0 - lane;
                const bool hit = k >= 0 && pj - (int)L.pm[k] < d;
                if (hit) L.keep[k] = 0;
                if (__ballot(hit) != ~0ull) break;
            }
            for (int k0 = j + 1; k0 < M; k0 += 64) {
                const int k = k0 + lane;
                const bool hit = k < M && (int)L.pm[k] - pj < d;
                if (hit) L.keep[k] = 0;
                if (__ballot(hit) != ~0ull) break;
            }
            __syncthreads();
        }
    }

    // ---- prominence of the survivors (wlen=None): the bases are the nearest samples that are not <= the peak (higher, or NaN)
    if (cond.has_prom) {
        const int nb = (cols + PKC_BLK - 1) / PKC_BLK;
        if (lane < nb) {
            const int b0 = lane * PKC_BLK, b1 = min(b0 + PKC_BLK, cols);
            K mx = L.xs[b0], mn = L.xs[b0];
            for (int i = b0 + 1; i < b1; i++) {
                const K v = L.xs[i];
                mx = (v > mx || v != v) ? v : mx;                   // a NaN sticks: the block is never skipped over
                mn = v < mn ? v : mn;
            }
            L.bmax[lane] = mx;
            L.bmin[lane] = mn;
        }
        __syncthreads();
        for (int k = lane; k < M; k += 64) {
            if (!L.keep[k]) continue;
            const int pk = L.pm[k], bk = pk / PKC_BLK;
            const K h = L.xs[pk];
            K lmin = h, rmin = h;
            int i = pk - 1;
            for (; i >= bk * PKC_BLK; i--) {
                const K v = L.xs[i];
                if (!(v <= h)) break;
                lmin = v < lmin ? v : lmin;
            }
            if (i < bk * PKC_BLK) {                                  // the own block did not end the search
                int bb = bk - 1;
                for (; bb >= 0 && L.bmax[bb] <= h; bb--) lmin = L.bmin[bb] < lmin ? L.bmin[bb] : lmin;
                if (bb >= 0)
                    for (i = bb * PKC_BLK + PKC_BLK - 1; i >= bb * PKC_BLK; i--) {
                        const K v = L.xs[i];
                        if (!(v <= h)) break;
                        lmin = v < lmin ? v : lmin;
                    }
            }
            const int bend = min(bk * PKC_BLK + PKC_BLK, cols);
            for (i = pk + 1; i < bend; i++) {
                const K v = L.xs[i];
                if (!(v <= h)) break;
                rmin = v < rmin ? v : rmin;
            }
            if (i == bend) {
                int bb = bk + 1;
                for (; bb < nb && L.bmax[bb] <= h; bb++) rmin = L.bmin[bb] < rmin ? L.bmin[bb] : rmin;
                if (bb < nb)
                    for (i = bb * PKC_BLK; i < min(bb * PKC_BLK + PKC_BLK, cols); i++) {
                        const K v = L.xs[i];
                        if (!(v <= h)) break;
                        rmin = v < rmin ? v : rmin;
                    }
            }
            const K base = lmin < rmin ? rmin : lmin;
            const double prom = __dsub_rn((double)pkc_val(h), (double)pkc_val(base));
            const bool ok = (isnan(cond.prom_min) || cond.prom_min <= prom) && (isnan(cond.prom_max) || prom <= cond.prom_max);
            if (!ok) L.keep[k] = 0;
        }
        __syncthreads();
    }

    // ---- survivors in range order -> float32 heights + positions, then the reference's mean + std threshold
    const int kitems = (M + 63) / 64;
    const int klo = lane * kitems, khi = min(klo + kitems, M);
    int c = 0;
    for (int k = klo; k < khi; k++) c += L.keep[k];
    int M2;
    int q = wave_excl_scan(c, lane, &M2);
    uint16_t *fp = reinterpret_cast<uint16_t *>(L.ts);
    float *hh = L.u.f.h, *sq = L.u.f.sq;
    for (int k = klo; k < khi; k++)
        if (L.keep[k]) {
            hh[q] = pkc_val(L.ck[k]);
            fp[q] = L.pm[k];
            q++;
        }
    __syncthreads();
    if (M2 == 0) {                                                   // numpy: mean of empty = NaN -> nothing passes
        if (lane == 0) *cnt_out = 0;
        return;
    }
    const float fM = (float)M2;
    const float mean = __fdiv_rn(block_np_sum(L.leaf_sum, hh, M2), fM);
    for (int k = lane; k < M2; k += 64) {
        const float dd = __fsub_rn(hh[k], mean);
        sq[k] = __fmul_rn(dd, dd);
    }
    __syncthreads();
    const float var = __fdiv_rn(block_np_sum(L.leaf_sum, sq, M2), fM);
    const float thr = __fadd_rn(mean, rn_sqrtf(var));

    const int titems = (M2 + 63) / 64;
    const int tlo = lane * titems, thi = min(tlo + titems, M2);
    int c2 = 0;
    for (int k = tlo; k < thi; k++) c2 += (hh[k] >= thr) ? 1 : 0;
    int total;
    int p2 = wave_excl_scan(c2, lane, &total);
    uint16_t *dst = row_stage + ((int64_t)b * rows + r) * stage_cap;
    for (int k = tlo; k < thi; k++)
        if (hh[k] >= thr) {
            if (p2 < stage_cap) dst[p2] = fp[k];
            p2++;
        }
    if (lane == 0) *cnt_out = total;
}

hipError_t launch_peaks_cond(hipStream_t st, PeakSrc src, int B, int rows, int cols, PeakCond cond, uint16_t *row_stage,
                             int stage_cap, int32_t *row_count, int32_t *out, int32_t cap, int32_t *n_out)
{
    if (cols < 1 || cols > PKC_MAXC || stage_cap < (cols + 1) / 2) return hipErrorInvalidValue;
    if (src.is_u8)
        hipLaunchKernelGGL(peaks_cond_rows_kernel<true>, dim3(rows, B), dim3(64), 0, st, src, rows, cols, cond, row_stage, stage_cap,
                           row_count);
    else
        hipLaunchKernelGGL(peaks_cond_rows_kernel<false>, dim3(rows, B), dim3(64), 0, st, src, rows, cols, cond, row_stage, stage_cap,
                           row_count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_peaks_gather(st, B, rows, row_stage, stage_cap, row_count, out, cap, n_out);
}
