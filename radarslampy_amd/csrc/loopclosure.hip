// Loop-closure candidates by radar scan context (Kim et al., the MulRan data set).  The reference has no place recognition (a
// commented-out "import m2dp" at Mapping.py:7 and an unused Keyframe.pointCloud at :61-62), so parity is unpinned: the contract is
// tests/scan_context_model.py.  Kernels, the database and the ABI entries of the unit.
//
// Descriptor (scan_context_kernel).  The polar scan is area-averaged to S sectors x R rings with integer bin edges
// (floor(s rows / S), floor(r clip / R)).  One workgroup per (image, sector): the 256 lanes walk the clipped row, each summing its
// columns over the sector's rows (reads coalesced along range), the column sums go to LDS, then wave w adds the columns of the rings
// w, w + 4, ... with a fixed butterfly - no atomics, one order whatever the batch.  u8 record codes are summed as integers (exact);
// float32 images in float64.  The workgroup owns a whole sector column, so it also writes what a query needs: the column divided by
// its float64 norm (zero-padded to a multiple of four rings) and a validity flag, the norm taken by sc_sector_norm - the one
// function that roam_loop_db_add_desc's kernel runs on ready-made descriptors, so that an entry's stored bits depend on its
// descriptor alone.
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
// Selection (loop_select_kernel): one workgroup per query, k <= 32 passes, each the lexicographic minimum of (distance, index)
// above the previous pick, among the indices below max_index with distance <= max_distance.
//
// Peak clouds (roam_loop_db_keep_clouds).  A database that keeps clouds stores, beside each descriptor, the scan's polar peaks in metres:
// the peaks of roam_peaks_record_u8 / roam_peaks_polar_f32 in their azimuth-major order, N of them, of which the entry keeps
// q = 0, step, 2 step, ... with step = max(point_stride, ceil(N / max_points)), as x = fl64(fl64(r res) cos_t[theta]) and y likewise
// with sin_t; the tables come from the host's libm (roam_polar_cloud_table), the device only multiplies.  The peak row kernels of
// peaks.hip leave row_stage / row_count; cloud_gather_kernel, one workgroup per scan, scans the row counts, derives step from the total
// and writes the selected peaks straight to the entry's slot - the int32 peak list is never made.  A lane owns a run of consecutive
// rows and knows the global index of their first peak from the scan, so what is stored depends on the scan alone, not on the batch or
// the chunk.  Verification (roam_loop_db_verify, roam_loop_db_query_verify) runs icp.hip's store kernel on pairs of slots; the
// query form enqueues distance, selection, loop_pairs_kernel (candidates -> pairs and their yaw seeds) and the ICP on one stream.
#include "roam_internal.h"
#include "peaks_common.h"
#include <math.h>
#include <stdlib.h>
#include <limits>
#include <type_traits>

#define SC_THREADS 256
#define SC_QW 4                                  // queries per wave
#define SC_QB (SC_QW * (SC_THREADS / 64))        // queries per workgroup
#define SC_LDS_BYTES 32768                       // the doubled candidate of one phase
#define SC_DB_BYTES ((int64_t)2000 << 20)        // a database, and the scratch of one launch, as in the other batched stages
#define SC_MAX_ROWS 65536
#define CG_THREADS 512                           // cloud_gather_kernel: eight waves, a row per lane up to 512 azimuths

struct roam_loop_db {
    int S = 0, R = 0, Rp = 0, capacity = 0, count = 0;
    float *desc = nullptr;       // capacity x S x R
    double *nrm = nullptr;       // capacity x S x Rp: normalised columns, zero for an invalid sector and in the padding
    int32_t *valid = nullptr;    // capacity x S
    // the peak clouds (roam_loop_db_keep_clouds): cloud_rows = 0 when the database keeps none
    int cloud_rows = 0, max_points = 0, point_stride = 0;
    double res = 0.0;            // metres per range bin
    double *cloud = nullptr;     // capacity x max_points x 2, metres
    int32_t *cloud_n = nullptr, *cloud_peaks = nullptr;      // capacity each: the points stored, the scan's full peak count
    double *trig = nullptr;      // cos(phi_t), t < cloud_rows, then sin(phi_t)
    std::vector<int32_t> h_n, h_peaks;                       // host mirror of the two counts, kept by the blocking entries
};

// image z of a launch: base + (index ? index[z] : z) * image_stride (+ payload_off for u8 records); strides in elements
struct ScSrc {
    const void *base;
    int64_t image_stride, row_stride;
    int32_t payload_off;
    const int32_t *index;
};

// ---------------------------------------------------------------------------------------------------------------- device
// the float64 norm of one sector column of a descriptor, rings ascending
__device__ static double sc_sector_norm(const float *d, int R)
{
    double n2 = 0.0;
    for (int r = 0; r < R; ++r) n2 += (double)d[r] * (double)d[r];
    return sqrt(n2);
}

__device__ static double sc_normalised(float d, double norm) { return norm > 0.0 ? (double)d / norm : 0.0; }

template <bool U8>
__global__ __launch_bounds__(SC_THREADS) void scan_context_kernel(ScSrc src, int rows, int clip, int S, int R, int Rp, double floor_v,
                                                                  int floor_code, float *__restrict__ desc, double *__restrict__ nrm,
                                                                  int32_t *__restrict__ valid)
{
    extern __shared__ __align__(16) unsigned char sc_lds[];
    typedef typename std::conditional<U8, uint32_t, double>::type ColT;
    typedef typename std::conditional<U8, unsigned long long, double>::type SumT;
    double *nv = (double *)sc_lds;                        // the norm of the sector's descriptor column
    ColT *col = (ColT *)(nv + 1);                         // clip column sums of this sector
    float *dv = (float *)(col + clip);                    // R: the descriptor column
    const int64_t z = blockIdx.x;
    const int s = blockIdx.y;
    const int y0 = (int)((int64_t)s * rows / S), y1 = (int)((int64_t)(s + 1) * rows / S);
    const int64_t img = src.index ? src.index[z] : z;
    for (int c = threadIdx.x; c < clip; c += SC_THREADS) {
        ColT a = 0;
        if constexpr (U8) {
            const uint8_t *p = (const uint8_t *)src.base + img * src.image_stride + src.payload_off + c;
            for (int y = y0; y < y1; ++y) a += (ColT)max((int)p[y * src.row_stride] - floor_code, 0);
        } else {
            const float *p = (const float *)src.base + img * src.image_stride + c;
            for (int y = y0; y < y1; ++y) a += (ColT)fmax((double)p[y * src.row_stride] - floor_v, 0.0);
        }
        col[c] = a;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < R; r += SC_THREADS / 64) {
        const int c0 = (int)((int64_t)r * clip / R), c1 = (int)((int64_t)(r + 1) * clip / R);
        SumT sum = 0;
        for (int c = c0 + lane; c < c1; c += 64) sum += (SumT)col[c];
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == 0) {
            const double cells = (double)((int64_t)(y1 - y0) * (c1 - c0));
            dv[r] = U8 ? (float)((double)sum / (255.0 * cells)) : (float)((double)sum / cells);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) nv[0] = sc_sector_norm(dv, R);
    __syncthreads();
    const double norm = nv[0];
    const int64_t row = z * S + s;
    for (int r = threadIdx.x; r < Rp; r += SC_THREADS) {
        if (r < R) desc[row * R + r] = dv[r];
        if (nrm) nrm[row * Rp + r] = r < R ? sc_normalised(dv[r], norm) : 0.0;
    }
    if (threadIdx.x == 0 && valid) valid[row] = norm > 0.0;
}

// ready-made descriptors: one lane per (entry, sector)
__global__ __launch_bounds__(SC_THREADS) void scan_context_norm_kernel(const float *__restrict__ desc, int64_t n_rows, int R, int Rp,
                                                                       double *__restrict__ nrm, int32_t *__restrict__ valid)
{
    const int64_t row = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (row >= n_rows) return;
    const float *d = desc + row * R;
    const double norm = sc_sector_norm(d, R);
    for (int r = 0; r < Rp; ++r) nrm[row * Rp + r] = r < R ? sc_normalised(d[r], norm) : 0.0;
    valid[row] = norm > 0.0;
}

// rings of one LDS phase: all of them (padded to a multiple of four) when the doubled candidate fits, else the largest multiple of four
__host__ __device__ static int sc_phase_rings(int S, int Rp)
{
    const int fit = (SC_LDS_BYTES / (8 * (2 * S + 1))) & ~3;
    return Rp < fit ? Rp : fit;
}

// dist / shift: nq x count, row q = query qidx[q].  qmax (optional): candidate j is computed for query q only when j < qmax[q]
template <int TK>
__global__ __launch_bounds__(SC_THREADS) void loop_distance_kernel(const double *__restrict__ nrm, const int32_t *__restrict__ valid,
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
                    const double *qp = nrm + ((int64_t)qi[i] * S + s) * Rp + r0 + r;      // wave-uniform: scalar loads
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
        for (int i = 0; i < SC_QW; ++i) vq[i] = valid[(int64_t)qi[i] * S + s];
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

// the stored cloud of scan b of the launch (entry first + b, the pointers already moved there) from the row kernel's staging: see the
// head of the file.  A lane takes the rows [lo, hi) and walks their peaks with the global index q = off + j
__global__ __launch_bounds__(CG_THREADS) void cloud_gather_kernel(const uint16_t *__restrict__ row_stage, int stage_cap,
                                                                  const int32_t *__restrict__ row_count, int rows, const double *__restrict__ trig,
                                                                  double res, int max_points, int point_stride, double *__restrict__ cloud,
                                                                  int32_t *__restrict__ cloud_n, int32_t *__restrict__ cloud_peaks)
{
    __shared__ int scan_sh[8];
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const int ritems = (rows + CG_THREADS - 1) / CG_THREADS;
    const int lo = min(t * ritems, rows), hi = min(lo + ritems, rows);
    const int32_t *rc = row_count + b * rows;
    int c = 0;
    for (int r = lo; r < hi; ++r) c += min(rc[r], stage_cap);
    int total;
    int off = block_excl_scan(c, scan_sh, &total);
    const int fit = (total + max_points - 1) / max_points;
    const int step = fit > point_stride ? fit : point_stride;
    double *out = cloud + 2 * b * max_points;
    for (int r = lo; r < hi; ++r) {
        const int n = min(rc[r], stage_cap);
        const uint16_t *sr = row_stage + (b * rows + r) * stage_cap;
        const double ct = trig[r], st = trig[rows + r];
        const int rem = off % step;
        for (int j = rem ? step - rem : 0; j < n; j += step) {
            const int slot = (off + j) / step;             // < ceil(total / step) <= max_points
            const double rho = (double)sr[j] * res;
            out[2 * slot] = rho * ct;
            out[2 * slot + 1] = rho * st;
        }
        off += n;
    }
    if (t == 0) {
        cloud_n[b] = (total + step - 1) / step;
        cloud_peaks[b] = total;
    }
}

// query_verify: slot (q, s) of the selection -> pair q k + s: the query's cloud onto the candidate's (-1: an empty pair) from
// (yaw, 0, 0), yaw = 2 pi shift / S in (-pi, pi] by LoopClosure._yaw's operations
__global__ __launch_bounds__(SC_THREADS) void loop_pairs_kernel(const int32_t *__restrict__ qidx, const int32_t *__restrict__ ci,
                                                                const int32_t *__restrict__ cs, int n_pairs, int k, int S,
                                                                int32_t *__restrict__ src_index, int32_t *__restrict__ dst_index,
                                                                double *__restrict__ init)
{
    const int p = blockIdx.x * SC_THREADS + threadIdx.x;
    if (p >= n_pairs) return;
    src_index[p] = qidx[p / k];
    dst_index[p] = ci[p];
    const double a = (6.283185307179586 * (double)cs[p]) / (double)S;
    init[3 * (int64_t)p] = a > 3.141592653589793 ? a - 6.283185307179586 : a;
    init[3 * (int64_t)p + 1] = 0.0;
    init[3 * (int64_t)p + 2] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- host
// the launch scratch: SC_DB_BYTES, or the tests' smaller figure from ROAM_LOOP_CHUNK_BYTES (read per call).  It only decides where a
// batch of images or queries is cut
static int64_t sc_chunk_limit()
{
    int64_t limit = SC_DB_BYTES;
    if (const char *ce = getenv("ROAM_LOOP_CHUNK_BYTES")) {
        const long long c = atoll(ce);
        if (c >= 1 && c < limit) limit = c;
    }
    return limit;
}

// events around `reps` launches on st, after two warm ones -> milliseconds per launch
template <typename F>
static int32_t sc_time_launches(roam_ctx *ctx, hipStream_t st, int reps, float *ms_per_rep, F launch)
{
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) HIP_TRY(ctx, launch());
    HIP_TRY(ctx, hipEventRecord(e0, st));
    for (int i = 0; i < reps; ++i) HIP_TRY(ctx, launch());
    HIP_TRY(ctx, hipEventRecord(e1, st));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    *ms_per_rep = ms / reps;
    HIP_TRY(ctx, hipEventDestroy(e0));
    HIP_TRY(ctx, hipEventDestroy(e1));
    return ROAM_OK;
}

#define SC_FAIL(err, cap, ...)                              \
    do {                                                    \
        if (err) snprintf(err, cap, __VA_ARGS__);           \
        return ROAM_E_ARG;                                  \
    } while (0)

// the checks of the geometry, shared by every describing entry -> the clip
static int32_t sc_check_geometry(char *err, size_t cap, int32_t rows, int32_t cols, int32_t clip_px, int32_t sectors, int32_t rings, int *clip_out)
{
    if (sectors < 2 || sectors > ROAM_SCAN_CONTEXT_MAX_SECTORS) SC_FAIL(err, cap, "scan context: sectors in [2, %d], not %d", ROAM_SCAN_CONTEXT_MAX_SECTORS, sectors);
    if (rings < 1 || rings > ROAM_SCAN_CONTEXT_MAX_RINGS) SC_FAIL(err, cap, "scan context: rings in [1, %d], not %d", ROAM_SCAN_CONTEXT_MAX_RINGS, rings);
    if (rows < sectors || rows > SC_MAX_ROWS) SC_FAIL(err, cap, "scan context: rows in [sectors = %d, %d], not %d", sectors, SC_MAX_ROWS, rows);
    if (cols < 1) SC_FAIL(err, cap, "scan context: cols >= 1, not %d", cols);
    const int clip = (clip_px > 0 && clip_px < cols) ? clip_px : cols;
    if (clip < rings || clip > ROAM_SCAN_CONTEXT_MAX_CLIP)
        SC_FAIL(err, cap, "scan context: clip_px (the range bins kept) in [rings = %d, %d], not %d", rings, ROAM_SCAN_CONTEXT_MAX_CLIP, clip);
    *clip_out = clip;
    return ROAM_OK;
}

extern "C" int32_t roam_scan_context_plan(int32_t rows, int32_t cols, int32_t clip_px, int32_t sectors, int32_t rings, int32_t *row_edges,
                                          int32_t *col_edges)
{
    int clip;
    const int32_t rc = sc_check_geometry(nullptr, 0, rows, cols, clip_px, sectors, rings, &clip);
    if (rc != ROAM_OK) return rc;
    for (int s = 0; s <= sectors && row_edges; ++s) row_edges[s] = (int32_t)((int64_t)s * rows / sectors);
    for (int r = 0; r <= rings && col_edges; ++r) col_edges[r] = (int32_t)((int64_t)r * clip / rings);
    return ROAM_OK;
}

static size_t sc_describe_lds(bool u8, int clip, int R) { return sizeof(double) + (size_t)clip * (u8 ? 4 : 8) + sizeof(float) * R; }

// n images -> rows of desc / nrm / valid starting at entry `first` (nrm / valid may be null)
static hipError_t sc_launch_describe(hipStream_t st, bool u8, const ScSrc &src, int n, int rows, int clip, int S, int R, double floor_v,
                                     int floor_code, float *desc, double *nrm, int32_t *valid, int64_t first)
{
    const int Rp = (R + 3) & ~3;
    float *d = desc + first * S * R;
    double *nn = nrm ? nrm + first * S * Rp : nullptr;
    int32_t *vv = valid ? valid + first * S : nullptr;
    if (u8)
        hipLaunchKernelGGL(scan_context_kernel<true>, dim3(n, S), dim3(SC_THREADS), sc_describe_lds(true, clip, R), st, src, rows, clip, S, R, Rp,
                           floor_v, floor_code, d, nn, vv);
    else
        hipLaunchKernelGGL(scan_context_kernel<false>, dim3(n, S), dim3(SC_THREADS), sc_describe_lds(false, clip, R), st, src, rows, clip, S, R, Rp,
                           floor_v, floor_code, d, nn, vv);
    return hipGetLastError();
}

// ---- the peak clouds
// bytes of row staging one scan of `cols` range bins takes (row_stage + row_count)
static int64_t sc_stage_bytes(int rows, int cols) { return (int64_t)rows * ((cols + 1) / 2) * sizeof(uint16_t) + (int64_t)rows * sizeof(int32_t); }

static hipError_t sc_launch_cloud_gather(hipStream_t st, const roam_loop_db *db, int nb, const uint16_t *stage, int stage_cap, const int32_t *rcount,
                                         int64_t first)
{
    hipLaunchKernelGGL(cloud_gather_kernel, dim3(nb), dim3(CG_THREADS), 0, st, stage, stage_cap, rcount, db->cloud_rows, db->trig, db->res,
                       db->max_points, db->point_stride, db->cloud + 2 * first * db->max_points, db->cloud_n + first, db->cloud_peaks + first);
    return hipGetLastError();
}

// the staging of nb scans (taken from the scratch slots S_TMP0 / S_TMP1, which no enqueued engine step reads: a step owns its buffers)
static int32_t sc_cloud_stage(roam_ctx *ctx, int rows, int cols, int nb, uint16_t **stage, int32_t **rcount)
{
    const int stage_cap = (cols + 1) / 2;
    *stage = (uint16_t *)roam_scratch(ctx, S_TMP0, sizeof(uint16_t) * (size_t)nb * rows * stage_cap);
    *rcount = (int32_t *)roam_scratch(ctx, S_TMP1, sizeof(int32_t) * (size_t)nb * rows);
    return *stage && *rcount ? ROAM_OK : ROAM_E_HIP;
}

// the clouds of the nb scans of `ps` (cols range bins each) -> the entries from `first` on; enqueued, not awaited
static int32_t sc_build_clouds(roam_ctx *ctx, const roam_loop_db *db, const PeakSrc &ps, int nb, int cols, int64_t first)
{
    uint16_t *stage;
    int32_t *rcount;
    const int32_t rc = sc_cloud_stage(ctx, db->cloud_rows, cols, nb, &stage, &rcount);
    if (rc != ROAM_OK) return rc;
    HIP_TRY(ctx, launch_peaks_rows(ctx->stream, ps, nb, db->cloud_rows, cols, stage, (cols + 1) / 2, rcount));
    HIP_TRY(ctx, sc_launch_cloud_gather(ctx->stream, db, nb, stage, (cols + 1) / 2, rcount, first));
    return ROAM_OK;
}

// what an add to a cloud-keeping database refuses beyond the descriptor's checks
static int32_t sc_check_cloud_add(roam_ctx *ctx, const roam_loop_db *db, int rows, int cols)
{
    if (rows != db->cloud_rows) {
        ROAM_SET_ERR(ctx, "loop db: rows = %d, but the database keeps clouds of %d azimuths", rows, db->cloud_rows);
        return ROAM_E_ARG;
    }
    if (cols > ROAM_MAX_COLS) { ROAM_SET_ERR(ctx, "loop db: cols <= %d for a database that keeps clouds, not %d", ROAM_MAX_COLS, cols); return ROAM_E_ARG; }
    return ROAM_OK;
}

// the end of a blocking add of n entries from `first` on: their counts to the host mirror; waits for the stream
static int32_t sc_mirror_counts(roam_ctx *ctx, roam_loop_db *db, int64_t first, int n)
{
    HIP_TRY(ctx, hipMemcpyAsync(db->h_n.data() + first, db->cloud_n + first, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(db->h_peaks.data() + first, db->cloud_peaks + first, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

// host float32 images in chunks under the scratch limit: upload the clipped columns tightly, describe into desc (+ nrm, valid) from
// entry `first` on
// cloud_db (optional, a database that keeps clouds; cols = the images' full width): all the columns are uploaded, and the images'
// peak clouds go to the entries from `first` on as well
static int32_t sc_describe_host_f32(roam_ctx *ctx, const float *polar, int n, int rows, int64_t row_stride, int64_t image_stride, int clip,
                                    int S, int R, double floor_v, float *desc, double *nrm, int32_t *valid, int64_t first,
                                    const roam_loop_db *cloud_db = nullptr, int cols = 0)
{
    const hipStream_t st = ctx->stream;
    const int width = cloud_db ? cols : clip;
    const int64_t per = (int64_t)sizeof(float) * rows * width + (cloud_db ? sc_stage_bytes(rows, cols) : 0);
    int64_t chunk = sc_chunk_limit() / per;
    if (chunk < 1) chunk = 1;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int nb = (int)(n - i0 < chunk ? n - i0 : chunk);
        float *d_in = (float *)roam_scratch(ctx, S_IN0, sizeof(float) * (size_t)rows * width * nb);
        if (!d_in) return ROAM_E_HIP;
        HIP_TRY(ctx, roam_upload_packed_f32(st, d_in, polar + i0 * image_stride, nb, width, rows, row_stride, image_stride));
        const ScSrc src = {d_in, (int64_t)rows * width, width, 0, nullptr};
        HIP_TRY(ctx, sc_launch_describe(st, false, src, nb, rows, clip, S, R, floor_v, 0, desc, nrm, valid, first + i0));
        if (cloud_db) {
            const PeakSrc ps = {d_in, (int64_t)rows * width, width, 0, 0, nullptr};
            const int32_t rc = sc_build_clouds(ctx, cloud_db, ps, nb, cols, first + i0);
            if (rc != ROAM_OK) return rc;
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));           // the next chunk reuses the upload buffer
    }
    return ROAM_OK;
}

static int32_t sc_check_f32_args(roam_ctx *ctx, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride,
                                 int64_t image_stride, int32_t clip_px, int32_t sectors, int32_t rings, double floor, int *clip)
{
    if (!polar) { ROAM_SET_ERR(ctx, "scan context: polar is null"); return ROAM_E_ARG; }
    if (n < 1) { ROAM_SET_ERR(ctx, "scan context: n >= 1 images, not %d", n); return ROAM_E_ARG; }
    const int32_t rc = sc_check_geometry(ctx->err, sizeof(ctx->err), rows, cols, clip_px, sectors, rings, clip);
    if (rc != ROAM_OK) return rc;
    if (row_stride < cols) { ROAM_SET_ERR(ctx, "scan context: row_stride %lld below cols %d", (long long)row_stride, cols); return ROAM_E_ARG; }
    if (n > 1 && image_stride < (int64_t)(rows - 1) * row_stride + cols) {
        ROAM_SET_ERR(ctx, "scan context: image_stride %lld below the extent of an image", (long long)image_stride);
        return ROAM_E_ARG;
    }
    if (!(std::isfinite(floor) && floor >= 0.0)) { ROAM_SET_ERR(ctx, "scan context: floor finite and >= 0, not %g", floor); return ROAM_E_ARG; }
    return ROAM_OK;
}

extern "C" int32_t roam_scan_context_f32(roam_ctx *ctx, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride,
                                         int64_t image_stride, int32_t clip_px, int32_t sectors, int32_t rings, double floor, float *desc_out)
{
    if (!ctx) return ROAM_E_ARG;
    int clip;
    const int32_t rc = sc_check_f32_args(ctx, polar, n, rows, cols, row_stride, image_stride, clip_px, sectors, rings, floor, &clip);
    if (rc != ROAM_OK) return rc;
    if (!desc_out) { ROAM_SET_ERR(ctx, "scan context: desc_out is null"); return ROAM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float) * (size_t)n * sectors * rings;
    float *d_desc = (float *)roam_scratch(ctx, S_OUT0, bytes);
    if (!d_desc) return ROAM_E_HIP;
    const int32_t rd = sc_describe_host_f32(ctx, polar, n, rows, row_stride, image_stride, clip, sectors, rings, floor, d_desc, nullptr, nullptr, 0);
    if (rd != ROAM_OK) return rd;
    HIP_TRY(ctx, hipMemcpyAsync(desc_out, d_desc, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

static void sc_db_free(roam_loop_db *db)
{
    if (db->desc) (void)hipFree(db->desc);
    if (db->nrm) (void)hipFree(db->nrm);
    if (db->valid) (void)hipFree(db->valid);
    if (db->cloud) (void)hipFree(db->cloud);
    if (db->cloud_n) (void)hipFree(db->cloud_n);
    if (db->cloud_peaks) (void)hipFree(db->cloud_peaks);
    if (db->trig) (void)hipFree(db->trig);
    delete db;
}

extern "C" int32_t roam_loop_db_create(roam_ctx *ctx, int32_t capacity, int32_t sectors, int32_t rings, roam_loop_db **out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!out) { ROAM_SET_ERR(ctx, "loop db: out is null"); return ROAM_E_ARG; }
    if (sectors < 2 || sectors > ROAM_SCAN_CONTEXT_MAX_SECTORS || rings < 1 || rings > ROAM_SCAN_CONTEXT_MAX_RINGS) {
        ROAM_SET_ERR(ctx, "loop db: sectors in [2, %d] and rings in [1, %d], not %d and %d", ROAM_SCAN_CONTEXT_MAX_SECTORS,
                     ROAM_SCAN_CONTEXT_MAX_RINGS, sectors, rings);
        return ROAM_E_ARG;
    }
    const int Rp = (rings + 3) & ~3;
    const int64_t per = (int64_t)sectors * (sizeof(float) * rings + sizeof(double) * Rp + sizeof(int32_t));
    if (capacity < 1 || capacity > SC_DB_BYTES / per) {
        ROAM_SET_ERR(ctx, "loop db: capacity in [1, %lld] (%lld bytes per entry, %lld in all), not %d", (long long)(SC_DB_BYTES / per),
                     (long long)per, (long long)SC_DB_BYTES, capacity);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    roam_loop_db *db = new roam_loop_db;
    db->S = sectors; db->R = rings; db->Rp = Rp; db->capacity = capacity;
    const size_t rows = (size_t)capacity * sectors;
    if (hipMalloc(&db->desc, sizeof(float) * rows * rings) != hipSuccess || hipMalloc(&db->nrm, sizeof(double) * rows * Rp) != hipSuccess ||
        hipMalloc(&db->valid, sizeof(int32_t) * rows) != hipSuccess) {
        ROAM_SET_ERR(ctx, "loop db: hipMalloc of %lld bytes failed", (long long)(per * capacity));
        sc_db_free(db);
        return ROAM_E_HIP;
    }
    *out = db;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_destroy(roam_ctx *ctx, roam_loop_db *db)
{
    if (!ctx || !db) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // nothing enqueued reads it any more
    sc_db_free(db);
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_count(const roam_loop_db *db, int32_t *count)
{
    if (!db || !count) return ROAM_E_ARG;
    *count = db->count;
    return ROAM_OK;
}

static int32_t sc_check_room(roam_ctx *ctx, const roam_loop_db *db, int32_t n)
{
    if (n < 1) { ROAM_SET_ERR(ctx, "loop db: n >= 1 entries, not %d", n); return ROAM_E_ARG; }
    if (n > db->capacity - db->count) {
        ROAM_SET_ERR(ctx, "loop db: %d entries do not fit (%d of %d used)", n, db->count, db->capacity);
        return ROAM_E_CAPACITY;
    }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_add_f32(roam_ctx *ctx, roam_loop_db *db, const float *polar, int32_t n, int32_t rows, int32_t cols,
                                        int64_t row_stride, int64_t image_stride, int32_t clip_px, double floor, int32_t *first_index_out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    int clip;
    int32_t rc = sc_check_f32_args(ctx, polar, n, rows, cols, row_stride, image_stride, clip_px, db->S, db->R, floor, &clip);
    if (rc != ROAM_OK) return rc;
    if (db->cloud_rows && (rc = sc_check_cloud_add(ctx, db, rows, cols)) != ROAM_OK) return rc;
    if ((rc = sc_check_room(ctx, db, n)) != ROAM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = sc_describe_host_f32(ctx, polar, n, rows, row_stride, image_stride, clip, db->S, db->R, floor, db->desc, db->nrm, db->valid, db->count,
                              db->cloud_rows ? db : nullptr, cols);
    if (rc != ROAM_OK) return rc;
    if (db->cloud_rows && (rc = sc_mirror_counts(ctx, db, db->count, n)) != ROAM_OK) return rc;
    if (first_index_out) *first_index_out = db->count;
    db->count += n;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_add_desc(roam_ctx *ctx, roam_loop_db *db, const float *desc, int32_t n, int32_t *first_index_out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db || !desc) { ROAM_SET_ERR(ctx, "loop db: %s is null", db ? "desc" : "db"); return ROAM_E_ARG; }
    int32_t rc = sc_check_room(ctx, db, n);
    if (rc != ROAM_OK) return rc;
    const int64_t per = (int64_t)db->S * db->R;
    for (int64_t q = 0; q < per * n; ++q)
        if (!std::isfinite(desc[q])) {
            ROAM_SET_ERR(ctx, "loop db: desc entry %lld, element %lld is not finite", (long long)(q / per), (long long)(q % per));
            return ROAM_E_ARG;
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(db->desc + db->count * per, desc, sizeof(float) * per * n, hipMemcpyHostToDevice, st));
    const int64_t n_rows = (int64_t)n * db->S;
    hipLaunchKernelGGL(scan_context_norm_kernel, dim3((unsigned)((n_rows + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, st,
                       db->desc + db->count * per, n_rows, db->R, db->Rp, db->nrm + (int64_t)db->count * db->S * db->Rp,
                       db->valid + (int64_t)db->count * db->S);
    HIP_TRY(ctx, hipGetLastError());
    if (db->cloud_rows) {                                 // ready-made descriptors bring no scan: empty clouds (roam_loop_db_set_cloud fills them)
        HIP_TRY(ctx, hipMemsetAsync(db->cloud_n + db->count, 0, sizeof(int32_t) * (size_t)n, st));
        HIP_TRY(ctx, hipMemsetAsync(db->cloud_peaks + db->count, 0, sizeof(int32_t) * (size_t)n, st));
        for (int i = 0; i < n; ++i) db->h_n[db->count + i] = db->h_peaks[db->count + i] = 0;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (first_index_out) *first_index_out = db->count;
    db->count += n;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_get(roam_ctx *ctx, roam_loop_db *db, int32_t first, int32_t n, float *desc_out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db || !desc_out) { ROAM_SET_ERR(ctx, "loop db: %s is null", db ? "desc_out" : "db"); return ROAM_E_ARG; }
    if (first < 0 || n < 1 || n > db->count - first) {
        ROAM_SET_ERR(ctx, "loop db: entries [%d, %d + %d) outside the %d stored", first, first, n, db->count);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t per = (int64_t)db->S * db->R;
    HIP_TRY(ctx, hipMemcpyAsync(desc_out, db->desc + first * per, sizeof(float) * per * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

// engine_lanes.hip's roam_engine_loop_db_add after its own checks (the engine, the pool indices): n resident u8 records of `cols` range bins.
// after (optional): an event the stream waits for once the arguments have passed - the pool's pending uploads.  time_ms (optional):
// instead of appending, time_reps launches of the describing kernel into the free entries between two events, two warm ones first
int32_t roam_loop_db_add_records(roam_ctx *ctx, roam_loop_db *db, const uint8_t *pool, int64_t rec_bytes, int64_t row_stride, int32_t payload_off,
                                 int32_t rows, int32_t cols, int32_t n, const int32_t *pool_idx, int32_t clip_px, int32_t floor_code,
                                 int32_t *first_index_out, hipEvent_t after, int32_t time_reps, float *time_ms, float *cloud_ms)
{
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    int clip;
    int32_t rc = sc_check_geometry(ctx->err, sizeof(ctx->err), rows, cols, clip_px, db->S, db->R, &clip);
    if (rc != ROAM_OK) return rc;
    if (floor_code < 0 || floor_code > 254) { ROAM_SET_ERR(ctx, "loop db: floor_code in [0, 254], not %d", floor_code); return ROAM_E_ARG; }
    if (cloud_ms && !db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db timing: db keeps no clouds"); return ROAM_E_ARG; }
    if (db->cloud_rows && (rc = sc_check_cloud_add(ctx, db, rows, cols)) != ROAM_OK) return rc;
    if ((rc = sc_check_room(ctx, db, n)) != ROAM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    if (after) HIP_TRY(ctx, hipStreamWaitEvent(st, after, 0));
    int32_t *d_idx = (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * (size_t)n);
    if (!d_idx) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, pool_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    const ScSrc src = {pool, rec_bytes, row_stride, payload_off, d_idx};
    if (time_ms) {                                        // roam_engine_time_loop_describe: the launch alone, nothing is appended
        if (time_reps < 1) { ROAM_SET_ERR(ctx, "loop db timing: reps >= 1, not %d", time_reps); return ROAM_E_ARG; }
        return sc_time_launches(ctx, st, time_reps, time_ms, [&] {
            return sc_launch_describe(st, true, src, n, rows, clip, db->S, db->R, 0.0, floor_code, db->desc, db->nrm, db->valid, db->count);
        });
    }
    if (cloud_ms) {                                       // roam_engine_time_loop_cloud: the two kernels of the cloud build, each alone
        if (time_reps < 1) { ROAM_SET_ERR(ctx, "loop db timing: reps >= 1, not %d", time_reps); return ROAM_E_ARG; }
        if (n * sc_stage_bytes(rows, cols) > SC_DB_BYTES) { ROAM_SET_ERR(ctx, "loop db timing: %d records do not fit one launch", n); return ROAM_E_ARG; }
        uint16_t *stage;
        int32_t *rcount;
        if ((rc = sc_cloud_stage(ctx, rows, cols, n, &stage, &rcount)) != ROAM_OK) return rc;
        const PeakSrc ps = {pool, rec_bytes, row_stride, payload_off, 1, d_idx};
        rc = sc_time_launches(ctx, st, time_reps, cloud_ms, [&] { return launch_peaks_rows(st, ps, n, rows, cols, stage, (cols + 1) / 2, rcount); });
        if (rc != ROAM_OK) return rc;
        return sc_time_launches(ctx, st, time_reps, cloud_ms + 1,
                                [&] { return sc_launch_cloud_gather(st, db, n, stage, (cols + 1) / 2, rcount, db->count); });
    }
    HIP_TRY(ctx, sc_launch_describe(st, true, src, n, rows, clip, db->S, db->R, 0.0, floor_code, db->desc, db->nrm, db->valid, db->count));
    if (db->cloud_rows) {                                 // in chunks that bound the staging; what is stored does not depend on the cut
        int64_t chunk = sc_chunk_limit() / sc_stage_bytes(rows, cols);
        if (chunk < 1) chunk = 1;
        for (int64_t i0 = 0; i0 < n; i0 += chunk) {
            const int nb = (int)(n - i0 < chunk ? n - i0 : chunk);
            const PeakSrc ps = {pool, rec_bytes, row_stride, payload_off, 1, d_idx + i0};
            if ((rc = sc_build_clouds(ctx, db, ps, nb, cols, db->count + i0)) != ROAM_OK) return rc;
        }
        if ((rc = sc_mirror_counts(ctx, db, db->count, n)) != ROAM_OK) return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));               // the index list is the caller's
    if (first_index_out) *first_index_out = db->count;
    db->count += n;
    return ROAM_OK;
}

// the distance kernel for nq queries (d_q: their indices, d_mask: optional max_index) against every entry, and the selection
static hipError_t sc_launch_distance(hipStream_t st, const roam_loop_db *db, const int32_t *d_q, const int32_t *d_mask, int nq, double *d_dist,
                                     int32_t *d_shift)
{
    const int count = db->count, S = db->S, Rp = db->Rp;
    const int RL = sc_phase_rings(S, Rp);
    const size_t lds = sizeof(double) * (size_t)RL * (2 * S + 1) + sizeof(int32_t) * 2 * S;
    const dim3 grid(count, (nq + SC_QB - 1) / SC_QB);
    switch ((S + 63) / 64) {
    case 1: hipLaunchKernelGGL(loop_distance_kernel<1>, grid, dim3(SC_THREADS), lds, st, db->nrm, db->valid, d_q, d_mask, nq, count, S, Rp, RL, d_dist, d_shift); break;
    case 2: hipLaunchKernelGGL(loop_distance_kernel<2>, grid, dim3(SC_THREADS), lds, st, db->nrm, db->valid, d_q, d_mask, nq, count, S, Rp, RL, d_dist, d_shift); break;
    case 3: hipLaunchKernelGGL(loop_distance_kernel<3>, grid, dim3(SC_THREADS), lds, st, db->nrm, db->valid, d_q, d_mask, nq, count, S, Rp, RL, d_dist, d_shift); break;
    default: hipLaunchKernelGGL(loop_distance_kernel<4>, grid, dim3(SC_THREADS), lds, st, db->nrm, db->valid, d_q, d_mask, nq, count, S, Rp, RL, d_dist, d_shift); break;
    }
    return hipGetLastError();
}

static hipError_t sc_launch_select(hipStream_t st, const roam_loop_db *db, const int32_t *d_qmax, int nq, int k, double max_distance,
                                   const double *d_dist, const int32_t *d_shift, int32_t *d_ci, double *d_cd, int32_t *d_cs)
{
    hipLaunchKernelGGL(loop_select_kernel, dim3(nq), dim3(SC_THREADS), 0, st, d_dist, d_shift, d_qmax, db->count, k, max_distance, d_ci, d_cd, d_cs);
    return hipGetLastError();
}

static int32_t sc_check_query(roam_ctx *ctx, const roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                              int32_t k, double max_distance)
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

extern "C" int32_t roam_loop_db_query(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                      int32_t k, double max_distance, int32_t *cand_index, double *cand_dist, int32_t *cand_shift,
                                      double *dist_full, int32_t *shift_full)
{
    if (!ctx) return ROAM_E_ARG;
    const int32_t rc = sc_check_query(ctx, db, n_query, query_index, max_index, k, max_distance);
    if (rc != ROAM_OK) return rc;
    if (!cand_index || !cand_dist || !cand_shift) {
        ROAM_SET_ERR(ctx, "loop db query: %s is null", !cand_index ? "cand_index" : !cand_dist ? "cand_dist" : "cand_shift");
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int count = db->count;
    const bool full = dist_full || shift_full;
    int64_t chunk = sc_chunk_limit() / ((int64_t)(sizeof(double) + sizeof(int32_t)) * count);
    if (chunk < 1) chunk = 1;
    if (chunk > 65535 * SC_QB) chunk = 65535 * SC_QB;     // the grid's y extent
    std::vector<int32_t> qm((size_t)n_query);
    for (int q = 0; q < n_query; ++q) qm[q] = max_index[q] < 0 ? 0 : max_index[q] > count ? count : max_index[q];
    for (int64_t q0 = 0; q0 < n_query; q0 += chunk) {
        const int nq = (int)(n_query - q0 < chunk ? n_query - q0 : chunk);
        double *d_dist = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * (size_t)nq * count);
        int32_t *d_shift = (int32_t *)roam_scratch(ctx, S_TMP1, sizeof(int32_t) * (size_t)nq * count);
        int32_t *d_q = (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * 2 * (size_t)nq);
        int32_t *d_ci = (int32_t *)roam_scratch(ctx, S_OUT0, sizeof(int32_t) * (size_t)nq * k);
        double *d_cd = (double *)roam_scratch(ctx, S_OUT1, sizeof(double) * (size_t)nq * k);
        int32_t *d_cs = (int32_t *)roam_scratch(ctx, S_OUT2, sizeof(int32_t) * (size_t)nq * k);
        if (!d_dist || !d_shift || !d_q || !d_ci || !d_cd || !d_cs) return ROAM_E_HIP;
        HIP_TRY(ctx, hipMemcpyAsync(d_q, query_index + q0, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_q + nq, qm.data() + q0, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, sc_launch_distance(st, db, d_q, full ? nullptr : d_q + nq, nq, d_dist, d_shift));      // the full outputs want every pair
        HIP_TRY(ctx, sc_launch_select(st, db, d_q + nq, nq, k, max_distance, d_dist, d_shift, d_ci, d_cd, d_cs));
        HIP_TRY(ctx, hipMemcpyAsync(cand_index + q0 * k, d_ci, sizeof(int32_t) * (size_t)nq * k, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(cand_dist + q0 * k, d_cd, sizeof(double) * (size_t)nq * k, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(cand_shift + q0 * k, d_cs, sizeof(int32_t) * (size_t)nq * k, hipMemcpyDeviceToHost, st));
        if (dist_full) HIP_TRY(ctx, hipMemcpyAsync(dist_full + q0 * count, d_dist, sizeof(double) * (size_t)nq * count, hipMemcpyDeviceToHost, st));
        if (shift_full) HIP_TRY(ctx, hipMemcpyAsync(shift_full + q0 * count, d_shift, sizeof(int32_t) * (size_t)nq * count, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return ROAM_OK;
}

extern "C" int32_t roam_time_loop_db_query(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                           int32_t k, double max_distance, int32_t reps, float *distance_ms, float *select_ms)
{
    if (!ctx) return ROAM_E_ARG;
    int32_t rc = sc_check_query(ctx, db, n_query, query_index, max_index, k, max_distance);
    if (rc != ROAM_OK) return rc;
    ARG_CHECK(ctx, reps >= 1 && distance_ms && select_ms);
    const int count = db->count;
    if ((int64_t)n_query * count * (int64_t)(sizeof(double) + sizeof(int32_t)) > SC_DB_BYTES || n_query > 65535 * SC_QB) {
        ROAM_SET_ERR(ctx, "loop db timing: %d queries against %d entries do not fit one launch", n_query, count);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    std::vector<int32_t> qm((size_t)n_query);
    for (int q = 0; q < n_query; ++q) qm[q] = max_index[q] < 0 ? 0 : max_index[q] > count ? count : max_index[q];
    double *d_dist = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * (size_t)n_query * count);
    int32_t *d_shift = (int32_t *)roam_scratch(ctx, S_TMP1, sizeof(int32_t) * (size_t)n_query * count);
    int32_t *d_q = (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * 2 * (size_t)n_query);
    int32_t *d_ci = (int32_t *)roam_scratch(ctx, S_OUT0, sizeof(int32_t) * (size_t)n_query * k);
    double *d_cd = (double *)roam_scratch(ctx, S_OUT1, sizeof(double) * (size_t)n_query * k);
    int32_t *d_cs = (int32_t *)roam_scratch(ctx, S_OUT2, sizeof(int32_t) * (size_t)n_query * k);
    if (!d_dist || !d_shift || !d_q || !d_ci || !d_cd || !d_cs) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(d_q, query_index, sizeof(int32_t) * (size_t)n_query, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_q + n_query, qm.data(), sizeof(int32_t) * (size_t)n_query, hipMemcpyHostToDevice, st));
    rc = sc_time_launches(ctx, st, reps, distance_ms, [&] { return sc_launch_distance(st, db, d_q, d_q + n_query, n_query, d_dist, d_shift); });
    if (rc != ROAM_OK) return rc;
    return sc_time_launches(ctx, st, reps, select_ms,
                            [&] { return sc_launch_select(st, db, d_q + n_query, n_query, k, max_distance, d_dist, d_shift, d_ci, d_cd, d_cs); });
}

// ---------------------------------------------------------------------------------------------------------------- the cloud store
extern "C" int32_t roam_polar_cloud_table(int32_t rows, double *cos_out, double *sin_out)
{
    if (rows < 1 || rows > SC_MAX_ROWS || !cos_out || !sin_out) return ROAM_E_ARG;
    for (int t = 0; t < rows; ++t) {
        const double phi = (2.0 * M_PI * (double)t) / (double)rows;
        cos_out[t] = cos(phi);
        sin_out[t] = sin(phi);
    }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_keep_clouds(roam_ctx *ctx, roam_loop_db *db, int32_t rows, int32_t max_points, int32_t point_stride,
                                            double range_resolution_m)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    if (db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db: db keeps clouds already"); return ROAM_E_ARG; }
    if (db->count) { ROAM_SET_ERR(ctx, "loop db: keep_clouds wants an empty db, this one holds %d entries", db->count); return ROAM_E_ARG; }
    if (max_points < 1 || max_points > ROAM_ICP_MAX_POINTS) {
        ROAM_SET_ERR(ctx, "loop db: max_points in [1, %d], not %d", ROAM_ICP_MAX_POINTS, max_points);
        return ROAM_E_ARG;
    }
    if (point_stride < 1) { ROAM_SET_ERR(ctx, "loop db: point_stride >= 1, not %d", point_stride); return ROAM_E_ARG; }
    if (!(std::isfinite(range_resolution_m) && range_resolution_m > 0.0)) {
        ROAM_SET_ERR(ctx, "loop db: range_resolution_m finite and > 0, not %g", range_resolution_m);
        return ROAM_E_ARG;
    }
    if (rows < 1 || rows > SC_MAX_ROWS) { ROAM_SET_ERR(ctx, "loop db: rows in [1, %d], not %d", SC_MAX_ROWS, rows); return ROAM_E_ARG; }
    const int64_t per = (int64_t)max_points * 2 * sizeof(double);
    if (db->capacity > SC_DB_BYTES / per) {
        ROAM_SET_ERR(ctx, "loop db: capacity %d x max_points %d x 16 bytes is beyond the %lld bytes of a database", db->capacity, max_points,
                     (long long)SC_DB_BYTES);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<double> table(2 * (size_t)rows);
    (void)roam_polar_cloud_table(rows, table.data(), table.data() + rows);
    const size_t cap = (size_t)db->capacity;
    if (hipMalloc(&db->cloud, (size_t)per * cap) != hipSuccess || hipMalloc(&db->cloud_n, sizeof(int32_t) * cap) != hipSuccess ||
        hipMalloc(&db->cloud_peaks, sizeof(int32_t) * cap) != hipSuccess || hipMalloc(&db->trig, sizeof(double) * table.size()) != hipSuccess) {
        ROAM_SET_ERR(ctx, "loop db: hipMalloc of %lld bytes of clouds failed", (long long)(per * db->capacity));
        for (void **q : {(void **)&db->cloud, (void **)&db->cloud_n, (void **)&db->cloud_peaks, (void **)&db->trig}) {
            if (*q) (void)hipFree(*q);
            *q = nullptr;
        }
        return ROAM_E_HIP;
    }
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(db->cloud_n, 0, sizeof(int32_t) * cap, st));
    HIP_TRY(ctx, hipMemsetAsync(db->cloud_peaks, 0, sizeof(int32_t) * cap, st));
    HIP_TRY(ctx, hipMemcpyAsync(db->trig, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));               // the table is a local
    db->h_n.assign(cap, 0);
    db->h_peaks.assign(cap, 0);
    db->max_points = max_points; db->point_stride = point_stride; db->res = range_resolution_m;
    db->cloud_rows = rows;                                // last: the database keeps clouds from here on
    return ROAM_OK;
}

// db keeps clouds and `index` is a stored entry
static int32_t sc_check_cloud_entry(roam_ctx *ctx, const roam_loop_db *db, int32_t index)
{
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    if (!db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db: db keeps no clouds (roam_loop_db_keep_clouds)"); return ROAM_E_STATE; }
    if (index < 0 || index >= db->count) { ROAM_SET_ERR(ctx, "loop db: index %d outside the %d entries stored", index, db->count); return ROAM_E_ARG; }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_set_cloud(roam_ctx *ctx, roam_loop_db *db, int32_t index, const double *xy, int32_t n)
{
    if (!ctx) return ROAM_E_ARG;
    const int32_t rc = sc_check_cloud_entry(ctx, db, index);
    if (rc != ROAM_OK) return rc;
    if (n < 0 || n > db->max_points) { ROAM_SET_ERR(ctx, "loop db: n in [0, max_points = %d], not %d", db->max_points, n); return ROAM_E_ARG; }
    if (n > 0 && !xy) { ROAM_SET_ERR(ctx, "loop db: xy is null"); return ROAM_E_ARG; }
    for (int64_t q = 0; q < 2 * (int64_t)n; ++q)
        if (!(fabs(xy[q]) <= ROAM_ICP_MAX_COORD)) {       // NaN and the infinities fail too
            ROAM_SET_ERR(ctx, "loop db: xy point %lld: a coordinate that is not finite or beyond %g m", (long long)(q / 2), ROAM_ICP_MAX_COORD);
            return ROAM_E_ARG;
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int32_t two[2] = {n, n};
    if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(db->cloud + 2 * (int64_t)index * db->max_points, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(db->cloud_n + index, two, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(db->cloud_peaks + index, two + 1, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    db->h_n[index] = db->h_peaks[index] = n;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_get_cloud(roam_ctx *ctx, roam_loop_db *db, int32_t index, double *xy_out, int32_t cap, int32_t *n_out,
                                          int32_t *n_peaks_out)
{
    if (!ctx) return ROAM_E_ARG;
    const int32_t rc = sc_check_cloud_entry(ctx, db, index);
    if (rc != ROAM_OK) return rc;
    if (cap < 0 || (cap > 0 && !xy_out)) { ROAM_SET_ERR(ctx, "loop db: xy_out of cap >= 0 points, not %d%s", cap, cap > 0 ? " and null" : ""); return ROAM_E_ARG; }
    const int n = db->h_n[index];
    if (n_out) *n_out = n;
    if (n_peaks_out) *n_peaks_out = db->h_peaks[index];
    const int m = n < cap ? n : cap;
    if (m > 0) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipMemcpyAsync(xy_out, db->cloud + 2 * (int64_t)index * db->max_points, sizeof(double) * 2 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (n > cap) { ROAM_SET_ERR(ctx, "loop db: entry %d holds %d points, capacity %d", index, n, cap); return ROAM_E_CAPACITY; }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_cloud_counts(const roam_loop_db *db, int32_t first, int32_t n, int32_t *n_out, int32_t *n_peaks_out)
{
    if (!db || !db->cloud_rows || first < 0 || n < 0 || n > db->count - first) return ROAM_E_ARG;
    for (int i = 0; i < n; ++i) {
        if (n_out) n_out[i] = db->h_n[first + i];
        if (n_peaks_out) n_peaks_out[i] = db->h_peaks[first + i];
    }
    return ROAM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- verification
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
    int64_t chunk = sc_chunk_limit() / sc_pair_bytes(db);
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

extern "C" int32_t roam_loop_db_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_pairs, const int32_t *src_index, const int32_t *dst_index,
                                       const double *init, const roam_icp_opts *opts, double *pose_out, roam_icp_stats *stats)
{
    if (!ctx) return ROAM_E_ARG;
    int32_t rc = sc_check_pairs(ctx, db, n_pairs, src_index, dst_index, init);
    if (rc != ROAM_OK) return rc;
    if (!pose_out || !stats) { ROAM_SET_ERR(ctx, "loop db verify: %s is null", !pose_out ? "pose_out" : "stats"); return ROAM_E_ARG; }
    roam_icp_opts o;
    if ((rc = roam_icp_resolve_opts(ctx, opts, &o)) != ROAM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int64_t chunk = sc_pair_chunk(db);
    for (int64_t p0 = 0; p0 < n_pairs; p0 += chunk) {
        const int np = (int)(n_pairs - p0 < chunk ? n_pairs - p0 : chunk);
        IcpStoreArgs A;
        if ((rc = sc_verify_scratch(ctx, db, np, o, &A)) != ROAM_OK) return rc;
        if ((rc = sc_stage_pairs(ctx, A, (int)p0, np, src_index, dst_index, init)) != ROAM_OK) return rc;
        HIP_TRY(ctx, launch_icp2d_store(st, A, np));
        HIP_TRY(ctx, hipMemcpyAsync(pose_out + 3 * p0, A.pose, sizeof(double) * 3 * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(stats + p0, A.stats, sizeof(roam_icp_stats) * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));           // the next chunk reuses the scratch
    }
    return ROAM_OK;
}

extern "C" int32_t roam_time_loop_db_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_pairs, const int32_t *src_index, const int32_t *dst_index,
                                            const double *init, const roam_icp_opts *opts, int32_t reps, float *ms_per_rep)
{
    if (!ctx) return ROAM_E_ARG;
    int32_t rc = sc_check_pairs(ctx, db, n_pairs, src_index, dst_index, init);
    if (rc != ROAM_OK) return rc;
    ARG_CHECK(ctx, reps >= 1 && ms_per_rep);
    roam_icp_opts o;
    if ((rc = roam_icp_resolve_opts(ctx, opts, &o)) != ROAM_OK) return rc;
    if (n_pairs * sc_pair_bytes(db) > SC_DB_BYTES) { ROAM_SET_ERR(ctx, "loop db timing: %d pairs do not fit one launch", n_pairs); return ROAM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    IcpStoreArgs A;
    if ((rc = sc_verify_scratch(ctx, db, n_pairs, o, &A)) != ROAM_OK) return rc;
    if ((rc = sc_stage_pairs(ctx, A, 0, n_pairs, src_index, dst_index, init)) != ROAM_OK) return rc;
    return sc_time_launches(ctx, st, reps, ms_per_rep, [&] { return launch_icp2d_store(st, A, n_pairs); });
}

extern "C" int32_t roam_loop_db_query_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                             int32_t k, double max_distance, const roam_icp_opts *opts, int32_t *cand_index, double *cand_dist,
                                             int32_t *cand_shift, double *pose_out, roam_icp_stats *stats)
{
    if (!ctx) return ROAM_E_ARG;
    int32_t rc = sc_check_query(ctx, db, n_query, query_index, max_index, k, max_distance);
    if (rc != ROAM_OK) return rc;
    if (!db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db verify: db keeps no clouds (roam_loop_db_keep_clouds)"); return ROAM_E_STATE; }
    if (!cand_index || !cand_dist || !cand_shift || !pose_out || !stats) {
        ROAM_SET_ERR(ctx, "loop db query: %s is null", !cand_index ? "cand_index" : !cand_dist ? "cand_dist" : !cand_shift ? "cand_shift"
                                                       : !pose_out ? "pose_out" : "stats");
        return ROAM_E_ARG;
    }
    roam_icp_opts o;
    if ((rc = roam_icp_resolve_opts(ctx, opts, &o)) != ROAM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int count = db->count;
    // queries per launch: the distance scratch, the pairs' scratch and the grids' extents
    int64_t chunk = sc_chunk_limit() / ((int64_t)(sizeof(double) + sizeof(int32_t)) * count + (int64_t)k * sc_pair_bytes(db));
    if (chunk > ROAM_ICP_MAX_PAIRS / k) chunk = ROAM_ICP_MAX_PAIRS / k;
    if (chunk < 1) chunk = 1;
    std::vector<int32_t> qm((size_t)n_query);
    for (int q = 0; q < n_query; ++q) qm[q] = max_index[q] < 0 ? 0 : max_index[q] > count ? count : max_index[q];
    for (int64_t q0 = 0; q0 < n_query; q0 += chunk) {
        const int nq = (int)(n_query - q0 < chunk ? n_query - q0 : chunk);
        const int np = nq * k;
        double *d_dist = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * (size_t)nq * count);
        int32_t *d_shift = (int32_t *)roam_scratch(ctx, S_TMP1, sizeof(int32_t) * (size_t)nq * count);
        int32_t *d_q = (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * 2 * (size_t)nq);
        int32_t *d_ci = (int32_t *)roam_scratch(ctx, S_OUT0, sizeof(int32_t) * (size_t)np);
        double *d_cd = (double *)roam_scratch(ctx, S_OUT1, sizeof(double) * (size_t)np);
        int32_t *d_cs = (int32_t *)roam_scratch(ctx, S_OUT2, sizeof(int32_t) * (size_t)np);
        if (!d_dist || !d_shift || !d_q || !d_ci || !d_cd || !d_cs) return ROAM_E_HIP;
        IcpStoreArgs A;
        if ((rc = sc_verify_scratch(ctx, db, np, o, &A)) != ROAM_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(d_q, query_index + q0, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_q + nq, qm.data() + q0, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, sc_launch_distance(st, db, d_q, d_q + nq, nq, d_dist, d_shift));
        HIP_TRY(ctx, sc_launch_select(st, db, d_q + nq, nq, k, max_distance, d_dist, d_shift, d_ci, d_cd, d_cs));
        hipLaunchKernelGGL(loop_pairs_kernel, dim3((np + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, st, d_q, d_ci, d_cs, np, k, db->S,
                           (int32_t *)A.src_index, (int32_t *)A.dst_index, (double *)A.init);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, launch_icp2d_store(st, A, np));
        HIP_TRY(ctx, hipMemcpyAsync(cand_index + q0 * k, d_ci, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(cand_dist + q0 * k, d_cd, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(cand_shift + q0 * k, d_cs, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(pose_out + 3 * q0 * k, A.pose, sizeof(double) * 3 * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(stats + q0 * k, A.stats, sizeof(roam_icp_stats) * (size_t)np, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));           // the one wait of the chunk
    }
    return ROAM_OK;
}
