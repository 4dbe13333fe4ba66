// Loop-closure verification: batched trimmed point-to-point ICP in the plane.  The reference has no such step (its Keyframe.pointCloud,
// Mapping.py:61-62, is stored and never read), so parity is unpinned: the contract is tests/icp_model.py, which restates what follows
// operation by operation.
//
// One workgroup of ICP_THREADS lanes per pair, every pair of a chunk in one launch, the whole iteration loop inside the kernel: no host
// round trip, no workgroup waits for another, every loop is bounded by a count the host checked (max_iterations, the cloud sizes).
//
// An iteration at pose (th, tx, ty) and gate g.
//   Search (the hot loop, n m distance evaluations).  q_i = R(th) src_i + t in float64, rounded to float32; dst rounded to float32.
//   The nearest dst point of q_i minimises d2 = fl32(fl32(dx dx) + fl32(dy dy)) over float32 differences, un-contracted, the lowest
//   index of the minimum.  The search is exhaustive.  A lane keeps up to ICP_IC points q_i in registers (point i of a block of
//   ICP_THREADS ICP_IC points belongs to lane i mod ICP_THREADS); dst goes through LDS in tiles of ICP_TILE points, and every lane walks
//   the tile at the same address - a broadcast, no bank conflict - in 16-byte reads of two points, so one LDS instruction feeds
//   2 ICP_IC distance evaluations.  A lane walks j upwards and replaces on "<" only: the lowest index wins.
//   Pair i is kept when d2 <= fl32(g g).  Fewer than min_pairs kept: FEW_PAIRS, the pose stays.
//   Update, float64, from the float64 coordinates of the kept pairs (a = src_i, b = its partner): the centroids, then in a second
//   pass S_cos = sum (a - am) . (b - bm), S_sin = sum (a - am) x (b - bm); th' = atan2(S_sin, S_cos) (th when both are exactly 0),
//   t' = bm - R(th') am.
//   Stop with OK when g == gate_end, |wrap(th' - th)| < eps_rot and |t' - t| < eps_trans; with MAX_ITERATIONS after that many
//   updates; else g = max(gate_end, g gate_decay).
// A last pass at the final pose with gate_end counts the inliers and takes rms = sqrt(mean d2), d2 in float64 between the float64
// transformed point and its partner's float64 coordinates (+inf without inliers).
//
// Sums.  No floating-point atomics.  A lane adds its own points in ascending i from zero; a wave adds its lanes by the xor butterfly
// (32, 16, ... 1: every lane ends with the same bits); the waves' sums go to LDS and every lane adds them in wave order.  The order
// is a function of the pair alone, so a pair's result is the same bits alone, anywhere in a batch, in any chunk and in any call.
// The partner indices live in global scratch; each entry is written and read by the same lane only.
//
// Budget: 32 KiB of LDS for the tile plus 320 bytes for the sums; ICP_IC = 4 points (8 float32 + 4 best + 4 index) per lane keep
// the search in registers.
#include "loop.h"
#include <math.h>
#include <limits>

#define ICP_THREADS 512
#define ICP_WAVES (ICP_THREADS / 64)
#define ICP_IC 4                                  // points a lane holds through one sweep of dst
#define ICP_BLOCK (ICP_THREADS * ICP_IC)
#define ICP_TILE 4096                             // dst points of one LDS tile (float2 each)
#define ICP_NRED 5                                // doubles reduced at once
#define ICP_CHUNK_BYTES ((int64_t)2000 << 20)     // scratch of one launch, as in the other batched stages

struct IcpArgs {
    const int32_t *src_off, *dst_off;             // n_pairs + 1 each, as the caller gave them; the clouds below start at src_off[0] / dst_off[0]
    const double *src, *dst;
    const double *init;                           // n_pairs x 3
    int32_t *partner;                             // one per src point
    double *pose;                                 // n_pairs x 3
    roam_icp_stats *stats;
    roam_icp_opts o;
};

// ---------------------------------------------------------------------------------------------------------------- device
// the sums of v[0 .. NV) over the workgroup, the same bits in every lane: butterfly, then the waves in order
template <int NV>
__device__ static void icp_reduce(double *v, double (*red)[ICP_NRED])
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < NV; ++k)
        for (int d = 32; d > 0; d >>= 1) v[k] += __shfl_xor(v[k], d);
    __syncthreads();                              // the previous sums have been read
    if (lane == 0)
        for (int k = 0; k < NV; ++k) red[wv][k] = v[k];
    __syncthreads();
    for (int k = 0; k < NV; ++k) {
        double s = red[0][k];
        for (int w = 1; w < ICP_WAVES; ++w) s += red[w][k];
        v[k] = s;
    }
}

// KC rows of ICP_THREADS points from i0 on against every dst point: partner[i] = the nearest within gate2, else -1
template <int KC>
__device__ static void icp_sweep(const double *__restrict__ src, int n, int i0, const double *__restrict__ dst, int m, double c, double s,
                                 double tx, double ty, float gate2, float4 *tile, int32_t *__restrict__ partner)
{
    float qx[KC], qy[KC], best[KC];
    int bj[KC];
    for (int k = 0; k < KC; ++k) {
        const int i = i0 + k * ICP_THREADS + (int)threadIdx.x;
        double x = 0.0, y = 0.0;
        if (i < n) { x = src[2 * (int64_t)i]; y = src[2 * (int64_t)i + 1]; }
        qx[k] = (float)((c * x - s * y) + tx);
        qy[k] = (float)((s * x + c * y) + ty);
        best[k] = std::numeric_limits<float>::infinity();
        bj[k] = -1;
    }
    for (int t0 = 0; t0 < m; t0 += ICP_TILE) {
        const int tl = m - t0 < ICP_TILE ? m - t0 : ICP_TILE;
        const int tl2 = (tl + 1) >> 1;            // 16-byte cells; an odd tile ends with a point at infinity, which is never "<"
        __syncthreads();                          // the previous tile has been read
        for (int h = threadIdx.x; h < tl2; h += ICP_THREADS) {
            const int j = t0 + 2 * h;
            float4 v;
            v.x = (float)dst[2 * (int64_t)j];
            v.y = (float)dst[2 * (int64_t)j + 1];
            v.z = v.w = std::numeric_limits<float>::infinity();
            if (2 * h + 1 < tl) { v.z = (float)dst[2 * (int64_t)j + 2]; v.w = (float)dst[2 * (int64_t)j + 3]; }
            tile[h] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int h = 0; h < tl2; ++h) {
            const float4 v = tile[h];             // one address for the whole wave
            const int j = t0 + 2 * h;
            for (int k = 0; k < KC; ++k) {
                const float dx0 = qx[k] - v.x, dy0 = qy[k] - v.y;
                const float d0 = __fadd_rn(__fmul_rn(dx0, dx0), __fmul_rn(dy0, dy0));
                if (d0 < best[k]) { best[k] = d0; bj[k] = j; }
                const float dx1 = qx[k] - v.z, dy1 = qy[k] - v.w;
                const float d1 = __fadd_rn(__fmul_rn(dx1, dx1), __fmul_rn(dy1, dy1));
                if (d1 < best[k]) { best[k] = d1; bj[k] = j + 1; }
            }
        }
    }
    for (int k = 0; k < KC; ++k) {
        const int i = i0 + k * ICP_THREADS + (int)threadIdx.x;
        if (i < n) partner[i] = (bj[k] >= 0 && bj[k] < m && best[k] <= gate2) ? bj[k] : -1;
    }
}

// the search of every src point at pose (th, tx, ty)
__device__ static void icp_search(const double *src, int n, const double *dst, int m, double th, double tx, double ty, float gate2, float4 *tile,
                                  int32_t *partner)
{
    double s, c;
    sincos(th, &s, &c);
    for (int i0 = 0; i0 < n; i0 += ICP_BLOCK) {
        const int rows = (n - i0 + ICP_THREADS - 1) / ICP_THREADS;      // uniform: the rows of this block that hold a point
        if (rows >= 4) icp_sweep<4>(src, n, i0, dst, m, c, s, tx, ty, gate2, tile, partner);
        else if (rows == 3) icp_sweep<3>(src, n, i0, dst, m, c, s, tx, ty, gate2, tile, partner);
        else if (rows == 2) icp_sweep<2>(src, n, i0, dst, m, c, s, tx, ty, gate2, tile, partner);
        else icp_sweep<1>(src, n, i0, dst, m, c, s, tx, ty, gate2, tile, partner);
    }
}

// one pair, by the whole workgroup: src (n points) onto dst (m points) from the pose init[0 .. 3), partner = n ints of global scratch
// that no other workgroup touches -> pose[0 .. 3), *stats (written by lane 0).  The LDS is declared here, once for every kernel that
// runs a pair: the search then reads its tile at an address the compiler knows (ds_read_b128), not through a generic pointer
__device__ static void icp2d_pair(const double *__restrict__ src, int n, const double *__restrict__ dst, int m, int32_t *__restrict__ partner,
                                  const double *__restrict__ init, const roam_icp_opts &o, double *__restrict__ pose,
                                  roam_icp_stats *__restrict__ stats)
{
    __shared__ float4 tile[ICP_TILE / 2];
    __shared__ double red[ICP_WAVES][ICP_NRED];
    const double inf = std::numeric_limits<double>::infinity();
    double th = init[0], tx = init[1], ty = init[2];
    int status = ROAM_ICP_MAX_ITERATIONS, iterations = 0, n_last = 0;
    double v[ICP_NRED];

    if (n < 1 || m < 1) status = ROAM_ICP_FEW_PAIRS;
    else {
        double g = o.gate_start;
        for (int it = 0; it < o.max_iterations; ++it) {
            icp_search(src, n, dst, m, th, tx, ty, (float)(g * g), tile, partner);
            for (int k = 0; k < ICP_NRED; ++k) v[k] = 0.0;
            for (int i = threadIdx.x; i < n; i += ICP_THREADS) {
                const int j = partner[i];
                if (j < 0) continue;
                v[0] += 1.0;
                v[1] += src[2 * (int64_t)i];
                v[2] += src[2 * (int64_t)i + 1];
                v[3] += dst[2 * (int64_t)j];
                v[4] += dst[2 * (int64_t)j + 1];
            }
            icp_reduce<5>(v, red);
            n_last = (int)v[0];
            if (n_last < o.min_pairs) { status = ROAM_ICP_FEW_PAIRS; break; }
            const double amx = v[1] / v[0], amy = v[2] / v[0], bmx = v[3] / v[0], bmy = v[4] / v[0];
            v[0] = v[1] = 0.0;
            for (int i = threadIdx.x; i < n; i += ICP_THREADS) {
                const int j = partner[i];
                if (j < 0) continue;
                const double ax = src[2 * (int64_t)i] - amx, ay = src[2 * (int64_t)i + 1] - amy;
                const double bx = dst[2 * (int64_t)j] - bmx, by = dst[2 * (int64_t)j + 1] - bmy;
                v[0] += ax * bx + ay * by;
                v[1] += ax * by - ay * bx;
            }
            icp_reduce<2>(v, red);
            const double th2 = (v[0] == 0.0 && v[1] == 0.0) ? th : atan2(v[1], v[0]);
            double s2, c2;
            sincos(th2, &s2, &c2);
            const double tx2 = bmx - (c2 * amx - s2 * amy), ty2 = bmy - (s2 * amx + c2 * amy);
            const double dth = fabs(roam_normalize_angle(th2 - th));
            const double ex = tx2 - tx, ey = ty2 - ty;
            const double dt = sqrt(ex * ex + ey * ey);
            th = th2; tx = tx2; ty = ty2;
            iterations = it + 1;
            if (g == o.gate_end && dth < o.eps_rot && dt < o.eps_trans) { status = ROAM_ICP_OK; break; }
            const double gn = g * o.gate_decay;
            g = gn > o.gate_end ? gn : o.gate_end;
        }
    }

    // the score at the final pose
    int n_in = 0;
    double rms = inf;
    if (n >= 1 && m >= 1) {
        icp_search(src, n, dst, m, th, tx, ty, (float)(o.gate_end * o.gate_end), tile, partner);
        double s, c;
        sincos(th, &s, &c);
        v[0] = v[1] = 0.0;
        for (int i = threadIdx.x; i < n; i += ICP_THREADS) {
            const int j = partner[i];
            if (j < 0) continue;
            const double x = src[2 * (int64_t)i], y = src[2 * (int64_t)i + 1];
            const double ex = ((c * x - s * y) + tx) - dst[2 * (int64_t)j], ey = ((s * x + c * y) + ty) - dst[2 * (int64_t)j + 1];
            v[0] += 1.0;
            v[1] += ex * ex + ey * ey;
        }
        icp_reduce<2>(v, red);
        n_in = (int)v[0];
        if (n_in > 0) rms = sqrt(v[1] / v[0]);
    }
    if (threadIdx.x == 0) {
        pose[0] = th;
        pose[1] = tx;
        pose[2] = ty;
        roam_icp_stats st;
        st.status = status;
        st.iterations = iterations;
        st.n_pairs_last = n_last;
        st.n_inliers = n_in;
        st.rms = rms;
        *stats = st;
    }
}

__global__ __launch_bounds__(ICP_THREADS) void icp2d_kernel(IcpArgs A)
{
    const int p = blockIdx.x;
    const int64_t s0 = (int64_t)A.src_off[p] - A.src_off[0], d0 = (int64_t)A.dst_off[p] - A.dst_off[0];
    const int n = A.src_off[p + 1] - A.src_off[p], m = A.dst_off[p + 1] - A.dst_off[p];
    icp2d_pair(A.src + 2 * s0, n, A.dst + 2 * d0, m, A.partner + s0, A.init + 3 * (int64_t)p, A.o, A.pose + 3 * (int64_t)p, A.stats + p);
}

// the pairs of the loop database's cloud store.  The partner scratch is per PAIR (p max_points): one stored cloud may be the source of
// several pairs of a launch - a query against its k candidates - and each workgroup needs partners of its own
__global__ __launch_bounds__(ICP_THREADS) void icp2d_store_kernel(IcpStoreArgs A)
{
    const int p = blockIdx.x;
    const int si = A.src_index[p], di = A.dst_index[p];
    const int n = si >= 0 ? A.cloud_n[si] : 0, m = di >= 0 ? A.cloud_n[di] : 0;
    const double *src = A.cloud + 2 * (int64_t)(si >= 0 ? si : 0) * A.max_points, *dst = A.cloud + 2 * (int64_t)(di >= 0 ? di : 0) * A.max_points;
    icp2d_pair(src, n, dst, m, A.partner + (int64_t)p * A.max_points, A.init + 3 * (int64_t)p, A.o, A.pose + 3 * (int64_t)p, A.stats + p);
}

// ---------------------------------------------------------------------------------------------------------------- host
static const roam_icp_opts ICP_DEFAULTS = {3.0, 0.5, 0.8, 40, 1e-4, 1e-5, 3};

// the options' limits, shared with the loop database's verification
static int32_t icp_check_opts(roam_ctx *ctx, const roam_icp_opts *o)
{
    if (!(std::isfinite(o->gate_start) && std::isfinite(o->gate_end) && o->gate_end > 0.0 && o->gate_end <= o->gate_start &&
          o->gate_start <= ROAM_ICP_MAX_COORD)) {
        ROAM_SET_ERR(ctx, "icp2d: gates 0 < gate_end <= gate_start <= %g, not %g and %g", ROAM_ICP_MAX_COORD, o->gate_end, o->gate_start);
        return ROAM_E_ARG;
    }
    if (!(o->gate_decay > 0.0 && o->gate_decay <= 1.0)) { ROAM_SET_ERR(ctx, "icp2d: gate_decay in (0, 1], not %g", o->gate_decay); return ROAM_E_ARG; }
    if (o->max_iterations < 1 || o->max_iterations > ROAM_ICP_ITERATION_LIMIT) {
        ROAM_SET_ERR(ctx, "icp2d: max_iterations in [1, %d], not %d", ROAM_ICP_ITERATION_LIMIT, o->max_iterations);
        return ROAM_E_ARG;
    }
    if (o->min_pairs < 2) { ROAM_SET_ERR(ctx, "icp2d: min_pairs >= 2, not %d", o->min_pairs); return ROAM_E_ARG; }
    if (!(o->eps_trans >= 0.0 && o->eps_rot >= 0.0)) {      // NaN fails too
        ROAM_SET_ERR(ctx, "icp2d: eps_trans and eps_rot >= 0, not %g and %g", o->eps_trans, o->eps_rot);
        return ROAM_E_ARG;
    }
    return ROAM_OK;
}

int32_t roam_icp_resolve_opts(roam_ctx *ctx, const roam_icp_opts *opts, roam_icp_opts *o)
{
    *o = opts ? *opts : ICP_DEFAULTS;
    return icp_check_opts(ctx, o);
}

// everything roam_icp2d_batch refuses, before any device call
static int32_t icp_check(roam_ctx *ctx, int32_t n_pairs, const int32_t *src_off, const double *src, const int32_t *dst_off, const double *dst,
                         const double *init, const roam_icp_opts *o, const double *pose_out, const roam_icp_stats *stats)
{
    if (!src_off || !src || !dst_off || !dst || !init || !pose_out || !stats) {
        ROAM_SET_ERR(ctx, "icp2d: %s is null", !src_off ? "src_off" : !src ? "src" : !dst_off ? "dst_off" : !dst ? "dst" : !init ? "init"
                                               : !pose_out ? "pose_out" : "stats");
        return ROAM_E_ARG;
    }
    if (n_pairs < 1 || n_pairs > ROAM_ICP_MAX_PAIRS) {
        ROAM_SET_ERR(ctx, "icp2d: n_pairs in [1, %d], not %d", ROAM_ICP_MAX_PAIRS, n_pairs);
        return ROAM_E_ARG;
    }
    const int32_t ro = icp_check_opts(ctx, o);
    if (ro != ROAM_OK) return ro;
    for (int side = 0; side < 2; ++side) {
        const int32_t *off = side ? dst_off : src_off;
        const double *xy = side ? dst : src;
        const char *name = side ? "dst" : "src";
        if (off[0] < 0) { ROAM_SET_ERR(ctx, "icp2d: %s_off[0] = %d is negative", name, off[0]); return ROAM_E_ARG; }
        for (int p = 0; p < n_pairs; ++p) {
            const int64_t len = (int64_t)off[p + 1] - off[p];
            if (len < 0) { ROAM_SET_ERR(ctx, "icp2d: %s_off decreases at pair %d (%d after %d)", name, p, off[p + 1], off[p]); return ROAM_E_ARG; }
            if (len > ROAM_ICP_MAX_POINTS) {
                ROAM_SET_ERR(ctx, "icp2d: pair %d: %s has %lld points, more than %d", p, name, (long long)len, ROAM_ICP_MAX_POINTS);
                return ROAM_E_ARG;
            }
        }
        for (int64_t q = 2 * (int64_t)off[0]; q < 2 * (int64_t)off[n_pairs]; ++q)
            if (!(fabs(xy[q]) <= ROAM_ICP_MAX_COORD)) {       // NaN and the infinities fail too
                ROAM_SET_ERR(ctx, "icp2d: %s point %lld: a coordinate that is not finite or beyond %g m", name, (long long)(q / 2), ROAM_ICP_MAX_COORD);
                return ROAM_E_ARG;
            }
    }
    for (int p = 0; p < n_pairs; ++p)
        if (!(std::isfinite(init[3 * p]) && fabs(init[3 * p + 1]) <= ROAM_ICP_MAX_COORD && fabs(init[3 * p + 2]) <= ROAM_ICP_MAX_COORD)) {
            ROAM_SET_ERR(ctx, "icp2d: pair %d: an initial pose that is not finite or beyond %g m", p, ROAM_ICP_MAX_COORD);
            return ROAM_E_ARG;
        }
    return ROAM_OK;
}

// bytes of device scratch the pairs [p0, p1) take
static int64_t icp_pairs_bytes(const int32_t *src_off, const int32_t *dst_off, int p0, int p1)
{
    const int64_t ns = (int64_t)src_off[p1] - src_off[p0], nd = (int64_t)dst_off[p1] - dst_off[p0];
    return ns * (2 * sizeof(double) + sizeof(int32_t)) + nd * 2 * sizeof(double) +
           (int64_t)(p1 - p0) * (6 * sizeof(double) + sizeof(roam_icp_stats) + 2 * sizeof(int32_t)) + 2 * sizeof(int32_t);
}

// upload the pairs [p0, p1) and fill the kernel's arguments
static int32_t icp_stage(roam_ctx *ctx, int p0, int p1, const int32_t *src_off, const double *src, const int32_t *dst_off, const double *dst,
                         const double *init, const roam_icp_opts &o, IcpArgs *A)
{
    const hipStream_t st = ctx->stream;
    const int np = p1 - p0;
    const size_t ns = (size_t)(src_off[p1] - src_off[p0]), nd = (size_t)(dst_off[p1] - dst_off[p0]);
    double *d_src = (double *)roam_scratch(ctx, S_IN0, sizeof(double) * 2 * (ns ? ns : 1));
    double *d_dst = (double *)roam_scratch(ctx, S_IN1, sizeof(double) * 2 * (nd ? nd : 1));
    int32_t *d_off = (int32_t *)roam_scratch(ctx, S_IN2, sizeof(int32_t) * 2 * (size_t)(np + 1));
    double *d_init = (double *)roam_scratch(ctx, S_IN3, sizeof(double) * 3 * (size_t)np);
    int32_t *d_partner = (int32_t *)roam_scratch(ctx, S_TMP0, sizeof(int32_t) * (ns ? ns : 1));
    double *d_pose = (double *)roam_scratch(ctx, S_OUT0, sizeof(double) * 3 * (size_t)np);
    roam_icp_stats *d_stats = (roam_icp_stats *)roam_scratch(ctx, S_OUT1, sizeof(roam_icp_stats) * (size_t)np);
    if (!d_src || !d_dst || !d_off || !d_init || !d_partner || !d_pose || !d_stats) return ROAM_E_HIP;
    if (ns) HIP_TRY(ctx, hipMemcpyAsync(d_src, src + 2 * (int64_t)src_off[p0], sizeof(double) * 2 * ns, hipMemcpyHostToDevice, st));
    if (nd) HIP_TRY(ctx, hipMemcpyAsync(d_dst, dst + 2 * (int64_t)dst_off[p0], sizeof(double) * 2 * nd, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_off, src_off + p0, sizeof(int32_t) * (size_t)(np + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_off + np + 1, dst_off + p0, sizeof(int32_t) * (size_t)(np + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_init, init + 3 * (int64_t)p0, sizeof(double) * 3 * (size_t)np, hipMemcpyHostToDevice, st));
    *A = IcpArgs{d_off, d_off + np + 1, d_src, d_dst, d_init, d_partner, d_pose, d_stats, o};
    return ROAM_OK;
}

static hipError_t icp_launch(hipStream_t st, const IcpArgs &A, int np)
{
    hipLaunchKernelGGL(icp2d_kernel, dim3(np), dim3(ICP_THREADS), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_icp2d_store(hipStream_t st, const IcpStoreArgs &A, int np)
{
    hipLaunchKernelGGL(icp2d_store_kernel, dim3(np), dim3(ICP_THREADS), 0, st, A);
    return hipGetLastError();
}

extern "C" int32_t roam_icp2d_batch(roam_ctx *ctx, int32_t n_pairs, const int32_t *src_off, const double *src, const int32_t *dst_off,
                                    const double *dst, const double *init, const roam_icp_opts *opts, double *pose_out, roam_icp_stats *stats)
{
    if (!ctx) return ROAM_E_ARG;
    const roam_icp_opts o = opts ? *opts : ICP_DEFAULTS;
    const int32_t rc = icp_check(ctx, n_pairs, src_off, src, dst_off, dst, init, &o, pose_out, stats);
    if (rc != ROAM_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int64_t limit = roam_chunk_limit("ROAM_ICP_CHUNK_BYTES", ICP_CHUNK_BYTES);
    for (int p0 = 0; p0 < n_pairs;) {
        int p1 = p0 + 1;                          // a pair is at most 8192 + 8192 points: it always fits
        while (p1 < n_pairs && icp_pairs_bytes(src_off, dst_off, p0, p1 + 1) <= limit) ++p1;
        IcpArgs A;
        const int32_t rs = icp_stage(ctx, p0, p1, src_off, src, dst_off, dst, init, o, &A);
        if (rs != ROAM_OK) return rs;
        HIP_TRY(ctx, icp_launch(st, A, p1 - p0));
        HIP_TRY(ctx, hipMemcpyAsync(pose_out + 3 * (int64_t)p0, A.pose, sizeof(double) * 3 * (size_t)(p1 - p0), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(stats + p0, A.stats, sizeof(roam_icp_stats) * (size_t)(p1 - p0), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));   // the next chunk reuses the scratch
        p0 = p1;
    }
    return ROAM_OK;
}

extern "C" int32_t roam_time_icp2d_batch(roam_ctx *ctx, int32_t n_pairs, const int32_t *src_off, const double *src, const int32_t *dst_off,
                                         const double *dst, const double *init, const roam_icp_opts *opts, int32_t reps, float *ms_per_rep)
{
    if (!ctx) return ROAM_E_ARG;
    const roam_icp_opts o = opts ? *opts : ICP_DEFAULTS;
    ARG_CHECK(ctx, reps >= 1 && ms_per_rep);
    double pose_dummy = 0;
    roam_icp_stats stats_dummy;
    const int32_t rc = icp_check(ctx, n_pairs, src_off, src, dst_off, dst, init, &o, &pose_dummy, &stats_dummy);
    if (rc != ROAM_OK) return rc;
    if (icp_pairs_bytes(src_off, dst_off, 0, n_pairs) > ICP_CHUNK_BYTES) {
        ROAM_SET_ERR(ctx, "icp2d timing: %d pairs do not fit one launch", n_pairs);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    IcpArgs A;
    const int32_t rs = icp_stage(ctx, 0, n_pairs, src_off, src, dst_off, dst, init, o, &A);
    if (rs != ROAM_OK) return rs;
    return roam_time_launches(ctx, st, reps, ms_per_rep, [&] { return icp_launch(st, A, n_pairs); });
}
