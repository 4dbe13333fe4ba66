// Laplacian-of-Gaussian blob candidates: the image-scale part of skimage.feature.blob_log as
// getFeatures.getBlobsFromCart calls it with method="log" (reference getFeatures.py:22-53).
// Per sigma, float64 like the reference (scipy.ndimage.gaussian_laplace on cartImage.astype(double)):
//   log_cols : C0 = cols_k0(img), C2 = cols_k2(img)   (1-D correlation along axis 0; the symmetric
//              pair sum x[i-j] + x[i+j] is shared by both kernels)
//   log_rows : layer = -(rows_k0(C2) + rows_k2(C0)) * sigma^2   (along axis 1, row staged in LDS)
// Both follow scipy's symmetric correlate1d path term for term: t = x[i]*w[r]; then for j = r..1,
// t += (x[i-j] + x[i+j]) * w[r-j]; boundary 'reflect' (half-sample symmetric, period 2n, so a radius
// larger than the line reflects again).  The kernel weights come from the caller (NumPy, as scipy
// computes them).  A thread keeps K consecutive outputs and slides two windows of K inputs across
// the taps: two loads per tap for K outputs.
//   log_maxima (count + write) : peak_local_max of the (sigma, row, col) cube with a 3x3x3 footprint,
//              positions outside the cube count as 0, v > threshold, C (row, col, sigma) order, and no
//              peaks at all for a trivial cube (every position equal to its neighbourhood maximum, which
//              happens exactly when the cube is constant and >= 0).
#include "roam_internal.h"

#define LOG_KC 8                 // outputs per thread, column pass
#define LOG_KR 9                 // outputs per thread, row pass (odd: 9-double LDS stride is free of bank conflicts)
#define LOG_ROW_SPAN (256 * LOG_KR)
#define LOG_MAX_RADIUS 800       // row pass LDS: 2 * (LOG_ROW_SPAN + 2r) doubles <= 64 KiB

// scipy's NI_EXTEND_REFLECT extended to any distance: period 2n, mirrored second half
__device__ __forceinline__ int log_refl(int k, int n)
{
    if ((unsigned)k < (unsigned)n) return k;
    const int p = 2 * n;
    k %= p;
    if (k < 0) k += p;
    return k < n ? k : p - 1 - k;
}

// block: 64 columns x 4 waves, a wave = LOG_KC consecutive output rows of 64 columns (the row index is wave-uniform)
template <typename T>
__global__ __launch_bounds__(256) void log_cols_kernel(const T *__restrict__ img, int H, int W, int r, const double *__restrict__ w0,
                                                       const double *__restrict__ w2, double *__restrict__ C0, double *__restrict__ C2)
{
    constexpr int K = LOG_KC;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i0 = (blockIdx.y * 4 + wv) * K;
    if (i0 >= H) return;
    const int c = blockIdx.x * 64 + lane;
    const T *col = img + (c < W ? c : W - 1);
    auto ld = [&](int i) -> double { return (double)col[(int64_t)log_refl(i, H) * W]; };
    double a0[K], a2[K], L[K], R[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double x = ld(i0 + k);
        a0[k] = x * w0[r];
        a2[k] = x * w2[r];
    }
    if (r > 0) {
#pragma unroll
        for (int k = 0; k < K; k++) { L[k] = ld(i0 + k - r); R[k] = ld(i0 + k + r); }
    }
#pragma unroll 4
    for (int s = 0; s < r; s++) {                    // j = r - s; weight index r - j = s
        const double u0 = w0[s], u2 = w2[s];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double p = L[k] + R[k];
            a0[k] = a0[k] + p * u0;
            a2[k] = a2[k] + p * u2;
        }
        const int j = r - s;
        if (j > 1) {
#pragma unroll
            for (int k = 0; k < K - 1; k++) L[k] = L[k + 1];
            L[K - 1] = ld(i0 + K - j);
#pragma unroll
            for (int k = K - 1; k > 0; k--) R[k] = R[k - 1];
            R[0] = ld(i0 + j - 1);
        }
    }
    if (c >= W) return;
#pragma unroll
    for (int k = 0; k < K; k++)
        if (i0 + k < H) {
            const int64_t o = (int64_t)(i0 + k) * W + c;
            C0[o] = a0[k];
            C2[o] = a2[k];
        }
}

// block: LOG_ROW_SPAN columns of one row; thread t computes columns cb + t*K .. + K-1.  Dynamic LDS: 2 * (LOG_ROW_SPAN + 2r) doubles.
__global__ __launch_bounds__(256) void log_rows_kernel(const double *__restrict__ C0, const double *__restrict__ C2, int H, int W, int r,
                                                       const double *__restrict__ w0, const double *__restrict__ w2, double scale,
                                                       double *__restrict__ out)
{
    constexpr int K = LOG_KR;
    extern __shared__ double lds[];
    const int row = blockIdx.y, cb = blockIdx.x * LOG_ROW_SPAN;
    const int span = LOG_ROW_SPAN + 2 * r;
    double *s0 = lds, *s2 = lds + span;
    const double *c0 = C0 + (int64_t)row * W, *c2 = C2 + (int64_t)row * W;
    for (int e = threadIdx.x; e < span; e += 256) {
        const int cc = log_refl(cb - r + e, W);
        s0[e] = c0[cc];
        s2[e] = c2[cc];
    }
    __syncthreads();
    const int q = threadIdx.x * K;                   // LDS index of column cb + q + k is q + k + r
    double a[K], b[K], L0[K], R0[K], L2[K], R2[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        a[k] = s2[q + k + r] * w0[r];                // rows_k0(C2)
        b[k] = s0[q + k + r] * w2[r];                // rows_k2(C0)
    }
    if (r > 0) {
#pragma unroll
        for (int k = 0; k < K; k++) { L0[k] = s0[q + k]; R0[k] = s0[q + k + 2 * r]; L2[k] = s2[q + k]; R2[k] = s2[q + k + 2 * r]; }
    }
#pragma unroll 2
    for (int s = 0; s < r; s++) {
        const double u0 = w0[s], u2 = w2[s];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double p2 = L2[k] + R2[k], p0 = L0[k] + R0[k];
            a[k] = a[k] + p2 * u0;
            b[k] = b[k] + p0 * u2;
        }
        const int j = r - s;
        if (j > 1) {
#pragma unroll
            for (int k = 0; k < K - 1; k++) { L0[k] = L0[k + 1]; L2[k] = L2[k + 1]; }
            L0[K - 1] = s0[q + K + r - j];
            L2[K - 1] = s2[q + K + r - j];
#pragma unroll
            for (int k = K - 1; k > 0; k--) { R0[k] = R0[k - 1]; R2[k] = R2[k - 1]; }
            R0[0] = s0[q + r + j - 1];
            R2[0] = s2[q + r + j - 1];
        }
    }
    __syncthreads();                                 // stage the results for coalesced stores
#pragma unroll
    for (int k = 0; k < K; k++) s0[q + k] = (-(a[k] + b[k])) * scale;
    __syncthreads();
    double *o = out + (int64_t)row * W;
    const int nc = min(LOG_ROW_SPAN, W - cb);
    for (int e = threadIdx.x; e < nc; e += 256) o[cb + e] = s0[e];
}

// v (> thr >= 0) at (s, r, c) is a maximum of its 3x3x3 neighbourhood; positions outside the cube are 0 <= thr < v
__device__ __forceinline__ bool log_is_max(const double *Q, int64_t plane, int S, int H, int W, int r, int c, int s, double v)
{
    for (int ds = -1; ds <= 1; ds++) {
        const int ss = s + ds;
        if (ss < 0 || ss >= S) continue;
        const double *P = Q + ss * plane;
        for (int dr = -1; dr <= 1; dr++) {
            const int rr = r + dr;
            if (rr < 0 || rr >= H) continue;
            for (int dc = -1; dc <= 1; dc++) {
                const int cc = c + dc;
                if (cc < 0 || cc >= W) continue;
                if (P[(int64_t)rr * W + cc] > v) return false;
            }
        }
    }
    return true;
}

__device__ __forceinline__ int log_blk_scan(int v, int *sh, int *total)
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
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) { int s = sh[i]; if (i < w) base += s; tot += s; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// WRITE=false: row_count[r] = maxima in row r, row_const[r] = every value of row r (all sigmas) equals Q[0].
// WRITE=true: emit at row_off[r] + position, unless the scan found the cube trivial.
template <bool WRITE>
__global__ __launch_bounds__(256) void log_maxima_kernel(const double *__restrict__ Q, int S, int H, int W, double thr,
                                                         int32_t *__restrict__ row_count, int32_t *__restrict__ row_const,
                                                         const int32_t *__restrict__ row_off, const int32_t *__restrict__ trivial,
                                                         int32_t *__restrict__ out_rcs, double *__restrict__ out_val, int cap)
{
    __shared__ int sh[8];
    if (WRITE && *trivial) return;
    const int r = blockIdx.x, t = threadIdx.x;
    const int64_t plane = (int64_t)H * W;
    const int items = (W + 255) / 256;
    const int lo = t * items, hi = min(lo + items, W);
    const double v0 = Q[0];
    int cnt = 0, same = 1;
    for (int c = lo; c < hi; c++)
        for (int s = 0; s < S; s++) {
            const double v = Q[s * plane + (int64_t)r * W + c];
            if (!WRITE) same &= v == v0;
            cnt += (v > thr && log_is_max(Q, plane, S, H, W, r, c, s, v)) ? 1 : 0;
        }
    int total;
    int pos = log_blk_scan(cnt, sh, &total);
    if (!WRITE) {
        same = __syncthreads_and(same);
        if (t == 0) { row_count[r] = total; row_const[r] = same; }
        return;
    }
    pos += row_off[r];
    for (int c = lo; c < hi; c++)
        for (int s = 0; s < S; s++) {
            const double v = Q[s * plane + (int64_t)r * W + c];
            if (v > thr && log_is_max(Q, plane, S, H, W, r, c, s, v)) {
                if (pos < cap) {
                    out_rcs[3 * (int64_t)pos] = r; out_rcs[3 * (int64_t)pos + 1] = c; out_rcs[3 * (int64_t)pos + 2] = s;
                    out_val[pos] = v;
                }
                pos++;
            }
        }
}

// row offsets + the trivial-cube rule (peak_local_max: no peak when every position equals its neighbourhood maximum;
// a one-element cube is compared with the threshold only)
__global__ __launch_bounds__(256) void log_row_scan_kernel(const double *__restrict__ Q, int64_t size, const int32_t *__restrict__ row_count,
                                                           const int32_t *__restrict__ row_const, int H, int32_t *__restrict__ row_off,
                                                           int32_t *__restrict__ total_out, int32_t *__restrict__ trivial_out)
{
    __shared__ int sh[8];
    const int t = threadIdx.x;
    const int items = (H + 255) / 256;
    const int lo = t * items, hi = min(lo + items, H);
    int c = 0, same = 1;
    for (int r = lo; r < hi; r++) { c += row_count[r]; same &= row_const[r]; }
    same = __syncthreads_and(same);
    int total;
    int pos = log_blk_scan(c, sh, &total);
    for (int r = lo; r < hi; r++) { row_off[r] = pos; pos += row_count[r]; }
    if (t == 0) {
        const int triv = same && Q[0] >= 0.0 && size > 1;
        *trivial_out = triv;
        *total_out = triv ? 0 : total;
    }
}

extern "C" int32_t roam_log_maxima(roam_ctx *ctx, const void *img, int32_t img_bytes_per_px, int32_t w, int32_t h, int32_t num_sigma,
                                   const int32_t *radius, const double *kernels, const double *scale, double threshold,
                                   int32_t *out_rcs, double *out_val, int32_t cap, int32_t *n_out, double *out_layers)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, img && radius && kernels && scale && out_rcs && out_val && n_out && w >= 1 && h >= 1 && num_sigma >= 1 &&
                       h <= 65535 && cap >= 0 && threshold >= 0 && (img_bytes_per_px == 4 || img_bytes_per_px == 8));
    int64_t nw = 0;
    for (int s = 0; s < num_sigma; s++) {
        const int r = radius[s];
        ARG_CHECK(ctx, r >= 0 && r <= LOG_MAX_RADIUS);
        const double *k0 = kernels + nw, *k2 = k0 + 2 * r + 1;
        for (int j = 1; j <= r; j++)                  // scipy's symmetric correlate1d path is the one restated
            ARG_CHECK(ctx, k0[r - j] == k0[r + j] && k2[r - j] == k2[r + j]);
        nw += 2 * (2 * r + 1);
    }
    hipStream_t st = ctx->stream;
    const size_t npx = (size_t)w * h;
    void *dimg = roam_scratch(ctx, S_IN0, (size_t)img_bytes_per_px * npx);
    double *dk = (double *)roam_scratch(ctx, S_IN1, sizeof(double) * (size_t)nw);
    double *C = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * 2 * npx);
    double *Q = (double *)roam_scratch(ctx, S_TMP2, sizeof(double) * npx * (size_t)num_sigma);
    int32_t *rowi = (int32_t *)roam_scratch(ctx, S_TMP1, sizeof(int32_t) * (3 * (size_t)h + 2));
    int32_t *drcs = (int32_t *)roam_scratch(ctx, S_OUT0, sizeof(int32_t) * 3 * (size_t)(cap > 0 ? cap : 1));
    double *dval = (double *)roam_scratch(ctx, S_OUT1, sizeof(double) * (size_t)(cap > 0 ? cap : 1));
    if (!dimg || !dk || !C || !Q || !rowi || !drcs || !dval) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(dimg, img, (size_t)img_bytes_per_px * npx, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dk, kernels, sizeof(double) * (size_t)nw, hipMemcpyHostToDevice, st));
    double *C0 = C, *C2 = C + npx;
    nw = 0;
    for (int s = 0; s < num_sigma; s++) {
        const int r = radius[s];
        const double *k0 = dk + nw, *k2 = k0 + 2 * r + 1;
        nw += 2 * (2 * r + 1);
        const dim3 gc((w + 63) / 64, (h + 4 * LOG_KC - 1) / (4 * LOG_KC));
        if (img_bytes_per_px == 4)
            hipLaunchKernelGGL(log_cols_kernel<float>, gc, dim3(256), 0, st, (const float *)dimg, h, w, r, k0, k2, C0, C2);
        else
            hipLaunchKernelGGL(log_cols_kernel<double>, gc, dim3(256), 0, st, (const double *)dimg, h, w, r, k0, k2, C0, C2);
        const size_t lds = sizeof(double) * 2 * (LOG_ROW_SPAN + 2 * (size_t)r);
        hipLaunchKernelGGL(log_rows_kernel, dim3((w + LOG_ROW_SPAN - 1) / LOG_ROW_SPAN, h), dim3(256), lds, st, C0, C2, h, w, r, k0, k2,
                           scale[s], Q + (size_t)s * npx);
        HIP_TRY(ctx, hipGetLastError());
    }
    int32_t *rowc = rowi, *rowk = rowi + h, *rowo = rowi + 2 * h, *dtotal = rowi + 3 * h, *dtriv = dtotal + 1;
    hipLaunchKernelGGL(log_maxima_kernel<false>, dim3(h), dim3(256), 0, st, Q, num_sigma, h, w, threshold, rowc, rowk, rowo, dtriv,
                       drcs, dval, cap);
    hipLaunchKernelGGL(log_row_scan_kernel, dim3(1), dim3(256), 0, st, Q, (int64_t)npx * num_sigma, rowc, rowk, h, rowo, dtotal, dtriv);
    hipLaunchKernelGGL(log_maxima_kernel<true>, dim3(h), dim3(256), 0, st, Q, num_sigma, h, w, threshold, rowc, rowk, rowo, dtriv,
                       drcs, dval, cap);
    HIP_TRY(ctx, hipGetLastError());
    int32_t n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, dtotal, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (out_layers) HIP_TRY(ctx, hipMemcpyAsync(out_layers, Q, sizeof(double) * npx * (size_t)num_sigma, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *n_out = n;
    const int m = n < cap ? n : cap;
    if (m > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(out_rcs, drcs, sizeof(int32_t) * 3 * (size_t)m, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out_val, dval, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    if (n > cap) { ROAM_SET_ERR(ctx, "log: %d maxima, capacity %d", n, cap); return ROAM_E_CAPACITY; }
    return ROAM_OK;
}
