// FMT.getTranslationUsingPhaseCorrelation (reference FMT.py:13-33: cv2.createHanningWindow + cv2.phaseCorrelate on two images of any
// shape) on the FFT of fft.hip: window and zero-pad into float64 planes of the optimal DFT size, two forward transforms, the normalised
// cross-power spectrum, the inverse transform, the peak and its 5 x 5 centroid.  pc_correlate is that core on filled planes: the
// Fourier-Mellin passes of fmt.hip run it on planes that the kernels of fmt_batch.hip and fmt_register.hip fill.  fft.h declares it.
#include "cvmap.h"
#include "fft.h"
#include <math.h>
#include <stdlib.h>

// ------------------------------------------------------------------------------------------------ phase correlation
// window (cv2.createHanningWindow: sqrt(float32(wr[y] wc[x])) from the float64 factors) times image, rounded to float32, zero-padded
// into the M x N float64 plane.  wr == null: no window.  grid (ceil(N / 256), M, batch)
__global__ __launch_bounds__(256) void pc_window_kernel(const float *__restrict__ img, int rows, int cols, const double *__restrict__ wr,
                                                        const double *__restrict__ wc, int M, int N, double *__restrict__ out)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= N) return;
    double val = 0.0;
    if (x < cols && y < rows) {
        const float v = img[((int64_t)b * rows + y) * cols + x];
        val = (double)(wr ? cv_hanning_product(wr[y], wc[x], v) : v);
    }
    out[((int64_t)b * M + y) * N + x] = val;
}

// normalised cross-power spectrum: mulSpectrums(F1, F2, conjB) then divSpectrums by its magnitude: P |P| / (|P|^2 + FLT_EPSILON)
static __global__ void fmt_cross_power_kernel(const double *__restrict__ r1, const double *__restrict__ i1, const double *__restrict__ r2,
                                              const double *__restrict__ i2, int n, double *__restrict__ cr, double *__restrict__ ci)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double pr = r1[k] * r2[k] + i1[k] * i2[k], pi = i1[k] * r2[k] - r1[k] * i2[k];
    const double mag = sqrt(pr * pr + pi * pi), den = mag * mag + 1.1920928955078125e-07;
    cr[k] = pr * mag / den; ci[k] = pi * mag / den;
}

// np.fft.fftshift: shifted[i] = plane[(i + n - n / 2) mod n]
__device__ __forceinline__ double pc_shifted(const double *__restrict__ c, int M, int N, int y, int x)
{
    int sy = y + M - M / 2, sx = x + N - N / 2;
    if (sy >= M) sy -= M;
    if (sx >= N) sx -= N;
    return c[(int64_t)sy * N + sx];
}

// stage 1 of the peak search: block (blk, b) scans the indices [blk per, (blk + 1) per) of plane b's SHIFTED image in row-major
// order and leaves its maximum and the lowest index that holds it
__global__ __launch_bounds__(256) void pc_peak_partial_kernel(const double *__restrict__ c, int M, int N, int per, double *__restrict__ pv,
                                                              int *__restrict__ pi)
{
    __shared__ double bv[256];
    __shared__ int bi[256];
    const int t = threadIdx.x, n = M * N, b = blockIdx.y;
    const double *pl = c + (int64_t)b * n;
    const int k0 = blockIdx.x * per, k1 = min(n, k0 + per);
    double best = -1e300; int besti = n;
    for (int k = k0 + t; k < k1; k += 256) {
        const int y = k / N, x = k - y * N;
        const double v = pc_shifted(pl, M, N, y, x);
        if (v > best) { best = v; besti = k; }
    }
    bv[t] = best; bi[t] = besti;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s && (bv[t + s] > bv[t] || (bv[t + s] == bv[t] && bi[t + s] < bi[t]))) { bv[t] = bv[t + s]; bi[t] = bi[t + s]; }
        __syncthreads();
    }
    if (t == 0) { pv[(int64_t)b * gridDim.x + blockIdx.x] = bv[0]; pi[(int64_t)b * gridDim.x + blockIdx.x] = bi[0]; }
}

// stage 2: the first maximum of plane b among its nblk partial results, then the 5 x 5 weighted centroid on the plane scaled by
// 1 / (M N) (the inverse transform is unscaled) -> out3[b] = {dx, dy, response}.  One workgroup per plane.
__global__ __launch_bounds__(256) void pc_peak_final_kernel(const double *__restrict__ c, int M, int N, int nblk, const double *__restrict__ pv,
                                                            const int *__restrict__ pi, double *__restrict__ out3)
{
    __shared__ double bv[256];
    __shared__ int bi[256];
    const int t = threadIdx.x, n = M * N, b = blockIdx.x;
    const double *pl = c + (int64_t)b * n;
    double best = -1e300; int besti = n;
    for (int k = t; k < nblk; k += 256) {
        const double v = pv[(int64_t)b * nblk + k]; const int i = pi[(int64_t)b * nblk + k];
        if (v > best || (v == best && i < besti)) { best = v; besti = i; }
    }
    bv[t] = best; bi[t] = besti;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s && (bv[t + s] > bv[t] || (bv[t + s] == bv[t] && bi[t + s] < bi[t]))) { bv[t] = bv[t + s]; bi[t] = bi[t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        const int at = bi[0] < n ? bi[0] : 0;               // a plane without a finite value: the centroid of its corner (NaN out)
        const int py = at / N, px = at - py * N;
        const int r0 = max(py - 2, 0), r1 = min(py + 2, M - 1), c0 = max(px - 2, 0), c1 = min(px + 2, N - 1);
        const double inv = 1.0 / ((double)M * (double)N);
        double sx = 0, sy = 0, sum = 0;
        for (int y = r0; y <= r1; y++)
            for (int x = c0; x <= c1; x++) {
                const double v = pc_shifted(pl, M, N, y, x) * inv;
                sx += (double)x * v; sy += (double)y * v; sum += v;
            }
        const double den = sum + 2.220446049250313e-16;
        out3[3 * b + 0] = (double)N / 2.0 - sx / den;
        out3[3 * b + 1] = (double)M / 2.0 - sy / den;
        out3[3 * b + 2] = sum;
    }
}

// cv2.createHanningWindow's float64 factor per row or column of a side of n
void roam_hanning_factors(int n, double *w)
{
    for (int i = 0; i < n; i++) w[i] = 0.5 * (1.0 - cos(2.0 * M_PI / (double)(n - 1) * (double)i));
}

size_t pc_chunk(size_t bytes_per_pair, size_t n, size_t cap, bool env)
{
    size_t chunk = ((size_t)2000 << 20) / bytes_per_pair;
    if (chunk < 1) chunk = 1;
    if (chunk > n) chunk = n;
    if (chunk > cap) chunk = cap;
    if (const char *ce = env ? getenv("ROAM_FMT_BATCH_CHUNK") : nullptr) {
        const long c = atol(ce);
        if (c >= 1 && (size_t)c < chunk) chunk = (size_t)c;
    }
    return chunk;
}

// Per image set a row pass, a transpose and a row pass (the spectrum stays transposed, N x M); the cross-power spectrum; the three
// inverse passes; the peak search
int32_t pc_correlate(roam_ctx *ctx, hipStream_t st, int nb, int M, int N, const PcWork &w, const double *win0, const double *win1)
{
    const size_t pl = (size_t)M * N * nb;
    const PcPlanes p = pc_planes(w.f, pl);
    const PcPeakGrid g = pc_peak_grid((size_t)M * N);
    double *const a = p.a, *const tr = p.tr, *const ti = p.ti;
    const double *win[2] = {win0, win1};
    for (int k = 0; k < 2; k++) {
        FFT_TRY(fft_rows(ctx, st, win[k], nullptr, tr, ti, (int64_t)nb * M, N, false));
        FFT_TRY(fft_transpose(ctx, st, tr, ti, nb, M, N, p.F[k][0], p.F[k][1]));
        FFT_TRY(fft_rows(ctx, st, p.F[k][0], p.F[k][1], p.F[k][0], p.F[k][1], (int64_t)nb * N, M, false));       // spectrum, N x M
    }
    hipLaunchKernelGGL(fmt_cross_power_kernel, dim3((unsigned)((pl + 255) / 256)), dim3(256), 0, st, p.F[0][0], p.F[0][1], p.F[1][0], p.F[1][1],
                       (int)pl, tr, ti);
    HIP_TRY(ctx, hipGetLastError());
    FFT_TRY(fft_rows(ctx, st, tr, ti, tr, ti, (int64_t)nb * N, M, true));
    FFT_TRY(fft_transpose(ctx, st, tr, ti, nb, N, M, p.F[0][0], p.F[0][1]));
    FFT_TRY(fft_rows(ctx, st, p.F[0][0], p.F[0][1], a, nullptr, (int64_t)nb * M, N, true));                      // real part only
    hipLaunchKernelGGL(pc_peak_partial_kernel, dim3(g.nblk, nb), dim3(256), 0, st, a, M, N, g.per, w.pv, w.pi);
    hipLaunchKernelGGL(pc_peak_final_kernel, dim3(nb), dim3(256), 0, st, a, M, N, g.nblk, w.pv, w.pi, w.out);
    HIP_TRY(ctx, hipGetLastError());
    return ROAM_OK;
}

extern "C" int32_t roam_phase_correlate_f32(roam_ctx *ctx, const float *src, const float *tgt, int32_t batch, int32_t rows, int32_t cols,
                                            int64_t row_stride, int64_t image_stride, int32_t hanning, double *out_dxdy, double *out_response)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, src && tgt && out_dxdy && batch >= 1);
    ARG_CHECK(ctx, rows >= 2 && rows <= FFT_MAX_N && cols >= 2 && cols <= FFT_MAX_N);
    ARG_CHECK(ctx, row_stride >= cols && (batch == 1 || image_stride >= (int64_t)(rows - 1) * row_stride + cols));
    const int M = optimal_dft_size(rows), N = optimal_dft_size(cols);
    const size_t nmn = (size_t)M * N, nimg = (size_t)rows * cols;
    // per pair: the 7 float64 planes and the two float32 images
    const size_t chunk = pc_chunk(7 * sizeof(double) * nmn + 2 * sizeof(float) * nimg, batch, 32768, false);
    const PcWorkBytes wb = pc_work_bytes(nmn, chunk);
    hipStream_t st = ctx->stream;
    float *d_src = (float *)roam_scratch(ctx, S_IN0, sizeof(float) * nimg * chunk);
    float *d_tgt = (float *)roam_scratch(ctx, S_IN1, sizeof(float) * nimg * chunk);
    double *d_win = (double *)roam_scratch(ctx, S_TMP1, sizeof(double) * ((size_t)rows + cols));
    Slab count{nullptr};
    pc_work_take(count, wb);
    Slab slab{(uint8_t *)roam_scratch(ctx, S_TMP2, count.off)};
    const PcWork w = pc_work_take(slab, wb);
    if (!d_src || !d_tgt || !d_win || !slab.base) return ROAM_E_HIP;
    std::vector<double> win((size_t)rows + cols), o(3 * chunk);
    if (hanning) {
        roam_hanning_factors(rows, win.data());
        roam_hanning_factors(cols, win.data() + rows);
        HIP_TRY(ctx, hipMemcpyAsync(d_win, win.data(), sizeof(double) * win.size(), hipMemcpyHostToDevice, st));
    }
    for (size_t b0 = 0; b0 < (size_t)batch; b0 += chunk) {
        const int nb = (int)(((size_t)batch - b0) < chunk ? ((size_t)batch - b0) : chunk);
        const PcPlanes p = pc_planes(w.f, nmn * nb);
        double *wpl[2] = {p.a, p.F[1][0]};                   // the windowed images: sources, targets
        const float *host[2] = {src, tgt};
        float *dev[2] = {d_src, d_tgt};
        for (int k = 0; k < 2; k++) {
            HIP_TRY(ctx, roam_upload_packed_f32(st, dev[k], host[k] + (int64_t)b0 * image_stride, nb, cols, rows, row_stride, image_stride));
            hipLaunchKernelGGL(pc_window_kernel, dim3((N + 255) / 256, M, nb), dim3(256), 0, st, dev[k], rows, cols,
                               hanning ? d_win : (const double *)nullptr, d_win + rows, M, N, wpl[k]);
            HIP_TRY(ctx, hipGetLastError());
        }
        FFT_TRY(pc_correlate(ctx, st, nb, M, N, w, wpl[0], wpl[1]));
        HIP_TRY(ctx, hipMemcpyAsync(o.data(), w.out, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int i = 0; i < nb; i++) {
            out_dxdy[2 * (b0 + i)] = o[3 * i]; out_dxdy[2 * (b0 + i) + 1] = o[3 * i + 1];
            if (out_response) out_response[b0 + i] = o[3 * i + 2];
        }
    }
    return ROAM_OK;
}
