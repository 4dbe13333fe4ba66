// Mixed-radix FFT (complex float64, n = 2^a 3^b 5^c <= 4096) and FMT.getTranslationUsingPhaseCorrelation (reference FMT.py:13-33:
// cv2.createHanningWindow + cv2.phaseCorrelate on two images of any shape) on top of it.  docs/KERNELS.md "FFT" has the structure.
//
//   rows:     fft_rows_kernel transforms whole rows in LDS.  Stockham autosort, radix 4 / 2 / 3 / 5, ONE buffer of 4096 complex
//             (real and imaginary parts in two arrays of doubles, 64 KB per workgroup; 512 threads): a stage reads the
//             inputs of all of a thread's butterflies into registers, the workgroup meets at a barrier, and only then are the
//             outputs written to their permuted places.  Rows shorter than 2048 share a workgroup (2048 / n of them).
//   columns:  a tiled transpose through LDS (fft_transpose_kernel, 32 x 32 tiles, both sides coalesced) and the row kernel again.
//             The forward transform of phase correlation leaves the spectrum transposed (N x M); the cross-power spectrum is
//             element-wise, and the inverse transform starts from that layout (columns first), so a 2-D transform costs ONE transpose.
//   twiddles: cos / sin of 2 pi m / n, m = 0 .. n - 1, made on the host in long double, one table per (context, length), uploaded on
//             first use.  A butterfly's twiddle index r k n / (Ns R) is an exact integer below n: no angle is reduced on the device.
//   inverse:  unscaled (cv2.idft without DFT_SCALE) as swap(FFT(swap(x))), swap = exchange of real and imaginary part: the launcher
//             exchanges the plane pointers, the kernel is the forward one.
// The rotation prior (roam_fmt_rotation, roam_fmt_rotation_batch_f32, roam_engine_fmt_rotation) runs the same correlation on planes that
// the kernels of fmt_batch.hip fill: its driver roam_fmt_batch_run is here because the row pass and the transpose are local to this unit.
// roam_fmt_rotation is n = 1 of it.
// The registration (roam_fmt_register_batch_f32, roam_engine_fmt_register) adds a second correlation, on the Cartesian images that the
// kernels of fmt_register.hip make and turn by the angle of the first: roam_fmt_register_run.
// Both halves are enqueue-only cores (fmt_rot_enqueue, fmt_trans_enqueue) that the blocking entries and the engine's in-step pass
// (roam_fmt_auto_enqueue, for roam_engine_set_auto_prior) share.
#include "cvmap.h"
#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <new>

#define FFT_MAX_N 4096
#define FFT_THREADS 512
#define FFT_MAX_STAGES 12
#ifndef FFT_SHARE_ELEMS
#define FFT_SHARE_ELEMS 2048            // rows shorter than this share a workgroup
#endif

struct FftPlan {
    int n, nstages;
    int radix[FFT_MAX_STAGES];
};

struct FftTwiddle {
    int n;
    double *cs;                         // device: cos[n] then sin[n]
};
struct FftTwiddles {
    std::vector<FftTwiddle> tables;
};

static bool fft_plan(int n, FftPlan *p)
{
    p->n = n; p->nstages = 0;
    if (n < 1 || n > FFT_MAX_N) return false;
    int m = n;
    // odd radices first: a stage's writes have stride R doubles while Ns < 16, conflict-free on the LDS banks only for odd R
    while (m % 5 == 0) { p->radix[p->nstages++] = 5; m /= 5; }
    while (m % 3 == 0) { p->radix[p->nstages++] = 3; m /= 3; }
    int twos = 0;
    for (int t = m; t % 2 == 0; t /= 2) twos++;
    if (twos & 1) { p->radix[p->nstages++] = 2; m /= 2; }
    while (m % 4 == 0) { p->radix[p->nstages++] = 4; m /= 4; }
    return m == 1;
}

void roam_fft_release(roam_ctx *ctx)
{
    if (!ctx->fft_tw) return;
    for (auto &t : ctx->fft_tw->tables) (void)hipFree(t.cs);
    delete ctx->fft_tw;
    ctx->fft_tw = nullptr;
}

static const double *fft_twiddles(roam_ctx *ctx, int n)
{
    if (!ctx->fft_tw) ctx->fft_tw = new FftTwiddles();
    for (auto &t : ctx->fft_tw->tables) if (t.n == n) return t.cs;
    std::vector<double> h(2 * (size_t)n);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int m = 0; m < n; m++) {
        const long double a = two_pi * (long double)m / (long double)n;
        h[m] = (double)cosl(a); h[n + m] = (double)sinl(a);
    }
    FftTwiddle t{n, nullptr};
    if (hipMalloc((void **)&t.cs, sizeof(double) * h.size()) != hipSuccess ||
        hipMemcpy(t.cs, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice) != hipSuccess) {
        ROAM_SET_ERR(ctx, "twiddle table of length %d: allocation or upload failed", n);
        if (t.cs) (void)hipFree(t.cs);
        return nullptr;
    }
    ctx->fft_tw->tables.push_back(t);
    return t.cs;
}

// forward DFT of R points in place (w = exp(-2 pi i / R))
template <int R> __device__ __forceinline__ void fft_butterfly(double *xr, double *xi);

template <> __device__ __forceinline__ void fft_butterfly<2>(double *xr, double *xi)
{
    const double ar = xr[0], ai = xi[0];
    xr[0] = ar + xr[1]; xi[0] = ai + xi[1];
    xr[1] = ar - xr[1]; xi[1] = ai - xi[1];
}

template <> __device__ __forceinline__ void fft_butterfly<3>(double *xr, double *xi)
{
    const double s60 = 0.86602540378443864676;
    const double sr = xr[1] + xr[2], si = xi[1] + xi[2], dr = xr[1] - xr[2], di = xi[1] - xi[2];
    const double mr = xr[0] - 0.5 * sr, mi = xi[0] - 0.5 * si, er = s60 * di, ei = -(s60 * dr);
    xr[0] = xr[0] + sr; xi[0] = xi[0] + si;
    xr[1] = mr + er; xi[1] = mi + ei;
    xr[2] = mr - er; xi[2] = mi - ei;
}

template <> __device__ __forceinline__ void fft_butterfly<4>(double *xr, double *xi)
{
    const double t0r = xr[0] + xr[2], t0i = xi[0] + xi[2], t1r = xr[0] - xr[2], t1i = xi[0] - xi[2];
    const double t2r = xr[1] + xr[3], t2i = xi[1] + xi[3], t3r = xr[1] - xr[3], t3i = xi[1] - xi[3];
    xr[0] = t0r + t2r; xi[0] = t0i + t2i;
    xr[2] = t0r - t2r; xi[2] = t0i - t2i;
    xr[1] = t1r + t3i; xi[1] = t1i - t3r;
    xr[3] = t1r - t3i; xi[3] = t1i + t3r;
}

template <> __device__ __forceinline__ void fft_butterfly<5>(double *xr, double *xi)
{
    const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410, s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;
    const double p1r = xr[1] + xr[4], p1i = xi[1] + xi[4], p2r = xr[2] + xr[3], p2i = xi[2] + xi[3];
    const double d1r = xr[1] - xr[4], d1i = xi[1] - xi[4], d2r = xr[2] - xr[3], d2i = xi[2] - xi[3];
    const double m1r = xr[0] + (c1 * p1r + c2 * p2r), m1i = xi[0] + (c1 * p1i + c2 * p2i);
    const double m2r = xr[0] + (c2 * p1r + c1 * p2r), m2i = xi[0] + (c2 * p1i + c1 * p2i);
    const double n1r = s1 * d1r + s2 * d2r, n1i = s1 * d1i + s2 * d2i;
    const double n2r = s2 * d1r - s1 * d2r, n2i = s2 * d1i - s1 * d2i;
    xr[0] = xr[0] + (p1r + p2r); xi[0] = xi[0] + (p1i + p2i);
    xr[1] = m1r + n1i; xi[1] = m1i - n1r;
    xr[4] = m1r - n1i; xi[4] = m1i + n1r;
    xr[2] = m2r + n2i; xi[2] = m2i - n2r;
    xr[3] = m2r - n2i; xi[3] = m2i + n2r;
}

// one Stockham stage of radix R over `rows_here` rows of length n held in sr / si; Ns = the product of the radices already done.
// butterfly j of a row reads x[j + r n / R], multiplies by w^(r k), k = j mod Ns, w = exp(-2 pi i / (Ns R)), and writes
// y[(j / Ns) Ns R + k + r Ns].  All reads of the workgroup happen before its first write (one buffer).
template <int R>
__device__ __forceinline__ void fft_stage(double *sr, double *si, const double *__restrict__ twc, const double *__restrict__ tws,
                                          int n, int rows_here, int Ns)
{
    constexpr int NB = (FFT_MAX_N / R + FFT_THREADS - 1) / FFT_THREADS;
    const int q = n / R, nb = rows_here * q, tstep = n / (Ns * R);
    double vr[NB][R], vi[NB][R];
    int dst[NB];
#pragma unroll
    for (int u = 0; u < NB; u++) {
        const int b = (int)threadIdx.x + u * FFT_THREADS;
        dst[u] = -1;
        if (b < nb) {
            const int row = b / q, j = b - row * q, k = j % Ns;
            const int src = row * n + j;
            vr[u][0] = sr[src]; vi[u][0] = si[src];
#pragma unroll
            for (int r = 1; r < R; r++) {
                const double xr = sr[src + r * q], xi = si[src + r * q];
                const int m = r * k * tstep;
                const double c = twc[m], s = -tws[m];
                vr[u][r] = xr * c - xi * s; vi[u][r] = xr * s + xi * c;
            }
            fft_butterfly<R>(vr[u], vi[u]);
            dst[u] = row * n + (j - k) * R + k;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NB; u++)
        if (dst[u] >= 0) {
#pragma unroll
            for (int r = 0; r < R; r++) { sr[dst[u] + r * Ns] = vr[u][r]; si[dst[u] + r * Ns] = vi[u][r]; }
        }
    __syncthreads();
}

// forward FFT of total_rows contiguous rows of length plan.n; rows_per_wg rows per workgroup (rows_per_wg * n <= 4096).
// re_in or im_in may be null (zeros), re_out or im_out may be null (not stored); in and out may be the same planes.
__global__ __launch_bounds__(FFT_THREADS) void fft_rows_kernel(const double *re_in, const double *im_in, double *re_out, double *im_out,
                                                               int64_t total_rows, FftPlan plan, int rows_per_wg,
                                                               const double *__restrict__ twc, const double *__restrict__ tws)
{
    __shared__ double sr[FFT_MAX_N], si[FFT_MAX_N];
    const int n = plan.n, t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t left = total_rows - row0;
    const int rows_here = left < rows_per_wg ? (int)left : rows_per_wg;
    const int cnt = rows_here * n;
    const int64_t base = row0 * n;
    for (int i = t; i < cnt; i += FFT_THREADS) {
        sr[i] = re_in ? re_in[base + i] : 0.0;
        si[i] = im_in ? im_in[base + i] : 0.0;
    }
    __syncthreads();
    int Ns = 1;
    for (int s = 0; s < plan.nstages; s++) {
        const int R = plan.radix[s];
        if (R == 4) fft_stage<4>(sr, si, twc, tws, n, rows_here, Ns);
        else if (R == 2) fft_stage<2>(sr, si, twc, tws, n, rows_here, Ns);
        else if (R == 3) fft_stage<3>(sr, si, twc, tws, n, rows_here, Ns);
        else fft_stage<5>(sr, si, twc, tws, n, rows_here, Ns);
        Ns *= R;
    }
    for (int i = t; i < cnt; i += FFT_THREADS) {
        if (re_out) re_out[base + i] = sr[i];
        if (im_out) im_out[base + i] = si[i];
    }
}

// (batch) M x N -> N x M, both planes; block (32, 8), grid (ceil(N / 32), ceil(M / 32), batch)
__global__ __launch_bounds__(256) void fft_transpose_kernel(const double *__restrict__ re_in, const double *__restrict__ im_in, int M, int N,
                                                            double *__restrict__ re_out, double *__restrict__ im_out)
{
    __shared__ double tr[32][33], ti[32][33];
    const int64_t plane = (int64_t)blockIdx.z * M * N;
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    for (int dy = threadIdx.y; dy < 32; dy += 8) {
        const int x = x0 + threadIdx.x, y = y0 + dy;
        if (x < N && y < M) { tr[dy][threadIdx.x] = re_in[plane + (int64_t)y * N + x]; ti[dy][threadIdx.x] = im_in[plane + (int64_t)y * N + x]; }
    }
    __syncthreads();
    for (int dx = threadIdx.y; dx < 32; dx += 8) {
        const int y = y0 + threadIdx.x, x = x0 + dx;
        if (x < N && y < M) { re_out[plane + (int64_t)x * M + y] = tr[threadIdx.x][dx]; im_out[plane + (int64_t)x * M + y] = ti[threadIdx.x][dx]; }
    }
}

static int32_t fft_rows(roam_ctx *ctx, hipStream_t st, const double *re_in, const double *im_in, double *re_out, double *im_out, int64_t total_rows, int n,
                        bool inverse)
{
    FftPlan plan;
    if (!fft_plan(n, &plan)) { ROAM_SET_ERR(ctx, "FFT length %d is not 2^a 3^b 5^c <= %d", n, FFT_MAX_N); return ROAM_E_ARG; }
    const double *tw = fft_twiddles(ctx, n);
    if (!tw) return ROAM_E_HIP;
    int rpw = FFT_SHARE_ELEMS / n;
    if (rpw < 1) rpw = 1;
    const int64_t groups = (total_rows + rpw - 1) / rpw;
    if (inverse) { const double *ti = re_in; re_in = im_in; im_in = ti; double *to = re_out; re_out = im_out; im_out = to; }
    hipLaunchKernelGGL(fft_rows_kernel, dim3((unsigned)groups), dim3(FFT_THREADS), 0, st, re_in, im_in, re_out, im_out, total_rows, plan,
                       rpw, tw, tw + n);
    HIP_TRY(ctx, hipGetLastError());
    return ROAM_OK;
}

static int32_t fft_transpose(roam_ctx *ctx, hipStream_t st, const double *re_in, const double *im_in, int batch, int M, int N, double *re_out, double *im_out)
{
    hipLaunchKernelGGL(fft_transpose_kernel, dim3((N + 31) / 32, (M + 31) / 32, batch), dim3(32, 8), 0, st, re_in, im_in, M, N, re_out,
                       im_out);
    HIP_TRY(ctx, hipGetLastError());
    return ROAM_OK;
}

#define FFT_TRY(call) do { const int32_t rc_ = (call); if (rc_ != ROAM_OK) return rc_; } while (0)

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

static bool fft_smooth(int n)
{
    FftPlan p;
    return fft_plan(n, &p);
}

// cv2.getOptimalDFTSize: the smallest 2^a 3^b 5^c >= n
static int optimal_dft_size(int n)
{
    int best = 0;
    for (long p2 = 1; p2 < 2L * n; p2 *= 2)
        for (long p3 = p2; p3 < 2L * n; p3 *= 3)
            for (long p5 = p3; p5 < 2L * n; p5 *= 5)
                if (p5 >= n && (best == 0 || p5 < best)) best = (int)p5;
    return best;
}

// cv2.createHanningWindow's float64 factor per row or column of a side of n
void roam_hanning_factors(int n, double *w)
{
    for (int i = 0; i < n; i++) w[i] = 0.5 * (1.0 - cos(2.0 * M_PI / (double)(n - 1) * (double)i));
}

// the 7 nb planes of a chunk of nb correlations, pl = nb M N doubles each: windowed image | work re, im | F1 re, im | F2 re, im
struct PcPlanes {
    double *a, *tr, *ti, *F[2][2];
};
static PcPlanes pc_planes(double *base, size_t pl)
{
    return {base, base + pl, base + 2 * pl, {{base + 3 * pl, base + 4 * pl}, {base + 5 * pl, base + 6 * pl}}};
}

// the grid of pc_peak_partial_kernel: indices per block, blocks per plane (at most 1024)
struct PcPeakGrid {
    int per, nblk;
};
static PcPeakGrid pc_peak_grid(size_t nmn)
{
    const int per = (int)((nmn + 1023) / 1024) < 1024 ? 1024 : (int)((nmn + 1023) / 1024);
    return {per, (int)((nmn + per - 1) / per)};
}

// pairs per chunk: 2000 MiB of scratch at bytes_per_pair, at least one, at most n and cap (the grid's z extent).  env: the tests' smaller
// chunk from ROAM_FMT_BATCH_CHUNK (read per call)
static size_t pc_chunk(size_t bytes_per_pair, size_t n, size_t cap, bool env)
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

// The correlation of nb pairs, 12 launches on st: win[0] / win[1] hold the nb windowed, zero-padded M x N sources / targets
// (planes of `base`: a, and F2 re - which nothing touches before its own row pass has consumed it).  Per image set a row pass, a
// transpose and a row pass (the spectrum stays transposed, N x M); the cross-power spectrum; the three inverse passes; the peak search
// -> d_out[3 b] = {dx, dy, response}.  d_pv, d_pi: nb x pc_peak_grid(M N).nblk partial maxima
static int32_t pc_correlate(roam_ctx *ctx, hipStream_t st, int nb, int M, int N, double *base, const double *win0, const double *win1, double *d_pv,
                            int *d_pi, double *d_out)
{
    const size_t pl = (size_t)M * N * nb;
    const PcPlanes p = pc_planes(base, pl);
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
    hipLaunchKernelGGL(pc_peak_partial_kernel, dim3(g.nblk, nb), dim3(256), 0, st, a, M, N, g.per, d_pv, d_pi);
    hipLaunchKernelGGL(pc_peak_final_kernel, dim3(nb), dim3(256), 0, st, a, M, N, g.nblk, d_pv, d_pi, d_out);
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
    const int nblk = pc_peak_grid(nmn).nblk;
    hipStream_t st = ctx->stream;
    float *d_src = (float *)roam_scratch(ctx, S_IN0, sizeof(float) * nimg * chunk);
    float *d_tgt = (float *)roam_scratch(ctx, S_IN1, sizeof(float) * nimg * chunk);
    double *d_f = (double *)roam_scratch(ctx, S_TMP2, sizeof(double) * nmn * 7 * chunk);
    double *d_win = (double *)roam_scratch(ctx, S_TMP1, sizeof(double) * ((size_t)rows + cols));
    double *d_pv = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * (size_t)nblk * chunk);
    int *d_pi = (int *)roam_scratch(ctx, S_TMP3, sizeof(int) * (size_t)nblk * chunk);
    double *d_out = (double *)roam_scratch(ctx, S_OUT0, sizeof(double) * 3 * chunk);
    if (!d_src || !d_tgt || !d_f || !d_win || !d_pv || !d_pi || !d_out) return ROAM_E_HIP;
    std::vector<double> win((size_t)rows + cols), o(3 * chunk);
    if (hanning) {
        roam_hanning_factors(rows, win.data());
        roam_hanning_factors(cols, win.data() + rows);
        HIP_TRY(ctx, hipMemcpyAsync(d_win, win.data(), sizeof(double) * win.size(), hipMemcpyHostToDevice, st));
    }
    for (size_t b0 = 0; b0 < (size_t)batch; b0 += chunk) {
        const int nb = (int)(((size_t)batch - b0) < chunk ? ((size_t)batch - b0) : chunk);
        const PcPlanes p = pc_planes(d_f, nmn * nb);
        double *wpl[2] = {p.a, p.F[1][0]};                   // the windowed images: sources, targets
        const float *host[2] = {src, tgt};
        float *dev[2] = {d_src, d_tgt};
        for (int k = 0; k < 2; k++) {
            HIP_TRY(ctx, roam_upload_packed_f32(st, dev[k], host[k] + (int64_t)b0 * image_stride, nb, cols, rows, row_stride, image_stride));
            hipLaunchKernelGGL(pc_window_kernel, dim3((N + 255) / 256, M, nb), dim3(256), 0, st, dev[k], rows, cols,
                               hanning ? d_win : (const double *)nullptr, d_win + rows, M, N, wpl[k]);
            HIP_TRY(ctx, hipGetLastError());
        }
        FFT_TRY(pc_correlate(ctx, st, nb, M, N, d_f, wpl[0], wpl[1], d_pv, d_pi, d_out));
        HIP_TRY(ctx, hipMemcpyAsync(o.data(), d_out, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int i = 0; i < nb; i++) {
            out_dxdy[2 * (b0 + i)] = o[3 * i]; out_dxdy[2 * (b0 + i) + 1] = o[3 * i + 1];
            if (out_response) out_response[b0 + i] = o[3 * i + 2];
        }
    }
    return ROAM_OK;
}

// ------------------------------------------------------------------------------------------------ enqueue-only cores
// Both halves of the registration as work that is only enqueued: caller-owned device buffers, a caller-given stream, no host
// synchronisation and no allocation (the twiddle tables of the plane sizes excepted: they are made on first use, which the blocking
// entries accept and roam_fmt_auto_init forestalls).  The blocking entries below and the engine's in-step pass (roam_fmt_auto_enqueue)
// call these two and differ only in what stands between them: the host's libm or fmtr_angle_matrix_kernel.

// the log-polar size of the rotation half and its DFT plane
struct FmtRotSize {
    int dw, dh, M, N, sz;
    size_t tab_bytes;
};
// FMT.py:84-90: the base of the log-polar radius and the scale of a shift along it
static double fmt_log_base(const FmtRotSize &g) { return exp(log((double)g.dh / 2.0) / (double)g.sz); }
static double fmt_scale(double log_base, double shift_x) { return pow(log_base, shift_x); }
static FmtRotSize fmt_rot_size(int R)
{
    FmtRotSize g;
    g.dw = (int)rint((double)R); g.dh = (int)rint((double)R * M_PI);
    g.M = optimal_dft_size(g.dh); g.N = optimal_dft_size(g.dw);
    g.sz = g.dh > g.dw ? g.dh : g.dw;
    g.tab_bytes = sizeof(double) * (3 * (size_t)g.dh + g.dw) + sizeof(float) * g.dw;
    return g;
}

// OpenCV's host tables of the forward warpPolar (Kmag and Kangle from the destination size) and createHanningWindow's factors:
// cos, sin per row (2 dh doubles) | window per row (dh) | per column (dw) | radius per column (dw floats)
static void fmt_rot_tables(const FmtRotSize &g, int R, unsigned char *tab)
{
    double *cs = (double *)tab, *wr = cs + 2 * g.dh, *wc = wr + g.dh;
    roam_warp_polar_tables(g.dw, g.dh, (double)(2 * R) / 2.0, true, (float *)(wc + g.dw), cs);
    roam_hanning_factors(g.dh, wr);
    roam_hanning_factors(g.dw, wc);
}

// rotation half of nb pairs (src: nb sources, then nb targets): front end of fmt_batch.hip, correlation -> d_out[3 b] = {shift_x,
// shift_y, response}.  d_tab: fmt_rot_tables on the device; d_f: 7 nb planes of M x N doubles; d_lp optional
static int32_t fmt_rot_enqueue(roam_ctx *ctx, hipStream_t st, const FmtBatchSrc &src, int nb, int rows, int clip, int R, const FmtRotSize &g,
                               const unsigned char *d_tab, float *d_small, float *d_cart, double *d_f, float *d_lp, double *d_pv, int *d_pi,
                               double *d_out)
{
    const double *d_tabd = (const double *)d_tab;
    const float *d_br = (const float *)(d_tabd + 3 * (size_t)g.dh + g.dw);
    const PcPlanes p = pc_planes(d_f, (size_t)g.M * g.N * nb);
    HIP_TRY(ctx, launch_fmt_batch_front(st, src, nb, rows, clip, R, g.dw, g.dh, g.M, g.N, d_tabd, d_br, d_small, d_cart, d_f, (int64_t)4 * nb, d_lp));
    return pc_correlate(ctx, st, nb, g.M, g.N, d_f, p.a, p.F[1][0], d_pv, d_pi, d_out);         // the windowed images: sources, targets
}

// translation half of nb pairs: the Cartesian images (2 nb x S x S, S = 2 Rc), the sources turned by d_M (6 doubles per pair,
// destination -> source), the window (d_win: S row factors, then S column factors), the correlation on M x M planes -> d_out[3 b] =
// {dx, dy, response}.  d_rot optional: the turned sources before the window
static int32_t fmt_trans_enqueue(roam_ctx *ctx, hipStream_t st, const FmtBatchSrc &src, int nb, int rows, int cols, int Rc, int M, float *d_cart,
                                 const double *d_M, const double *d_win, double *d_f, float *d_rot, double *d_pv, int *d_pi, double *d_out)
{
    const PcPlanes p = pc_planes(d_f, (size_t)M * M * nb);
    HIP_TRY(ctx, launch_fmtr_cart(st, src, 2 * nb, rows, cols, Rc, d_cart));
    HIP_TRY(ctx, launch_fmtr_rotate_window(st, d_cart, 2 * Rc, M, M, nb, (int64_t)4 * nb, d_M, d_win, d_f, d_rot));
    return pc_correlate(ctx, st, nb, M, M, d_f, p.a, p.F[1][0], d_pv, d_pi, d_out);             // the windowed images: turned sources, targets
}

// bytes of device memory per pair of the two halves on resident records (the planes of each half are counted: a chunk of the
// registration is one chunk of the rotation pass too)
static size_t fmt_rot_bytes_per_pair(int rows, int R)
{
    const FmtRotSize g = fmt_rot_size(R);
    return 7 * sizeof(double) * (size_t)g.M * g.N + 2 * sizeof(float) * ((size_t)rows * R + (size_t)(2 * R) * (2 * R)) + 2 * sizeof(int32_t);
}

// ------------------------------------------------------------------------------------------------ batched rotation prior
// FMT.getRotationUsingFMT for n pairs: the front end of fmt_batch.hip fills the planes, the correlation is the one above.  Per chunk of
// nb pairs, 7 nb planes: sources' windowed images | work re, im | F1 re, im | F2 re, im - the targets' windowed images wait in the
// F2 re planes, which nothing touches before their own row pass has consumed them.  One stream synchronisation per chunk.
int32_t roam_fmt_batch_run(roam_ctx *ctx, const FmtBatchIn &in, int n, int rows, int clip, int R, double *out3, float *logpolar_out)
{
    const FmtRotSize g = fmt_rot_size(R);
    const int W = 2 * R, dw = g.dw, dh = g.dh, M = g.M, N = g.N;
    ARG_CHECK(ctx, M <= FFT_MAX_N && N <= FFT_MAX_N);
    const bool host = in.host_src != nullptr;
    const size_t nmn = (size_t)M * N, nsmall = (size_t)rows * R, ncart = (size_t)W * W, nlp = (size_t)dh * dw;
    // a host image travels as whole rows when they are contiguous (one copy per image, or one per chunk), else as its first clip columns
    const bool whole_rows = host && in.row_stride == in.cols;
    const size_t in_w = whole_rows ? (size_t)in.cols : (size_t)clip, nin = host ? (size_t)rows * in_w : 0;
    const size_t per_pair = 7 * sizeof(double) * nmn + 2 * sizeof(float) * (nsmall + ncart + (logpolar_out ? nlp : 0) + nin) + 2 * sizeof(int32_t);
    const size_t chunk = pc_chunk(per_pair, n, 32767, true);                 // 2 chunk images in grid.z
    const int nblk = pc_peak_grid(nmn).nblk;
    hipStream_t st = ctx->stream;
    float *d_in = host ? (float *)roam_scratch(ctx, S_IN0, sizeof(float) * nin * 2 * chunk) : nullptr;
    int32_t *d_idx = host ? nullptr : (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * 2 * chunk);
    float *d_small = (float *)roam_scratch(ctx, S_TMP4, sizeof(float) * nsmall * 2 * chunk);
    float *d_cart = (float *)roam_scratch(ctx, S_TMP5, sizeof(float) * ncart * 2 * chunk);
    float *d_lp = logpolar_out ? (float *)roam_scratch(ctx, S_TMP6, sizeof(float) * nlp * 2 * chunk) : nullptr;
    double *d_f = (double *)roam_scratch(ctx, S_TMP2, sizeof(double) * nmn * 7 * chunk);
    const size_t tab_bytes = g.tab_bytes;
    unsigned char *d_tab = (unsigned char *)roam_scratch(ctx, S_TMP1, tab_bytes);
    double *d_pv = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * (size_t)nblk * chunk);
    int *d_pi = (int *)roam_scratch(ctx, S_TMP3, sizeof(int) * (size_t)nblk * chunk);
    double *d_out = (double *)roam_scratch(ctx, S_OUT0, sizeof(double) * 3 * chunk);
    if ((host && !d_in) || (!host && !d_idx) || !d_small || !d_cart || (logpolar_out && !d_lp) || !d_f || !d_tab || !d_pv || !d_pi || !d_out)
        return ROAM_E_HIP;
    std::vector<unsigned char> tab(tab_bytes);
    fmt_rot_tables(g, R, tab.data());
    HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, st));
    std::vector<double> o(3 * chunk);
    const int sz = g.sz;
    const double log_base = fmt_log_base(g);
    for (size_t b0 = 0; b0 < (size_t)n; b0 += chunk) {
        const int nb = (int)(((size_t)n - b0) < chunk ? ((size_t)n - b0) : chunk);
        FmtBatchSrc src;
        if (host) {
            const float *h[2] = {in.host_src, in.host_tgt};
            for (int k = 0; k < 2; k++)
                HIP_TRY(ctx, roam_upload_packed_f32(st, d_in + (size_t)k * nb * nin, h[k] + (int64_t)b0 * in.image_stride, nb, (int)in_w, rows,
                                                    in.row_stride, in.image_stride));
            src = {d_in, (int64_t)nin, (int64_t)in_w, 0, 0, nullptr};
        } else {
            HIP_TRY(ctx, hipMemcpyAsync(d_idx, in.prev_idx + b0, sizeof(int32_t) * nb, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_idx + nb, in.curr_idx + b0, sizeof(int32_t) * nb, hipMemcpyHostToDevice, st));
            src = {in.pool, in.rec_bytes, in.rec_stride, in.payload_off, in.pool_f32 ? 0 : 1, d_idx};
        }
        FFT_TRY(fmt_rot_enqueue(ctx, st, src, nb, rows, clip, R, g, d_tab, d_small, d_cart, d_f, d_lp, d_pv, d_pi, d_out));
        HIP_TRY(ctx, hipMemcpyAsync(o.data(), d_out, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost, st));
        if (logpolar_out) {
            HIP_TRY(ctx, hipMemcpyAsync(logpolar_out + b0 * nlp, d_lp, sizeof(float) * nlp * nb, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(logpolar_out + ((size_t)n + b0) * nlp, d_lp + (size_t)nb * nlp, sizeof(float) * nlp * nb,
                                        hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int i = 0; i < nb; i++) {                       // FMT.py:84-90: the shifts as an angle and a scale
            out3[3 * (b0 + i)] = roam_normalize_angle(-o[3 * i + 1] * 2.0 * M_PI / (double)sz);
            out3[3 * (b0 + i) + 1] = fmt_scale(log_base, o[3 * i]);
            out3[3 * (b0 + i) + 2] = o[3 * i + 2];
        }
    }
    return ROAM_OK;
}

// what the host entries of the rotation prior check alike: the image size and the downsampling, then clip = the range bins kept
// (clip_px <= 0 or >= cols: all of them) and R = clip / downsample, the columns after the resize
static int32_t fmt_clip_radius(roam_ctx *ctx, int rows, int cols, int clip_px, int downsample, int *clip, int *R)
{
    ARG_CHECK(ctx, rows >= 8 && rows <= 16384 && cols >= 2 && downsample >= 1);
    *clip = (clip_px > 0 && clip_px < cols) ? clip_px : cols;
    *R = *clip / downsample;
    ARG_CHECK(ctx, *R >= ROAM_FMT_MIN_R && *R <= ROAM_FMT_MAX_R);
    return ROAM_OK;
}

extern "C" int32_t roam_fmt_rotation_batch_f32(roam_ctx *ctx, const float *src, const float *tgt, int32_t n, int32_t rows, int32_t cols,
                                               int64_t row_stride, int64_t image_stride, int32_t clip_px, int32_t downsample, double *out3,
                                               float *logpolar_out)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, src && tgt && out3 && n >= 1);
    int clip, R;
    FFT_TRY(fmt_clip_radius(ctx, rows, cols, clip_px, downsample, &clip, &R));
    ARG_CHECK(ctx, row_stride >= cols && (n == 1 || image_stride >= (int64_t)(rows - 1) * row_stride + cols));
    FmtBatchIn in;
    in.host_src = src; in.host_tgt = tgt; in.row_stride = row_stride; in.image_stride = n == 1 ? (int64_t)rows * row_stride : image_stride;
    in.cols = cols;
    return roam_fmt_batch_run(ctx, in, n, rows, clip, R, out3, logpolar_out);
}

// one contiguous pair: n = 1 of the batch call
extern "C" int32_t roam_fmt_rotation(roam_ctx *ctx, const float *src_polar, const float *tgt_polar, int32_t rows, int32_t cols,
                                     int32_t clip_px, int32_t downsample, double *angle_rad, double *scale, double *response)
{
    if (!ctx) return ROAM_E_ARG;
    ARG_CHECK(ctx, src_polar && tgt_polar && angle_rad);
    int clip, R;
    FFT_TRY(fmt_clip_radius(ctx, rows, cols, clip_px, downsample, &clip, &R));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FmtBatchIn in;
    in.host_src = src_polar; in.host_tgt = tgt_polar; in.row_stride = cols; in.image_stride = (int64_t)rows * cols;
    in.cols = cols;
    double out3[3];
    FFT_TRY(roam_fmt_batch_run(ctx, in, 1, rows, clip, R, out3, nullptr));
    *angle_rad = out3[0];
    if (scale) *scale = out3[1];
    if (response) *response = out3[2];
    return ROAM_OK;
}

// ------------------------------------------------------------------------------------------------ batched registration
// Rotation, then translation, for n pairs (FMT.py:211-250, then rotateImg(prevImgCart, rotDeg) and a phase correlation of the turned
// source with the target).  Per chunk of nb pairs: roam_fmt_batch_run gives the angles and brings them to the host (first
// synchronisation); the host makes the nb inverse rotation matrices with its libm, as roam_warp_affine_f32 does; the kernels of
// fmt_register.hip make the 2 nb Cartesian images and fill the planes, laid out as in roam_fmt_batch_run; the correlation and the peak
// search are the ones above (second synchronisation).  Host images go up once, whole, and both halves read them on the device.
// The halves share S_TMP0 .. S_TMP3 and S_OUT0, one after the other: the second takes them (again) only after the first has returned,
// its results on the host.  What only this pass uses lies in slots that roam_fmt_batch_run does not touch.
int32_t roam_fmt_register_run(roam_ctx *ctx, const FmtBatchIn &in, int n, int rows, int clip, int R, int Rc, double *out6, float *cart_out)
{
    const int S = 2 * Rc;
    ARG_CHECK(ctx, S >= 2 && S <= FFT_MAX_N);
    const int M = optimal_dft_size(S), N = M;
    const bool host = in.host_src != nullptr;
    const size_t nmn = (size_t)M * N, ncart = (size_t)S * S, nin = host ? (size_t)rows * in.cols : 0;
    // the rotation half per pair, as roam_fmt_batch_run counts it for resident images, and this half (the shared planes count twice):
    // a chunk of this size is one chunk there too
    const size_t per_rot = fmt_rot_bytes_per_pair(rows, R);
    const size_t per_reg = 7 * sizeof(double) * nmn + sizeof(float) * (2 * ncart + (cart_out ? ncart : 0) + 2 * nin) + 6 * sizeof(double)
                           + 2 * sizeof(int32_t);
    const size_t chunk = pc_chunk(per_rot + per_reg, n, 32767, true);        // 2 chunk images in grid.z
    const int nblk = pc_peak_grid(nmn).nblk;
    hipStream_t st = ctx->stream;
    float *d_img = host ? (float *)roam_scratch(ctx, S_IN2, sizeof(float) * nin * 2 * chunk) : nullptr;
    int32_t *d_idx = host ? nullptr : (int32_t *)roam_scratch(ctx, S_IN3, sizeof(int32_t) * 2 * chunk);
    float *d_cart = (float *)roam_scratch(ctx, S_TMP7, sizeof(float) * ncart * 2 * chunk);
    float *d_rot = cart_out ? (float *)roam_scratch(ctx, S_OUT1, sizeof(float) * ncart * chunk) : nullptr;
    double *d_M = (double *)roam_scratch(ctx, S_OUT2, sizeof(double) * 6 * chunk);
    if ((host && !d_img) || (!host && !d_idx) || !d_cart || (cart_out && !d_rot) || !d_M) return ROAM_E_HIP;
    std::vector<double> win(2 * (size_t)S), o3(3 * chunk), o(3 * chunk), Mh(6 * chunk);
    roam_hanning_factors(S, win.data());
    roam_hanning_factors(S, win.data() + S);
    std::vector<int32_t> iota;
    if (host) {
        iota.resize(2 * chunk);
        for (size_t i = 0; i < 2 * chunk; i++) iota[i] = (int32_t)i;
    }
    for (size_t b0 = 0; b0 < (size_t)n; b0 += chunk) {
        const int nb = (int)(((size_t)n - b0) < chunk ? ((size_t)n - b0) : chunk);
        FmtBatchIn rin = in;
        FmtBatchSrc src;
        if (host) {
            const float *h[2] = {in.host_src, in.host_tgt};
            for (int k = 0; k < 2; k++)
                HIP_TRY(ctx, roam_upload_packed_f32(st, d_img + (size_t)k * nb * nin, h[k] + (int64_t)b0 * in.image_stride, nb, in.cols, rows,
                                                    in.row_stride, in.image_stride));
            rin = FmtBatchIn();
            rin.pool = (const uint8_t *)d_img; rin.rec_bytes = (int64_t)nin; rin.rec_stride = in.cols; rin.pool_f32 = 1;
            rin.prev_idx = iota.data(); rin.curr_idx = iota.data() + nb;
            src = {d_img, (int64_t)nin, (int64_t)in.cols, 0, 0, nullptr};
        } else {
            rin.prev_idx = in.prev_idx + b0; rin.curr_idx = in.curr_idx + b0;
            HIP_TRY(ctx, hipMemcpyAsync(d_idx, in.prev_idx + b0, sizeof(int32_t) * nb, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_idx + nb, in.curr_idx + b0, sizeof(int32_t) * nb, hipMemcpyHostToDevice, st));
            src = {in.pool, in.rec_bytes, in.rec_stride, in.payload_off, 1, d_idx};
        }
        FFT_TRY(roam_fmt_batch_run(ctx, rin, nb, rows, clip, R, o3.data(), nullptr));            // synchronises: the angles are here
        const double c = (double)(float)Rc;                  // getRotationMatrix2D's centre (w / 2, h / 2) as a cv::Point2f
        for (int i = 0; i < nb; i++) roam_rotation_inverse_map(c, c, o3[3 * i] * (180.0 / M_PI), &Mh[6 * (size_t)i]);
        double *d_f = (double *)roam_scratch(ctx, S_TMP2, sizeof(double) * nmn * 7 * chunk);
        double *d_win = (double *)roam_scratch(ctx, S_TMP1, sizeof(double) * win.size());
        double *d_pv = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * (size_t)nblk * chunk);
        int *d_pi = (int *)roam_scratch(ctx, S_TMP3, sizeof(int) * (size_t)nblk * chunk);
        double *d_out = (double *)roam_scratch(ctx, S_OUT0, sizeof(double) * 3 * chunk);
        if (!d_f || !d_win || !d_pv || !d_pi || !d_out) return ROAM_E_HIP;
        HIP_TRY(ctx, hipMemcpyAsync(d_win, win.data(), sizeof(double) * win.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_M, Mh.data(), sizeof(double) * 6 * nb, hipMemcpyHostToDevice, st));
        FFT_TRY(fmt_trans_enqueue(ctx, st, src, nb, rows, in.cols, Rc, M, d_cart, d_M, d_win, d_f, d_rot, d_pv, d_pi, d_out));
        HIP_TRY(ctx, hipMemcpyAsync(o.data(), d_out, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost, st));
        if (cart_out) {
            HIP_TRY(ctx, hipMemcpyAsync(cart_out + b0 * ncart, d_rot, sizeof(float) * ncart * nb, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(cart_out + ((size_t)n + b0) * ncart, d_cart + (size_t)nb * ncart, sizeof(float) * ncart * nb,
                                        hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int i = 0; i < nb; i++) {
            double *q = out6 + 6 * (b0 + i);
            q[0] = o3[3 * i]; q[1] = o3[3 * i + 1]; q[2] = o3[3 * i + 2];
            q[3] = o[3 * i]; q[4] = o[3 * i + 1]; q[5] = o[3 * i + 2];
        }
    }
    return ROAM_OK;
}

extern "C" int32_t roam_fmt_register_batch_f32(roam_ctx *ctx, const float *src, const float *tgt, int32_t n, int32_t rows, int32_t cols,
                                               int64_t row_stride, int64_t image_stride, int32_t clip_px, int32_t downsample,
                                               int32_t cart_downsample, double *out6, float *cart_out)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, src && tgt && out6 && n >= 1);
    int clip, R;
    FFT_TRY(fmt_clip_radius(ctx, rows, cols, clip_px, downsample, &clip, &R));
    ARG_CHECK(ctx, cols <= 16384 && cart_downsample >= 1);
    ARG_CHECK(ctx, row_stride >= cols && (n == 1 || image_stride >= (int64_t)(rows - 1) * row_stride + cols));
    const int Rc = cols / cart_downsample;
    ARG_CHECK(ctx, 2 * Rc >= 2 && 2 * Rc <= FFT_MAX_N);
    FmtBatchIn in;
    in.host_src = src; in.host_tgt = tgt; in.row_stride = row_stride; in.image_stride = n == 1 ? (int64_t)rows * row_stride : image_stride;
    in.cols = cols;
    return roam_fmt_register_run(ctx, in, n, rows, clip, R, Rc, out6, cart_out);
}

// ------------------------------------------------------------------------------------------------ in-step registration
// The registration as a part of roam_engine_step (roam_engine_set_auto_prior): the two cores above with fmtr_angle_matrix_kernel between
// them and fmtr_prior_kernel behind them, on a stream the engine gives, in buffers carved from one slab the engine allocated.  Nothing
// here synchronises or allocates once roam_fmt_auto_init has returned.
struct FmtAuto {
    FmtAutoCfg cfg;
    FmtAutoPlan plan;
    FmtRotSize g;
    int Mt;                             // DFT side of the translation half
    int32_t *h_idx = nullptr;           // pinned: 4 slots of 3 lanes ints (the chunks' index lists, then pair_of)
    int32_t *d_idx = nullptr;           // the same ring on the device
    unsigned char *d_tab = nullptr;
    double *d_win = nullptr, *d_f = nullptr, *d_pv = nullptr, *d_rot3 = nullptr, *d_trans3 = nullptr, *d_ang = nullptr, *d_M = nullptr;
    int *d_pi = nullptr;
    float *d_small = nullptr, *d_cart_r = nullptr, *d_cart_t = nullptr;
};

// the slab's parts in order, each on a 256-byte boundary; a null slab only counts
static size_t fmt_auto_carve(FmtAuto *a, const FmtAutoCfg &c, size_t chunk, uint8_t *slab)
{
    const FmtRotSize g = fmt_rot_size(c.R);
    const int S = 2 * c.Rc, Mt = optimal_dft_size(S);
    const size_t nmn_r = (size_t)g.M * g.N, nmn_t = (size_t)Mt * Mt, nmn = nmn_r > nmn_t ? nmn_r : nmn_t;
    const size_t nblk = (size_t)std::max(pc_peak_grid(nmn_r).nblk, pc_peak_grid(nmn_t).nblk), L = (size_t)c.lanes;
    size_t off = 0;
    auto take = [&](size_t bytes) { uint8_t *p = slab ? slab + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
    uint8_t *idx = take(sizeof(int32_t) * 4 * 3 * L), *tab = take(g.tab_bytes), *win = take(sizeof(double) * 2 * S);
    uint8_t *f = take(sizeof(double) * 7 * nmn * chunk), *pv = take(sizeof(double) * nblk * chunk), *pi = take(sizeof(int) * nblk * chunk);
    uint8_t *small = take(sizeof(float) * (size_t)c.rows * c.R * 2 * chunk), *cr = take(sizeof(float) * (size_t)(2 * c.R) * (2 * c.R) * 2 * chunk);
    uint8_t *ct = take(sizeof(float) * (size_t)S * S * 2 * chunk);
    uint8_t *r3 = take(sizeof(double) * 3 * L), *t3 = take(sizeof(double) * 3 * L), *ang = take(sizeof(double) * L), *M = take(sizeof(double) * 6 * L);
    if (a) {
        a->g = g; a->Mt = Mt;
        a->d_idx = (int32_t *)idx; a->d_tab = tab; a->d_win = (double *)win; a->d_f = (double *)f; a->d_pv = (double *)pv; a->d_pi = (int *)pi;
        a->d_small = (float *)small; a->d_cart_r = (float *)cr; a->d_cart_t = (float *)ct;
        a->d_rot3 = (double *)r3; a->d_trans3 = (double *)t3; a->d_ang = (double *)ang; a->d_M = (double *)M;
    }
    return off;
}

int32_t roam_fmt_auto_plan(roam_ctx *ctx, const FmtAutoCfg &c, FmtAutoPlan *plan)
{
    // what roam_engine_fmt_register refuses
    ARG_CHECK(ctx, c.lanes >= 1 && c.rows >= 8 && c.rows <= 16384 && c.cols >= 2 && c.cols <= 16384 && c.clip >= 1 && c.clip <= c.cols);
    ARG_CHECK(ctx, c.R >= ROAM_FMT_MIN_R && c.R <= ROAM_FMT_MAX_R && c.Rc >= 1 && 2 * c.Rc <= FFT_MAX_N);
    ARG_CHECK(ctx, c.min_rot >= 0.0 && c.min_rot <= 1e300 && c.min_trans >= 0.0 && c.min_trans <= 1e300);       // (NaN fails them too)
    const FmtRotSize g = fmt_rot_size(c.R);
    ARG_CHECK(ctx, g.M <= FFT_MAX_N && g.N <= FFT_MAX_N);
    const int S = 2 * c.Rc, Mt = optimal_dft_size(S);
    // as roam_fmt_register_run counts a pair on resident records
    const size_t per_reg = 7 * sizeof(double) * (size_t)Mt * Mt + sizeof(float) * 2 * (size_t)S * S + 6 * sizeof(double) + 2 * sizeof(int32_t);
    plan->per_pair = fmt_rot_bytes_per_pair(c.rows, c.R) + per_reg;
    plan->chunk = pc_chunk(plan->per_pair, (size_t)c.lanes, 32767, true);
    plan->slab_bytes = fmt_auto_carve(nullptr, c, plan->chunk, nullptr);
    plan->sz = g.sz;
    plan->log_base = fmt_log_base(g);
    return ROAM_OK;
}

double roam_fmt_scale(double log_base, double shift_x) { return fmt_scale(log_base, shift_x); }

void roam_fmt_auto_free(FmtAuto *a)
{
    if (!a) return;
    if (a->h_idx) (void)hipHostFree(a->h_idx);
    delete a;
}

int32_t roam_fmt_auto_init(roam_ctx *ctx, const FmtAutoCfg &c, const FmtAutoPlan &plan, uint8_t *slab, FmtAuto **out)
{
    FmtAuto *a = new (std::nothrow) FmtAuto();
    if (!a) { ROAM_SET_ERR(ctx, "auto prior: out of host memory"); return ROAM_E_HIP; }
    a->cfg = c; a->plan = plan;
    fmt_auto_carve(a, c, plan.chunk, slab);
    const int S = 2 * c.Rc;
    std::vector<unsigned char> tab(a->g.tab_bytes);
    std::vector<double> win(2 * (size_t)S);
    fmt_rot_tables(a->g, c.R, tab.data());
    roam_hanning_factors(S, win.data());
    roam_hanning_factors(S, win.data() + S);
    hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&a->h_idx), sizeof(int32_t) * 4 * 3 * (size_t)c.lanes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemcpyAsync(a->d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a->d_win, win.data(), sizeof(double) * win.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ROAM_SET_ERR(ctx, "auto prior: staging or table upload failed: %s", hipGetErrorString(e));
        roam_fmt_auto_free(a);
        return ROAM_E_HIP;
    }
    for (int n : {a->g.M, a->g.N, a->Mt})                  // now, not at the first step
        if (!fft_twiddles(ctx, n)) { roam_fmt_auto_free(a); return ROAM_E_HIP; }
    *out = a;
    return ROAM_OK;
}

int32_t roam_fmt_auto_enqueue(roam_ctx *ctx, FmtAuto *a, hipStream_t st, const FmtBatchIn &pool, int slot4, int npairs, const int32_t *prev,
                              const int32_t *curr, const int32_t *pair_of, uint8_t *prior_slot, FmtPriorRec *rec_slot)
{
    const FmtAutoCfg &c = a->cfg;
    const size_t L = (size_t)c.lanes, chunk = a->plan.chunk;
    int32_t *h = a->h_idx + (size_t)slot4 * 3 * L, *d = a->d_idx + (size_t)slot4 * 3 * L;
    for (size_t p0 = 0; p0 < (size_t)npairs; p0 += chunk) {          // chunk by chunk: the sources' records, then the targets'
        const size_t nb = std::min(chunk, (size_t)npairs - p0);
        memcpy(h + 2 * p0, prev + p0, sizeof(int32_t) * nb);
        memcpy(h + 2 * p0 + nb, curr + p0, sizeof(int32_t) * nb);
    }
    memcpy(h + 2 * L, pair_of, sizeof(int32_t) * L);
    HIP_TRY(ctx, hipMemcpyAsync(d, h, sizeof(int32_t) * 3 * L, hipMemcpyHostToDevice, st));
    const double cc = (double)(float)c.Rc;                   // getRotationMatrix2D's centre (w / 2, h / 2) as a cv::Point2f
    for (size_t p0 = 0; p0 < (size_t)npairs; p0 += chunk) {
        const int nb = (int)std::min(chunk, (size_t)npairs - p0);
        const FmtBatchSrc src = {pool.pool, pool.rec_bytes, pool.rec_stride, pool.payload_off, 1, d + 2 * p0};
        FFT_TRY(fmt_rot_enqueue(ctx, st, src, nb, c.rows, c.clip, c.R, a->g, a->d_tab, a->d_small, a->d_cart_r, a->d_f, nullptr, a->d_pv, a->d_pi,
                                a->d_rot3 + 3 * p0));
        HIP_TRY(ctx, launch_fmtr_angle_matrix(st, a->d_rot3 + 3 * p0, nb, a->plan.sz, cc, a->d_ang + p0, a->d_M + 6 * p0));
        FFT_TRY(fmt_trans_enqueue(ctx, st, src, nb, c.rows, c.cols, c.Rc, a->Mt, a->d_cart_t, a->d_M + 6 * p0, a->d_win, a->d_f, nullptr, a->d_pv,
                                  a->d_pi, a->d_trans3 + 3 * p0));
    }
    // the tracker's grid against the registration's: FMT.flowPriorFromFMT's s = (cols // 2) / (cols // cart_downsample)
    FmtPriorArgs pa = {d + 2 * L, a->d_rot3, a->d_ang, a->d_trans3, c.lanes, cc, (double)(c.cols / 2) / (double)c.Rc, c.min_rot, c.min_trans,
                       prior_slot, rec_slot};
    HIP_TRY(ctx, launch_fmtr_prior(st, pa));
    return ROAM_OK;
}

// ------------------------------------------------------------------------------------------------ test / measurement entries
// The direct 2-D DFT (float64 accumulation, twiddles from sincospi on (k mod n) / n), O(M N (M + N)): the baseline roam_time_fft2 times
// the FFT against (ROAM_TIME_DFT_FIVE).  No product path calls these three.
// along x: out[y][v] = sum_x in[y][x] exp(sign 2 pi i v x / N); in real (im_in == null) or complex
static __global__ void fmt_dft_x_kernel(const double *__restrict__ re_in, const double *__restrict__ im_in, int M, int N, double sign,
                                        double *__restrict__ re_out, double *__restrict__ im_out)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (v >= N) return;
    double ar = 0, ai = 0;
    for (int x = 0; x < N; x++) {
        double s, c;
        sincospi(sign * 2.0 * (double)((v * x) % N) / (double)N, &s, &c);
        const double xr = re_in[(int64_t)y * N + x], xi = im_in ? im_in[(int64_t)y * N + x] : 0.0;
        ar += xr * c - xi * s; ai += xr * s + xi * c;
    }
    re_out[(int64_t)y * N + v] = ar; im_out[(int64_t)y * N + v] = ai;
}

// along y: out[u][v] = sum_y in[y][v] exp(sign 2 pi i u y / M); im_out may be null
static __global__ void fmt_dft_y_kernel(const double *__restrict__ re_in, const double *__restrict__ im_in, int M, int N, double sign,
                                        double *__restrict__ re_out, double *__restrict__ im_out)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x, u = blockIdx.y;
    if (v >= N) return;
    double ar = 0, ai = 0;
    for (int y = 0; y < M; y++) {
        double s, c;
        sincospi(sign * 2.0 * (double)((u * y) % M) / (double)M, &s, &c);
        const double xr = re_in[(int64_t)y * N + v], xi = im_in[(int64_t)y * N + v];
        ar += xr * c - xi * s; ai += xr * s + xi * c;
    }
    re_out[(int64_t)u * N + v] = ar;
    if (im_out) im_out[(int64_t)u * N + v] = ai;
}

// fmt_dft_x_kernel into tmp, then fmt_dft_y_kernel
static hipError_t launch_fmt_dft2(hipStream_t st, const double *re_in, const double *im_in, int M, int N, double sign, double *tmp_re,
                                  double *tmp_im, double *re_out, double *im_out)
{
    const dim3 gmn((N + 63) / 64, M);
    hipLaunchKernelGGL(fmt_dft_x_kernel, gmn, dim3(64), 0, st, re_in, im_in, M, N, sign, tmp_re, tmp_im);
    hipLaunchKernelGGL(fmt_dft_y_kernel, gmn, dim3(64), 0, st, tmp_re, tmp_im, M, N, sign, re_out, im_out);
    return hipGetLastError();
}

extern "C" int32_t roam_debug_fft2_f64(roam_ctx *ctx, const double *re_in, const double *im_in, int32_t rows, int32_t cols, int32_t inverse,
                                       double *re_out, double *im_out)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, re_in && re_out && im_out && rows >= 1 && rows <= FFT_MAX_N && cols >= 1 && cols <= FFT_MAX_N);
    ARG_CHECK(ctx, fft_smooth(rows) && fft_smooth(cols));
    const int M = rows, N = cols;
    const size_t nmn = (size_t)M * N;
    double *d = (double *)roam_scratch(ctx, S_TMP2, sizeof(double) * nmn * 4);
    if (!d) return ROAM_E_HIP;
    double *ar = d, *ai = d + nmn, *br = d + 2 * nmn, *bi = d + 3 * nmn;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(ar, re_in, sizeof(double) * nmn, hipMemcpyHostToDevice, st));
    if (im_in) HIP_TRY(ctx, hipMemcpyAsync(ai, im_in, sizeof(double) * nmn, hipMemcpyHostToDevice, st));
    else HIP_TRY(ctx, hipMemsetAsync(ai, 0, sizeof(double) * nmn, st));
    FFT_TRY(fft_rows(ctx, st, ar, ai, ar, ai, M, N, inverse != 0));
    FFT_TRY(fft_transpose(ctx, st, ar, ai, 1, M, N, br, bi));
    FFT_TRY(fft_rows(ctx, st, br, bi, br, bi, N, M, inverse != 0));
    FFT_TRY(fft_transpose(ctx, st, br, bi, 1, N, M, ar, ai));
    HIP_TRY(ctx, hipMemcpyAsync(re_out, ar, sizeof(double) * nmn, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(im_out, ai, sizeof(double) * nmn, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return ROAM_OK;
}

extern "C" int32_t roam_time_fft2(roam_ctx *ctx, int32_t rows, int32_t cols, int32_t what, int32_t reps, float *ms_per_rep)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, ms_per_rep && reps >= 1 && what >= 0 && what <= 4 && rows >= 2 && rows <= FFT_MAX_N && cols >= 2 && cols <= FFT_MAX_N);
    ARG_CHECK(ctx, fft_smooth(rows) && fft_smooth(cols));
    ARG_CHECK(ctx, what != ROAM_TIME_DFT_FIVE || (int64_t)rows * cols <= (1 << 17));       // the direct form is O(M N (M + N))
    const int M = rows, N = cols;
    const size_t nmn = (size_t)M * N;
    double *d = (double *)roam_scratch(ctx, S_TMP2, sizeof(double) * nmn * 7);
    if (!d) return ROAM_E_HIP;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(d, 0, sizeof(double) * nmn * 7, st));
    const PcPlanes p = pc_planes(d, nmn);
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); ROAM_SET_ERR(ctx, "hipEventCreate failed"); return ROAM_E_HIP; }
    int32_t rc = ROAM_OK;
    for (int rep = -2; rep < reps && rc == ROAM_OK; rep++) {                 // two warm runs (they also upload the twiddle tables)
        if (rep == 0) (void)hipEventRecord(e0, st);
        if (what == ROAM_TIME_FFT_FIVE) {
            for (int k = 0; k < 2 && rc == ROAM_OK; k++) {
                rc = fft_rows(ctx, st, p.a, nullptr, p.tr, p.ti, M, N, false);
                if (rc == ROAM_OK) rc = fft_transpose(ctx, st, p.tr, p.ti, 1, M, N, p.F[k][0], p.F[k][1]);
                if (rc == ROAM_OK) rc = fft_rows(ctx, st, p.F[k][0], p.F[k][1], p.F[k][0], p.F[k][1], N, M, false);
            }
            if (rc == ROAM_OK) rc = fft_rows(ctx, st, p.tr, p.ti, p.tr, p.ti, N, M, true);
            if (rc == ROAM_OK) rc = fft_transpose(ctx, st, p.tr, p.ti, 1, N, M, p.F[0][0], p.F[0][1]);
            if (rc == ROAM_OK) rc = fft_rows(ctx, st, p.F[0][0], p.F[0][1], p.a, nullptr, M, N, true);
        } else if (what == ROAM_TIME_DFT_FIVE) {
            for (int k = 0; k < 2; k++) (void)launch_fmt_dft2(st, p.a, nullptr, M, N, -1.0, p.tr, p.ti, p.F[k][0], p.F[k][1]);
            (void)launch_fmt_dft2(st, p.tr, p.ti, M, N, 1.0, p.F[0][0], p.F[0][1], p.a, nullptr);
        } else if (what == ROAM_TIME_FFT_ROWS) {
            rc = fft_rows(ctx, st, p.tr, p.ti, p.tr, p.ti, M, N, false);
        } else if (what == ROAM_TIME_FFT_TRANSPOSE) {
            rc = fft_transpose(ctx, st, p.tr, p.ti, 1, M, N, p.F[0][0], p.F[0][1]);
        } else {
            rc = fft_rows(ctx, st, p.tr, p.ti, p.tr, p.ti, N, M, false);
        }
    }
    (void)hipEventRecord(e1, st);
    hipError_t e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc != ROAM_OK) return rc;
    HIP_TRY(ctx, e);
    HIP_TRY(ctx, hipGetLastError());
    *ms_per_rep = ms / (float)reps;
    return ROAM_OK;
}
