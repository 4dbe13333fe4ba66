// Mixed-radix FFT (complex float64, n = 2^a 3^b 5^c <= 4096): what phase correlation (phasecorr.hip) and, through it, the Fourier-Mellin
// passes (fmt.hip) transform with.  fft.h declares what those units call.  docs/KERNELS.md "FFT" has the structure.
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
// Behind the transform: the direct DFT it is timed against and the two test / timing entries.
#include "fft.h"
#include <math.h>

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

const double *fft_twiddles(roam_ctx *ctx, int n)
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

int32_t fft_rows(roam_ctx *ctx, hipStream_t st, const double *re_in, const double *im_in, double *re_out, double *im_out, int64_t total_rows, int n,
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

int32_t fft_transpose(roam_ctx *ctx, hipStream_t st, const double *re_in, const double *im_in, int batch, int M, int N, double *re_out, double *im_out)
{
    hipLaunchKernelGGL(fft_transpose_kernel, dim3((N + 31) / 32, (M + 31) / 32, batch), dim3(32, 8), 0, st, re_in, im_in, M, N, re_out,
                       im_out);
    HIP_TRY(ctx, hipGetLastError());
    return ROAM_OK;
}

bool fft_smooth(int n)
{
    FftPlan p;
    return fft_plan(n, &p);
}

// cv2.getOptimalDFTSize: the smallest 2^a 3^b 5^c >= n
int optimal_dft_size(int n)
{
    int best = 0;
    for (long p2 = 1; p2 < 2L * n; p2 *= 2)
        for (long p3 = p2; p3 < 2L * n; p3 *= 3)
            for (long p5 = p3; p5 < 2L * n; p5 *= 5)
                if (p5 >= n && (best == 0 || p5 < best)) best = (int)p5;
    return best;
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
    const size_t planes_bytes = pc_work_bytes(nmn, 1).f;        // the planes of one correlation, no peak search
    double *d = (double *)roam_scratch(ctx, S_TMP2, planes_bytes);
    if (!d) return ROAM_E_HIP;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(d, 0, planes_bytes, st));
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
