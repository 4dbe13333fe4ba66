// cv2.warpAffine(src, M, (dw, dh), INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT 0) on float32 images (reference FMT.py:93-100,
// rotateImg: getRotationMatrix2D + warpAffine; used by Tracker.py:67-69, plotCartPolarWithRotation and the script's perfect-image
// test, FMT.py:190-208).  OpenCV 4's CV_32F arithmetic (imgwarp.cpp, restated; parity with a cv2 build is unpinned, docs/PARITY.md):
//   host, float64: without WARP_INVERSE_MAP the 2 x 3 matrix is inverted in OpenCV's operation order (a singular one becomes all
//     zeros: every output pixel then reads src[0, 0]).
//   device, per output pixel (x, y), AB_SCALE = 1024, cvRound = nearest-even saturated to int32:
//     adelta = cvRound(M0 x 1024), bdelta = cvRound(M3 x 1024), X0 = cvRound((M1 y + M2) 1024) + 16, Y0 = cvRound((M4 y + M5) 1024) + 16,
//     X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5 in (wrapping) int32: 1/32-px coordinates; tap index saturate<int16>(X >> 5),
//     fraction X & 31.
//   remap: warppolar.hip's - weights wy * wx from (frac / 32, 1 - frac / 32), taps outside the source read 0, sum in OpenCV's order.
// One thread per output pixel in a 32 x 8 tile of the destination, blockIdx.z = image.  A 256-wide row strip of the destination walks
// a slanted line through the source (at 45 degrees 181 source rows, one 128-byte line or two from each); the 32 x 8 tile's footprint is a
// 32 x 8 rectangle of the source turned by the angle - inside a 34 x 34 box at any angle - so a line fetched for one wave serves the
// other three from the CU's L1 and neighbouring tiles from the L2.  Stores: a wave writes two full 128-byte row segments.
#include "roam_internal.h"
#include <cmath>

#define WA_MAX_SIDE 16384
#define WA_TILE_X 32
#define WA_TILE_Y 8

// saturate_cast<int>(double): nearest-even, saturated (the clamp is explicit: a float-to-int conversion out of range is undefined)
__device__ __forceinline__ unsigned wa_round(double v) { return (unsigned)(int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); }

// saturate_cast<short>(s >> INTER_BITS)
__device__ __forceinline__ int wa_tap_index(int s) { return min(max(s >> 5, -32768), 32767); }

__device__ __forceinline__ float wa_tap(const float *__restrict__ p, int rows, int cols, int64_t stride, int y, int x)
{
    return (x < 0 || x >= cols || y < 0 || y >= rows) ? 0.f : p[(int64_t)y * stride + x];
}

// M: the INVERSE maps (destination -> source), 6 doubles per matrix; m_stride = 0 (one for all images) or 6
__global__ __launch_bounds__(WA_TILE_X * WA_TILE_Y) void warp_affine_kernel(const float *__restrict__ src, int rows, int cols,
                                                                             int64_t row_stride, int64_t image_stride,
                                                                             const double *__restrict__ M, int m_stride,
                                                                             float *__restrict__ dst, int dw, int dh)
{
    const int x = blockIdx.x * WA_TILE_X + threadIdx.x, y = blockIdx.y * WA_TILE_Y + threadIdx.y;
    if (x >= dw || y >= dh) return;
    const int64_t img = blockIdx.z;
    const double *m = M + img * m_stride;
    const double dx = (double)x, dy = (double)y;
    // the int32 sums wrap (unsigned arithmetic)
    const unsigned adelta = wa_round(__dmul_rn(__dmul_rn(m[0], dx), 1024.0));
    const unsigned bdelta = wa_round(__dmul_rn(__dmul_rn(m[3], dx), 1024.0));
    const unsigned X0 = wa_round(__dmul_rn(__dadd_rn(__dmul_rn(m[1], dy), m[2]), 1024.0)) + 16u;
    const unsigned Y0 = wa_round(__dmul_rn(__dadd_rn(__dmul_rn(m[4], dy), m[5]), 1024.0)) + 16u;
    const int X = (int)(X0 + adelta) >> 5, Y = (int)(Y0 + bdelta) >> 5;
    const int ix = wa_tap_index(X), iy = wa_tap_index(Y);
    const float wx1 = __fmul_rn((float)(X & 31), 1.f / 32.f), wx0 = __fsub_rn(1.f, wx1);
    const float wy1 = __fmul_rn((float)(Y & 31), 1.f / 32.f), wy0 = __fsub_rn(1.f, wy1);
    const float *p = src + img * image_stride;
    float v = __fmul_rn(wa_tap(p, rows, cols, row_stride, iy, ix), __fmul_rn(wy0, wx0));
    v = __fadd_rn(v, __fmul_rn(wa_tap(p, rows, cols, row_stride, iy, ix + 1), __fmul_rn(wy0, wx1)));
    v = __fadd_rn(v, __fmul_rn(wa_tap(p, rows, cols, row_stride, iy + 1, ix), __fmul_rn(wy1, wx0)));
    v = __fadd_rn(v, __fmul_rn(wa_tap(p, rows, cols, row_stride, iy + 1, ix + 1), __fmul_rn(wy1, wx1)));
    dst[(img * dh + y) * dw + x] = v;
}

// OpenCV's invertAffineTransform as warpAffine applies it in place (no fused multiply-add: roam_internal.h)
static void wa_invert(const double *in, double *M)
{
    for (int k = 0; k < 6; k++) M[k] = in[k];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D;
    M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
}

// rotateImg's matrix (FMT.py:93-100) as warpAffine applies it: cv2.getRotationMatrix2D((cx, cy), angle_deg, 1.0) in float64 - the centre is
// a cv::Point2f, the caller passes float32 values - inverted by wa_invert -> Minv[6], destination -> source
void roam_rotation_inverse_map(double cx, double cy, double angle_deg, double *Minv)
{
    const double rad = angle_deg * M_PI / 180.0;
    const double a = cos(rad), b = sin(rad);
    const double M[6] = {a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy};
    wa_invert(M, Minv);
}

static void wa_launch(hipStream_t st, const float *d_in, int n, int rows, int cols, const double *d_M, int m_count, float *d_out, int dw,
                      int dh)
{
    const size_t nin = (size_t)rows * cols, nout = (size_t)dh * dw;
    for (int i0 = 0; i0 < n; i0 += 65535) {                 // (the grid's z extent)
        const int nb = n - i0 < 65535 ? n - i0 : 65535;
        const dim3 grid((dw + WA_TILE_X - 1) / WA_TILE_X, (dh + WA_TILE_Y - 1) / WA_TILE_Y, nb);
        hipLaunchKernelGGL(warp_affine_kernel, grid, dim3(WA_TILE_X, WA_TILE_Y), 0, st, d_in + (size_t)i0 * nin, rows, cols, (int64_t)cols,
                           (int64_t)nin, d_M + (m_count == 1 ? 0 : (size_t)i0 * 6), m_count == 1 ? 0 : 6, d_out + (size_t)i0 * nout, dw, dh);
    }
}

static int32_t wa_upload_matrices(roam_ctx *ctx, const double *M, int m_count, int flags, std::vector<double> &inv, const double **d_M)
{
    inv.resize((size_t)m_count * 6);
    for (int i = 0; i < m_count; i++) {
        if (flags & ROAM_WARP_AFFINE_INVERSE_MAP) memcpy(&inv[(size_t)i * 6], M + (size_t)i * 6, sizeof(double) * 6);
        else wa_invert(M + (size_t)i * 6, &inv[(size_t)i * 6]);
    }
    double *d = (double *)roam_scratch(ctx, S_TMP0, sizeof(double) * inv.size());
    if (!d) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(d, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice, ctx->stream));
    *d_M = d;
    return ROAM_OK;
}

extern "C" int32_t roam_warp_affine_f32(roam_ctx *ctx, const float *src, int32_t n, int32_t rows, int32_t cols, int64_t src_row_stride,
                                        int64_t src_image_stride, const double *M, int32_t m_count, float *dst, int32_t dw, int32_t dh,
                                        int32_t flags)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, src && M && dst && (flags & ~ROAM_WARP_AFFINE_INVERSE_MAP) == 0);
    ARG_CHECK(ctx, n >= 1 && rows >= 1 && cols >= 1 && dw >= 1 && dh >= 1);
    ARG_CHECK(ctx, rows <= WA_MAX_SIDE && cols <= WA_MAX_SIDE && dw <= WA_MAX_SIDE && dh <= WA_MAX_SIDE);
    ARG_CHECK(ctx, m_count == 1 || m_count == n);
    ARG_CHECK(ctx, src_row_stride >= cols && (n == 1 || src_image_stride >= (int64_t)(rows - 1) * src_row_stride + cols));
    hipStream_t st = ctx->stream;
    const size_t nin = (size_t)rows * cols, nout = (size_t)dh * dw;
    float *d_in = (float *)roam_scratch(ctx, S_IN0, sizeof(float) * nin * n);
    float *d_out = (float *)roam_scratch(ctx, S_OUT0, sizeof(float) * nout * n);
    if (!d_in || !d_out) return ROAM_E_HIP;
    // pack the images tightly on the way up, as roam_warp_polar_f32 does
    if (n == 1 || src_image_stride == (int64_t)rows * src_row_stride)
        HIP_TRY(ctx, hipMemcpy2DAsync(d_in, sizeof(float) * cols, src, sizeof(float) * src_row_stride, sizeof(float) * cols,
                                      (size_t)rows * n, hipMemcpyHostToDevice, st));
    else
        for (int i = 0; i < n; i++)
            HIP_TRY(ctx, hipMemcpy2DAsync(d_in + i * nin, sizeof(float) * cols, src + i * src_image_stride, sizeof(float) * src_row_stride,
                                          sizeof(float) * cols, rows, hipMemcpyHostToDevice, st));
    std::vector<double> inv;
    const double *d_M = nullptr;
    const int32_t rc = wa_upload_matrices(ctx, M, m_count, flags, inv, &d_M);
    if (rc != ROAM_OK) return rc;
    wa_launch(st, d_in, n, rows, cols, d_M, m_count, d_out, dw, dh);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_out, sizeof(float) * nout * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                 // (also keeps `inv` alive until its upload is done)
    return ROAM_OK;
}

extern "C" int32_t roam_time_warp_affine(roam_ctx *ctx, int32_t n, int32_t rows, int32_t cols, const double *M, int32_t reps,
                                         float *ms_per_rep)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, M && ms_per_rep && reps >= 1 && n >= 1 && n <= 65535 && rows >= 1 && cols >= 1 && rows <= WA_MAX_SIDE && cols <= WA_MAX_SIDE);
    hipStream_t st = ctx->stream;
    const size_t npx = (size_t)rows * cols * n;
    float *d_in = (float *)roam_scratch(ctx, S_IN0, sizeof(float) * npx);
    float *d_out = (float *)roam_scratch(ctx, S_OUT0, sizeof(float) * npx);
    if (!d_in || !d_out) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemsetAsync(d_in, 0, sizeof(float) * npx, st));
    std::vector<double> inv;
    const double *d_M = nullptr;
    const int32_t rc = wa_upload_matrices(ctx, M, 1, 0, inv, &d_M);
    if (rc != ROAM_OK) return rc;
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); ROAM_SET_ERR(ctx, "hipEventCreate failed"); return ROAM_E_HIP; }
    for (int rep = -2; rep < reps; rep++) {                 // two warm runs
        if (rep == 0) (void)hipEventRecord(e0, st);
        wa_launch(st, d_in, n, rows, cols, d_M, 1, d_out, cols, rows);
    }
    (void)hipEventRecord(e1, st);
    hipError_t e = hipEventSynchronize(e1);                 // (also keeps `inv` alive until its upload is done)
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e == hipSuccess) e = hipGetLastError();
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIP_TRY(ctx, e);
    *ms_per_rep = ms / reps;
    return ROAM_OK;
}
