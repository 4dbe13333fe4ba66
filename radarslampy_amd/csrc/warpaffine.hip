// cv2.warpAffine(src, M, (dw, dh), INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT 0) on float32 images (reference FMT.py:93-100,
// rotateImg: getRotationMatrix2D + warpAffine; used by Tracker.py:67-69, plotCartPolarWithRotation and the script's perfect-image
// test, FMT.py:190-208).  OpenCV 4's CV_32F arithmetic (imgwarp.cpp, restated; parity with a cv2 build is unpinned, docs/PARITY.md):
//   host, float64: without WARP_INVERSE_MAP the 2 x 3 matrix is inverted in OpenCV's operation order (a singular one becomes all
//     zeros: every output pixel then reads src[0, 0]).
//   device, per output pixel (x, y), AB_SCALE = 1024, cvRound = nearest-even saturated to int32:
//     adelta = cvRound(M0 x 1024), bdelta = cvRound(M3 x 1024), X0 = cvRound((M1 y + M2) 1024) + 16, Y0 = cvRound((M4 y + M5) 1024) + 16,
//     X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5 in (wrapping) int32: 1/32-px coordinates; tap index saturate<int16>(X >> 5),
//     fraction X & 31.
//   remap: cvmap.h's - weights wy * wx from (frac / 32, 1 - frac / 32), taps outside the source read 0, sum in OpenCV's order.
// The fixed-point block and the remap are cv_affine_fixed32 and cv_remap of cvmap.h, shared with fmt_register.hip.
// One thread per output pixel in a 32 x 8 tile of the destination, blockIdx.z = image.  A 256-wide row strip of the destination walks
// a slanted line through the source (at 45 degrees 181 source rows, one 128-byte line or two from each); the 32 x 8 tile's footprint is a
// 32 x 8 rectangle of the source turned by the angle - inside a 34 x 34 box at any angle - so a line fetched for one wave serves the
// other three from the CU's L1 and neighbouring tiles from the L2.  Stores: a wave writes two full 128-byte row segments.
#include "cvmap.h"
#include <cmath>

#define WA_MAX_SIDE 16384
#define WA_TILE_X 32
#define WA_TILE_Y 8

// M: the INVERSE maps (destination -> source), 6 doubles per matrix; m_stride = 0 (one for all images) or 6
__global__ __launch_bounds__(WA_TILE_X * WA_TILE_Y) void warp_affine_kernel(const float *__restrict__ src, int rows, int cols,
                                                                             int64_t row_stride, int64_t image_stride,
                                                                             const double *__restrict__ M, int m_stride,
                                                                             float *__restrict__ dst, int dw, int dh)
{
    const int x = blockIdx.x * WA_TILE_X + threadIdx.x, y = blockIdx.y * WA_TILE_Y + threadIdx.y;
    if (x >= dw || y >= dh) return;
    const int64_t img = blockIdx.z;
    int X, Y;
    cv_affine_fixed32(M + img * m_stride, x, y, X, Y);
    const CvCartTap tap = {src + img * image_stride, rows, cols, row_stride};
    dst[(img * dh + y) * dw + x] = cv_remap(tap, X, Y);
}

// rotateImg's matrix (FMT.py:93-100) as warpAffine applies it: cv2.getRotationMatrix2D((cx, cy), angle_deg, 1.0) in float64 - the centre is
// a cv::Point2f, the caller passes float32 values - inverted by cvmap.h's cv_invert_affine -> Minv[6], destination -> source
void roam_rotation_inverse_map(double cx, double cy, double angle_deg, double *Minv)
{
    const double rad = angle_deg * M_PI / 180.0;
    double M[6];
    cv_rotation_matrix(cos(rad), sin(rad), cx, cy, M);
    cv_invert_affine(M, Minv);
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
        else cv_invert_affine(M + (size_t)i * 6, &inv[(size_t)i * 6]);
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
    HIP_TRY(ctx, roam_upload_packed_f32(st, d_in, src, n, cols, rows, src_row_stride, src_image_stride));
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
    const int32_t rt = roam_time_launches(ctx, st, reps, ms_per_rep, [&] {
        wa_launch(st, d_in, n, rows, cols, d_M, 1, d_out, cols, rows);
        return hipGetLastError();
    });
    if (rt != ROAM_OK) (void)hipStreamSynchronize(st);      // `inv` lives until its upload is done (a timed run has waited already)
    return rt;
}
