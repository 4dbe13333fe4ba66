// cv2.warpPolar(src, dsize, center, maxRadius, INTER_LINEAR | WARP_FILL_OUTLIERS [| WARP_POLAR_LOG] [| WARP_INVERSE_MAP]) on float32
// images with free geometry, all four modes (reference parseData.py:69-157: convertCartesianImageToPolar,
// convertPolarImageToCartesian with any downsampleFactor / logPolarMode, convertPolarImgToLogPolar; FMT.py:191-226).
//   inverse (polar -> Cartesian): the polar source gets one wrapped row above and one below (copyMakeBorder BORDER_WRAP);
//     per pixel cartToPolar of (x - cx, y - cy) = sqrt + the degree-7 fastAtan polynomial, [log(mag + 1)], then
//     mx = p / Kmag, my = ang / Kangle + 1 with Kmag = maxRadius / cols (or log(maxRadius) / cols), Kangle = 2 pi / rows.
//   forward (Cartesian -> polar): dh rows of angle, dw columns of radius; the radius table br (dw floats) and cos / sin per row
//     (2 dh doubles) come from the HOST's libm, as OpenCV computes them, so that they equal what the oracle's C computes.
//   The maps and the remap are cvmap.h's, the definitions every unit that samples as OpenCV does calls; the host tables and the packed
//   upload defined here (roam_warp_polar_tables, roam_upload_packed_f32) serve phasecorr.hip, fmt.hip and warpaffine.hip too.
//   remap: coordinates rounded to 1/32 px (cvRound, half to even), tap index saturated to int16, bilinear weights
//     wy * wx from the 32-entry tables, taps outside the (padded) source read 0, sum in OpenCV's order.
// The inverse semilog mode takes (float)log((double)(mag + 1)) where OpenCV uses hal::log32f: parity with OpenCV is unpinned there
// (docs/PARITY.md).  One thread per output pixel, 256 along a destination row, blockIdx.y = row, blockIdx.z = image: coalesced
// stores, gathers through the L2.
#include "cvmap.h"
#include <cmath>

#define WP_MAX_SIDE 16384

// polar (rows x cols per image, image_stride floats apart) -> dh x dw Cartesian per image
template <bool LOG>
__global__ __launch_bounds__(256) void warp_polar_inverse_kernel(const float *__restrict__ src, int rows, int cols, int64_t row_stride,
                                                                 int64_t image_stride, float *__restrict__ dst, int dw, int dh, float cx,
                                                                 float cy, double Kmag, double Kangle)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const int64_t img = blockIdx.z;
    float mx, my;
    cv_polar_inverse_map<LOG>(x, y, cx, cy, Kmag, Kangle, mx, my);
    const CvPolarTap<false> tap = {src + img * image_stride, rows, cols, row_stride, 0};
    dst[(img * dh + y) * dw + x] = cv_remap(tap, mx, my);
}

// Cartesian (rows x cols per image) -> dh x dw polar per image; br[rho] the radius, cs[2 phi], cs[2 phi + 1] = cos, sin of the angle
__global__ __launch_bounds__(256) void warp_polar_forward_kernel(const float *__restrict__ src, int rows, int cols, int64_t row_stride,
                                                                 int64_t image_stride, float *__restrict__ dst, int dw, int dh, float cx,
                                                                 float cy, const float *__restrict__ br, const double *__restrict__ cs)
{
    const int rho = blockIdx.x * blockDim.x + threadIdx.x, phi = blockIdx.y;
    if (rho >= dw) return;
    const int64_t img = blockIdx.z;
    float mx, my;
    cv_polar_forward_map((double)br[rho], cs[2 * phi], cs[2 * phi + 1], (double)cx, (double)cy, mx, my);
    const CvCartTap tap = {src + img * image_stride, rows, cols, row_stride};
    dst[(img * dh + phi) * dw + rho] = cv_remap(tap, mx, my);
}

// OpenCV's host tables of the forward warpPolar (imgwarp.cpp): Kmag and Kangle from the DESTINATION size, the host's libm.
// br: the radius per destination column (dw floats); cs: cos, sin of the angle per destination row (2 dh doubles)
void roam_warp_polar_tables(int dw, int dh, double max_radius, bool semilog, float *br, double *cs)
{
    const double Kangle = 6.283185307179586476925286766559 / dh;
    if (semilog) {
        const double Kmag = std::log(max_radius) / dw;
        for (int rho = 0; rho < dw; rho++) br[rho] = (float)(std::exp(rho * Kmag) - 1.0);
    } else {
        const double Kmag = max_radius / dw;
        for (int rho = 0; rho < dw; rho++) br[rho] = (float)(rho * Kmag);
    }
    for (int phi = 0; phi < dh; phi++) {
        const double KKy = Kangle * phi;
        cs[2 * phi] = std::cos(KKy);
        cs[2 * phi + 1] = std::sin(KKy);
    }
}

// n host images (rows x width floats of rows row_stride apart, images image_stride apart; one image: image_stride is not read) -> a
// tight n x rows x width device array, asynchronous on st.  One copy when the images are contiguous, one per image when only the rows
// are (a 2-D copy moves the rows one by one), one 2-D copy when the images' rows follow each other at the row stride, else one per image
hipError_t roam_upload_packed_f32(hipStream_t st, float *dst, const float *src, int n, int width, int rows, int64_t row_stride,
                                  int64_t image_stride)
{
    const size_t nimg = (size_t)rows * width;
    const bool rows_follow = n == 1 || image_stride == (int64_t)rows * row_stride;
    if (row_stride == width && rows_follow) return hipMemcpyAsync(dst, src, sizeof(float) * nimg * n, hipMemcpyHostToDevice, st);
    if (rows_follow)
        return hipMemcpy2DAsync(dst, sizeof(float) * width, src, sizeof(float) * row_stride, sizeof(float) * width, (size_t)rows * n,
                                hipMemcpyHostToDevice, st);
    for (int i = 0; i < n; i++) {
        const float *h = src + (int64_t)i * image_stride;
        const hipError_t e = row_stride == width
                                 ? hipMemcpyAsync(dst + (size_t)i * nimg, h, sizeof(float) * nimg, hipMemcpyHostToDevice, st)
                                 : hipMemcpy2DAsync(dst + (size_t)i * nimg, sizeof(float) * width, h, sizeof(float) * row_stride,
                                                    sizeof(float) * width, rows, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

extern "C" int32_t roam_warp_polar_f32(roam_ctx *ctx, const float *src, int32_t n, int32_t rows, int32_t cols, int64_t src_row_stride,
                                       int64_t src_image_stride, float *dst, int32_t dw, int32_t dh, float cx, float cy,
                                       double max_radius, int32_t flags)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool semilog = (flags & ROAM_WARP_POLAR_LOG) != 0, inverse = (flags & ROAM_WARP_POLAR_INVERSE) != 0;
    ARG_CHECK(ctx, src && dst && (flags & ~(ROAM_WARP_POLAR_LOG | ROAM_WARP_POLAR_INVERSE)) == 0);
    ARG_CHECK(ctx, n > 0 && rows > 0 && cols > 0 && dw > 0 && dh > 0);
    ARG_CHECK(ctx, rows <= WP_MAX_SIDE && cols <= WP_MAX_SIDE && dw <= WP_MAX_SIDE && dh <= WP_MAX_SIDE);
    ARG_CHECK(ctx, src_row_stride >= cols && (n == 1 || src_image_stride >= (int64_t)(rows - 1) * src_row_stride + cols));
    ARG_CHECK(ctx, std::isfinite(max_radius) && max_radius > (semilog ? 1.0 : 0.0) && std::isfinite(cx) && std::isfinite(cy));
    hipStream_t st = ctx->stream;
    const size_t nin = (size_t)rows * cols, nout = (size_t)dh * dw;
    float *d_in = (float *)roam_scratch(ctx, S_IN0, sizeof(float) * nin * n);
    float *d_out = (float *)roam_scratch(ctx, S_OUT0, sizeof(float) * nout * n);
    if (!d_in || !d_out) return ROAM_E_HIP;
    // (a column slice of a wider record travels without its unused columns)
    HIP_TRY(ctx, roam_upload_packed_f32(st, d_in, src, n, cols, rows, src_row_stride, src_image_stride));
    std::vector<unsigned char> tab;
    const float *d_br = nullptr;
    const double *d_cs = nullptr;
    if (!inverse) {
        tab.resize(sizeof(double) * 2 * dh + sizeof(float) * dw);
        roam_warp_polar_tables(dw, dh, max_radius, semilog, (float *)((double *)tab.data() + 2 * dh), (double *)tab.data());
        unsigned char *d_tab = (unsigned char *)roam_scratch(ctx, S_TMP0, tab.size());
        if (!d_tab) return ROAM_E_HIP;
        HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
        d_cs = (const double *)d_tab;
        d_br = (const float *)(d_cs + 2 * dh);
    }
    const double Kangle_inv = 6.283185307179586476925286766559 / rows;
    const double Kmag_inv = semilog ? std::log(max_radius) / cols : max_radius / cols;
    for (int i0 = 0; i0 < n; i0 += 65535) {                 // (the grid's z extent)
        const int nb = n - i0 < 65535 ? n - i0 : 65535;
        const dim3 grid((dw + 255) / 256, dh, nb);
        const float *s = d_in + (size_t)i0 * nin;
        float *d = d_out + (size_t)i0 * nout;
        if (!inverse)
            hipLaunchKernelGGL(warp_polar_forward_kernel, grid, dim3(256), 0, st, s, rows, cols, (int64_t)cols, (int64_t)nin, d, dw, dh, cx, cy,
                               d_br, d_cs);
        else if (semilog)
            hipLaunchKernelGGL(warp_polar_inverse_kernel<true>, grid, dim3(256), 0, st, s, rows, cols, (int64_t)cols, (int64_t)nin, d, dw, dh,
                               cx, cy, Kmag_inv, Kangle_inv);
        else
            hipLaunchKernelGGL(warp_polar_inverse_kernel<false>, grid, dim3(256), 0, st, s, rows, cols, (int64_t)cols, (int64_t)nin, d, dw, dh,
                               cx, cy, Kmag_inv, Kangle_inv);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_out, sizeof(float) * nout * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));                 // (also keeps `tab` alive until its upload is done)
    return ROAM_OK;
}
