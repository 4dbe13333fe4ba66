// cv2.warpPolar(src, dsize, center, maxRadius, INTER_LINEAR | WARP_FILL_OUTLIERS [| WARP_POLAR_LOG] [| WARP_INVERSE_MAP]) on float32
// images with free geometry, all four modes (reference parseData.py:69-157: convertCartesianImageToPolar,
// convertPolarImageToCartesian with any downsampleFactor / logPolarMode, convertPolarImgToLogPolar; FMT.py:191-226).
//   inverse (polar -> Cartesian): the polar source gets one wrapped row above and one below (copyMakeBorder BORDER_WRAP);
//     per pixel cartToPolar of (x - cx, y - cy) = sqrt + the degree-7 fastAtan polynomial, [log(mag + 1)], then
//     mx = p / Kmag, my = ang / Kangle + 1 with Kmag = maxRadius / cols (or log(maxRadius) / cols), Kangle = 2 pi / rows.
//   forward (Cartesian -> polar): dh rows of angle, dw columns of radius; the radius table br (dw floats) and cos / sin per row
//     (2 dh doubles) come from the HOST's libm, as OpenCV computes them, so that they equal what the oracle's C computes.
//   remap: coordinates rounded to 1/32 px (cvRound, half to even), tap index saturated to int16, bilinear weights
//     wy * wx from the 32-entry tables, taps outside the (padded) source read 0, sum in OpenCV's order.
// The inverse semilog mode takes (float)log((double)(mag + 1)) where OpenCV uses hal::log32f: parity with OpenCV is unpinned there
// (docs/PARITY.md).  One thread per output pixel, 256 along a destination row, blockIdx.y = row, blockIdx.z = image: coalesced
// stores, gathers through the L2.
#include "roam_internal.h"
#include <cmath>

#define WP_PI 3.14159265358979323846
#define WP_MAX_SIDE 16384

__device__ __forceinline__ float wp_fast_atan2_deg(float y, float x)
{
    const float sc = (float)(180 / WP_PI);
    const float p1 = __fmul_rn(0.9997878412794807f, sc), p3 = __fmul_rn(-0.3258083974640975f, sc);
    const float p5 = __fmul_rn(0.1555786518463281f, sc), p7 = __fmul_rn(-0.04432655554792128f, sc);
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, __fadd_rn(ax, (float)2.220446049250313e-16)); c2 = __fmul_rn(c, c);
        a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    } else {
        c = __fdiv_rn(ax, __fadd_rn(ay, (float)2.220446049250313e-16)); c2 = __fmul_rn(c, c);
        a = __fsub_rn(90.f, __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c));
    }
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

// saturate_cast<short>(s >> INTER_BITS)
__device__ __forceinline__ int wp_tap_index(int s) { return min(max(s >> 5, -32768), 32767); }

// polar source with its wrapped border rows: py indexes the padded image (rows + 2), 0 -> row rows - 1, rows + 1 -> row 0
struct WpPolarTap {
    const float *p; int rows, cols; int64_t stride;
    __device__ float operator()(int py, int px) const
    {
        if (px < 0 || px >= cols || py < 0 || py >= rows + 2) return 0.f;
        int r = py - 1;
        if (r < 0) r += rows; else if (r >= rows) r -= rows;
        return p[(int64_t)r * stride + px];
    }
};

struct WpCartTap {
    const float *p; int rows, cols; int64_t stride;
    __device__ float operator()(int y, int x) const { return (x < 0 || x >= cols || y < 0 || y >= rows) ? 0.f : p[(int64_t)y * stride + x]; }
};

template <class Tap>
__device__ __forceinline__ float wp_remap(const Tap &tap, float mx, float my)
{
    const int sx = __float2int_rn(__fmul_rn(mx, 32.f)), sy = __float2int_rn(__fmul_rn(my, 32.f));
    const int ix = wp_tap_index(sx), iy = wp_tap_index(sy);
    const float wx1 = __fmul_rn((float)(sx & 31), 1.f / 32.f), wx0 = __fsub_rn(1.f, wx1);
    const float wy1 = __fmul_rn((float)(sy & 31), 1.f / 32.f), wy0 = __fsub_rn(1.f, wy1);
    float v = __fmul_rn(tap(iy, ix), __fmul_rn(wy0, wx0));
    v = __fadd_rn(v, __fmul_rn(tap(iy, ix + 1), __fmul_rn(wy0, wx1)));
    v = __fadd_rn(v, __fmul_rn(tap(iy + 1, ix), __fmul_rn(wy1, wx0)));
    v = __fadd_rn(v, __fmul_rn(tap(iy + 1, ix + 1), __fmul_rn(wy1, wx1)));
    return v;
}

// polar (rows x cols per image, image_stride floats apart) -> dh x dw Cartesian per image
template <bool LOG>
__global__ __launch_bounds__(256) void warp_polar_inverse_kernel(const float *__restrict__ src, int rows, int cols, int64_t row_stride,
                                                                 int64_t image_stride, float *__restrict__ dst, int dw, int dh, float cx,
                                                                 float cy, double Kmag, double Kangle)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const int64_t img = blockIdx.z;
    const float fx = __fsub_rn((float)x, cx), fy = __fsub_rn((float)y, cy);
    const float mag = rn_sqrtf(__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy)));
    const float ang = __fmul_rn(wp_fast_atan2_deg(fy, fx), (float)(WP_PI / 180.0));
    const float p = LOG ? (float)log((double)__fadd_rn(mag, 1.f)) : mag;
    const float mx = (float)__ddiv_rn((double)p, Kmag), my = __fadd_rn((float)__ddiv_rn((double)ang, Kangle), 1.f);
    const WpPolarTap tap = {src + img * image_stride, rows, cols, row_stride};
    dst[(img * dh + y) * dw + x] = wp_remap(tap, mx, my);
}

// Cartesian (rows x cols per image) -> dh x dw polar per image; br[rho] the radius, cs[2 phi], cs[2 phi + 1] = cos, sin of the angle
__global__ __launch_bounds__(256) void warp_polar_forward_kernel(const float *__restrict__ src, int rows, int cols, int64_t row_stride,
                                                                 int64_t image_stride, float *__restrict__ dst, int dw, int dh, float cx,
                                                                 float cy, const float *__restrict__ br, const double *__restrict__ cs)
{
    const int rho = blockIdx.x * blockDim.x + threadIdx.x, phi = blockIdx.y;
    if (rho >= dw) return;
    const int64_t img = blockIdx.z;
    const double b = (double)br[rho], cp = cs[2 * phi], sp = cs[2 * phi + 1];
    const float mx = (float)__dadd_rn(__dmul_rn(b, cp), (double)cx), my = (float)__dadd_rn(__dmul_rn(b, sp), (double)cy);
    const WpCartTap tap = {src + img * image_stride, rows, cols, row_stride};
    dst[(img * dh + phi) * dw + rho] = wp_remap(tap, mx, my);
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
    // pack the images tightly on the way up (a column slice of a wider record travels without its unused columns)
    if (n == 1 || src_image_stride == (int64_t)rows * src_row_stride)
        HIP_TRY(ctx, hipMemcpy2DAsync(d_in, sizeof(float) * cols, src, sizeof(float) * src_row_stride, sizeof(float) * cols,
                                      (size_t)rows * n, hipMemcpyHostToDevice, st));
    else
        for (int i = 0; i < n; i++)
            HIP_TRY(ctx, hipMemcpy2DAsync(d_in + i * nin, sizeof(float) * cols, src + i * src_image_stride, sizeof(float) * src_row_stride,
                                          sizeof(float) * cols, rows, hipMemcpyHostToDevice, st));
    std::vector<unsigned char> tab;
    const float *d_br = nullptr;
    const double *d_cs = nullptr;
    if (!inverse) {
        // OpenCV's host tables (imgwarp.cpp, warpPolar): Kmag and Kangle from the DESTINATION size
        tab.resize(sizeof(double) * 2 * dh + sizeof(float) * dw);
        double *cs = (double *)tab.data();
        float *br = (float *)(cs + 2 * dh);
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
