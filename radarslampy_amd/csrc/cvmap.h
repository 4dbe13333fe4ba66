// OpenCV's coordinate maps and its bilinear remap (imgwarp.cpp: warpPolar, warpAffine, remap with INTER_LINEAR on CV_32F), one
// definition of each piece for every unit that samples an image the way cv2 does: warp.hip, warppolar.hip, warpaffine.hip, fmt_batch.hip,
// fmt_register.hip, phasecorr.hip.  Bit-exactness with the oracle rests on these lines, so they are written with explicit
// IEEE round-to-nearest intrinsics and compiled without contraction (roam_internal.h).
//   maps:   a float coordinate (mx, my) per output pixel - the inverse polar map (cartToPolar = sqrt + the degree-7 fastAtan
//           polynomial, [log(mag + 1)], the two float64 divides, one wrapped border row above the source), the forward polar map from
//           host tables - or warpAffine's 1/1024 fixed point, which yields 1/32-px coordinates directly.
//   remap:  coordinates in 1/32 px (cvRound, half to even), tap index saturated to int16, weights wy * wx from (frac / 32,
//           1 - frac / 32), four taps summed in OpenCV's order; what lies outside the source is the tap functor's business (both
//           functors here read 0 there: BORDER_CONSTANT, WARP_FILL_OUTLIERS).
#pragma once
#include "roam_internal.h"

#define CVM_PI 3.14159265358979323846

// cv::fastAtan2 (degrees, [0, 360))
__device__ __forceinline__ float cv_fast_atan2_deg(float y, float x)
{
    const float sc = (float)(180 / CVM_PI);
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

// warpPolar with WARP_INVERSE_MAP: destination pixel (x, y) -> (mx, my) in the polar source PADDED with one wrapped row above (the
// + 1); Kmag = maxRadius / cols (LOG: log(maxRadius) / cols), Kangle = 2 pi / rows.  LOG takes (float)log((double)(mag + 1)) where
// OpenCV uses hal::log32f (docs/PARITY.md)
template <bool LOG>
__device__ __forceinline__ void cv_polar_inverse_map(int x, int y, float cx, float cy, double Kmag, double Kangle, float &mx, float &my)
{
    const float fx = __fsub_rn((float)x, cx), fy = __fsub_rn((float)y, cy);
    const float mag = rn_sqrtf(__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy)));
    const float ang = __fmul_rn(cv_fast_atan2_deg(fy, fx), (float)(CVM_PI / 180.0));
    const float p = LOG ? (float)log((double)__fadd_rn(mag, 1.f)) : mag;
    mx = (float)__ddiv_rn((double)p, Kmag);
    my = __fadd_rn((float)__ddiv_rn((double)ang, Kangle), 1.f);
}

// forward warpPolar: br the radius of the destination column, (cp, sp) = cos, sin of the destination row's angle
__device__ __forceinline__ void cv_polar_forward_map(double br, double cp, double sp, double cx, double cy, float &mx, float &my)
{
    mx = (float)__dadd_rn(__dmul_rn(br, cp), cx);
    my = (float)__dadd_rn(__dmul_rn(br, sp), cy);
}

// a float coordinate in 1/32 px: cvRound(m * INTER_TAB_SIZE)
__device__ __forceinline__ int cv_fixed32(float m) { return __float2int_rn(__fmul_rn(m, 32.f)); }

// saturate_cast<int>(double): nearest-even, saturated (the clamp is explicit: a float-to-int conversion out of range is undefined)
__device__ __forceinline__ unsigned cv_round_sat(double v) { return (unsigned)(int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); }

// warpAffine: destination pixel (x, y) and the INVERSE matrix m (6 doubles, destination -> source) -> (X, Y) in 1/32 px.
// AB_SCALE = 1024: adelta = cvRound(m0 x 1024), X0 = cvRound((m1 y + m2) 1024) + 16, X = (X0 + adelta) >> 5; the int32 sums wrap
// (unsigned arithmetic)
__device__ __forceinline__ void cv_affine_fixed32(const double *__restrict__ m, int x, int y, int &X, int &Y)
{
    const double dx = (double)x, dy = (double)y;
    const unsigned adelta = cv_round_sat(__dmul_rn(__dmul_rn(m[0], dx), 1024.0));
    const unsigned bdelta = cv_round_sat(__dmul_rn(__dmul_rn(m[3], dx), 1024.0));
    const unsigned X0 = cv_round_sat(__dmul_rn(__dadd_rn(__dmul_rn(m[1], dy), m[2]), 1024.0)) + 16u;
    const unsigned Y0 = cv_round_sat(__dmul_rn(__dadd_rn(__dmul_rn(m[4], dy), m[5]), 1024.0)) + 16u;
    X = (int)(X0 + adelta) >> 5;
    Y = (int)(Y0 + bdelta) >> 5;
}

// OpenCV's invertAffineTransform as warpAffine applies it in place, float64 (no fused multiply-add: roam_internal.h); a singular matrix
// becomes all zeros.  Host and device: the host entries invert with it, fmtr_angle_matrix_kernel on the device
__host__ __device__ inline void cv_invert_affine(const double *in, double *M)
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

// cv2.getRotationMatrix2D((cx, cy), degrees, 1.0) from the cosine and sine of the angle (the caller's libm makes them): 6 doubles
__host__ __device__ inline void cv_rotation_matrix(double a, double b, double cx, double cy, double *M)
{
    M[0] = a; M[1] = b; M[2] = (1 - a) * cx - b * cy;
    M[3] = -b; M[4] = a; M[5] = b * cx + (1 - a) * cy;
}

// saturate_cast<short>(s >> INTER_BITS)
__device__ __forceinline__ int cv_tap_index(int s) { return min(max(s >> 5, -32768), 32767); }

// the bilinear sample at (sx, sy) in 1/32 px; tap(row, column) reads one source element
template <class Tap>
__device__ __forceinline__ float cv_remap(const Tap &tap, int sx, int sy)
{
    const int ix = cv_tap_index(sx), iy = cv_tap_index(sy);
    const float wx1 = __fmul_rn((float)(sx & 31), 1.f / 32.f), wx0 = __fsub_rn(1.f, wx1);
    const float wy1 = __fmul_rn((float)(sy & 31), 1.f / 32.f), wy0 = __fsub_rn(1.f, wy1);
    float v = __fmul_rn(tap(iy, ix), __fmul_rn(wy0, wx0));
    v = __fadd_rn(v, __fmul_rn(tap(iy, ix + 1), __fmul_rn(wy0, wx1)));
    v = __fadd_rn(v, __fmul_rn(tap(iy + 1, ix), __fmul_rn(wy1, wx0)));
    v = __fadd_rn(v, __fmul_rn(tap(iy + 1, ix + 1), __fmul_rn(wy1, wx1)));
    return v;
}

template <class Tap>
__device__ __forceinline__ float cv_remap(const Tap &tap, float mx, float my)
{
    return cv_remap(tap, cv_fixed32(mx), cv_fixed32(my));
}

// polar source with its wrapped border rows: py indexes the padded image (rows + 2), 0 -> row rows - 1, rows + 1 -> row 0.
// U8: rows of u8 codes (stride in bytes, the payload payload_off bytes into a row), decoded as float(code) / 255.0f; else float32
// rows (stride in floats)
template <bool U8>
struct CvPolarTap {
    const void *p; int rows, cols; int64_t stride; int payload_off;
    __device__ __forceinline__ float operator()(int py, int px) const
    {
        if (px < 0 || px >= cols || py < 0 || py >= rows + 2) return 0.f;
        int r = py - 1;
        if (r < 0) r += rows; else if (r >= rows) r -= rows;
        if (U8) return __fdiv_rn((float)(reinterpret_cast<const uint8_t *>(p) + (int64_t)r * stride + payload_off)[px], 255.f);
        return (reinterpret_cast<const float *>(p) + (int64_t)r * stride)[px];
    }
};

// Cartesian float32 source, zero outside
struct CvCartTap {
    const float *p; int rows, cols; int64_t stride;
    __device__ __forceinline__ float operator()(int y, int x) const
    {
        return (x < 0 || x >= cols || y < 0 || y >= rows) ? 0.f : p[(int64_t)y * stride + x];
    }
};

// cv2.createHanningWindow's factor sqrt(float32(wr wc)) from the float64 row and column factors, times the pixel, rounded to float32
__device__ __forceinline__ float cv_hanning_product(double wr, double wc, float v)
{
    return __fmul_rn(rn_sqrtf((float)(wr * wc)), v);
}
