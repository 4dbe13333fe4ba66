// Front end of the translation half of the Fourier-Mellin scan registration (roam_fmt_register_batch_f32, roam_engine_fmt_register:
// the rotation of FMT.py:211-250, rotateImg(prevImgCart, rotDeg) of plotCartPolarWithRotation, FMT.py:134-168, then a second phase
// correlation on the de-rotated Cartesian images) for the 2 nb scans of a chunk of pairs, the image in grid.z: the first nb are the
// sources, the next nb their targets.
//   fmtr_cart_kernel           convertPolarImageToCartesian(., downsampleFactor = cart_downsample): inverse linear warpPolar of the
//                              full-width polar image to 2Rc x 2Rc, Rc = cols / cart_downsample, centre (Rc, Rc), maxRadius Rc.  The
//                              source is read in place: a float32 polar image (row and image stride) or a u8 record
//                              (float(u8) / 255.0f, the engine's pool through a list of record indices; no float32 polar copy is made).
//   fmtr_rotate_window_kernel  sources: rotateImg(cart, degrees(angle)) - a gather with the pair's own inverse matrix (made and inverted
//                              on the host in float64) - [the rotated image -> rot_out,] times the cv2.createHanningWindow factor,
//                              rounded to float32, zero-padded into the float64 M x N plane of the FFT; targets: the window only.
// The arithmetic is warppolar.hip's, warpaffine.hip's and pc_window_kernel's operation for operation (explicit __f*_rn, no
// contraction).  The correlation behind it is fft.hip's (roam_fmt_register_run): these kernels only fill its planes.  No atomics: every
// output element has one writer, and an image's result does not depend on its place in the batch.
// One thread per output pixel in a 32 x 8 tile, as warp_affine_kernel: a tile's taps lie in a compact patch of the source (a sector
// of the polar image, a turned rectangle of the Cartesian one), so its lines are shared through the L1 and the L2; stores are coalesced.
#include "roam_internal.h"

#define FMTR_PI 3.14159265358979323846
#define FMTR_TILE_X 32
#define FMTR_TILE_Y 8

// (the helpers below restate wp_fast_atan2_deg / wp_tap_index of warppolar.hip and wa_round of warpaffine.hip, local to those units)
__device__ __forceinline__ float fmtr_fast_atan2_deg(float y, float x)
{
    const float sc = (float)(180 / FMTR_PI);
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

__device__ __forceinline__ int fmtr_tap_index(int s) { return min(max(s >> 5, -32768), 32767); }

__device__ __forceinline__ unsigned fmtr_round(double v) { return (unsigned)(int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); }

// the polar source with its wrapped border rows: py indexes the padded image (rows + 2), 0 -> row rows - 1, rows + 1 -> row 0
template <bool U8>
__device__ __forceinline__ float fmtr_polar_tap(const void *img, int64_t row_stride, int rows, int cols, int py, int px)
{
    if (px < 0 || px >= cols || py < 0 || py >= rows + 2) return 0.f;
    int r = py - 1;
    if (r < 0) r += rows; else if (r >= rows) r -= rows;
    if (U8) return __fdiv_rn((float)((const uint8_t *)img)[(int64_t)r * row_stride + px], 255.f);
    return ((const float *)img)[(int64_t)r * row_stride + px];
}

__device__ __forceinline__ float fmtr_cart_tap(const float *__restrict__ p, int S, int y, int x)
{
    return (x < 0 || x >= S || y < 0 || y >= S) ? 0.f : p[(int64_t)y * S + x];
}

// grid (ceil(2Rc / 32), ceil(2Rc / 8), images): polar image z (rows x cols, in place) -> cart[z] (2Rc x 2Rc)
template <bool U8>
__global__ __launch_bounds__(FMTR_TILE_X * FMTR_TILE_Y) void fmtr_cart_kernel(FmtBatchSrc s, int rows, int cols, int Rc, float *__restrict__ cart)
{
    const int S = 2 * Rc;
    const int x = blockIdx.x * FMTR_TILE_X + threadIdx.x, y = blockIdx.y * FMTR_TILE_Y + threadIdx.y;
    if (x >= S || y >= S) return;
    const int64_t z = blockIdx.z;
    const int64_t img = s.index ? (int64_t)s.index[z] : z;
    const void *p = U8 ? (const void *)((const uint8_t *)s.base + img * s.image_stride + s.payload_off)
                       : (const void *)((const float *)s.base + img * s.image_stride);
    const double Kangle = 6.283185307179586476925286766559 / (double)rows, Kmag = (double)Rc / (double)cols;
    const float c = (float)Rc;
    const float fx = __fsub_rn((float)x, c), fy = __fsub_rn((float)y, c);
    const float mag = rn_sqrtf(__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy)));
    const float ang = __fmul_rn(fmtr_fast_atan2_deg(fy, fx), (float)(FMTR_PI / 180.0));
    const float mx = (float)__ddiv_rn((double)mag, Kmag), my = __fadd_rn((float)__ddiv_rn((double)ang, Kangle), 1.f);
    const int sx = __float2int_rn(__fmul_rn(mx, 32.f)), sy = __float2int_rn(__fmul_rn(my, 32.f));
    const int ix = fmtr_tap_index(sx), iy = fmtr_tap_index(sy);
    const float wx1 = __fmul_rn((float)(sx & 31), 1.f / 32.f), wx0 = __fsub_rn(1.f, wx1);
    const float wy1 = __fmul_rn((float)(sy & 31), 1.f / 32.f), wy0 = __fsub_rn(1.f, wy1);
    float v = __fmul_rn(fmtr_polar_tap<U8>(p, s.row_stride, rows, cols, iy, ix), __fmul_rn(wy0, wx0));
    v = __fadd_rn(v, __fmul_rn(fmtr_polar_tap<U8>(p, s.row_stride, rows, cols, iy, ix + 1), __fmul_rn(wy0, wx1)));
    v = __fadd_rn(v, __fmul_rn(fmtr_polar_tap<U8>(p, s.row_stride, rows, cols, iy + 1, ix), __fmul_rn(wy1, wx0)));
    v = __fadd_rn(v, __fmul_rn(fmtr_polar_tap<U8>(p, s.row_stride, rows, cols, iy + 1, ix + 1), __fmul_rn(wy1, wx1)));
    cart[(z * S + y) * S + x] = v;
}

// grid (ceil(N / 32), ceil(M / 8), images): cart[z] (S x S) -> the M x N plane of image z (zero outside S x S).  Image z < nb is a
// source: it is turned by Minv[z] (6 doubles, destination -> source) on the way and writes plane z; the others are targets and write
// plane z + plane_gap (their planes lie behind the work planes of the transforms, fft.hip).  win: the window factor per row (S
// doubles), then per column (S).  rot_out (optional): nb x S x S, the turned sources before the window.
__global__ __launch_bounds__(FMTR_TILE_X * FMTR_TILE_Y) void fmtr_rotate_window_kernel(const float *__restrict__ cart, int S, int M, int N, int nb,
                                                                                        int64_t plane_gap, const double *__restrict__ Minv,
                                                                                        const double *__restrict__ win,
                                                                                        double *__restrict__ planes, float *__restrict__ rot_out)
{
    const int x = blockIdx.x * FMTR_TILE_X + threadIdx.x, y = blockIdx.y * FMTR_TILE_Y + threadIdx.y;
    if (x >= N || y >= M) return;
    const int64_t z = blockIdx.z;
    double val = 0.0;
    if (x < S && y < S) {
        const float *p = cart + z * S * S;
        float v;
        if (z < nb) {
            const double *m = Minv + z * 6;
            const double dx = (double)x, dy = (double)y;
            // the int32 sums wrap (unsigned arithmetic)
            const unsigned adelta = fmtr_round(__dmul_rn(__dmul_rn(m[0], dx), 1024.0));
            const unsigned bdelta = fmtr_round(__dmul_rn(__dmul_rn(m[3], dx), 1024.0));
            const unsigned X0 = fmtr_round(__dmul_rn(__dadd_rn(__dmul_rn(m[1], dy), m[2]), 1024.0)) + 16u;
            const unsigned Y0 = fmtr_round(__dmul_rn(__dadd_rn(__dmul_rn(m[4], dy), m[5]), 1024.0)) + 16u;
            const int X = (int)(X0 + adelta) >> 5, Y = (int)(Y0 + bdelta) >> 5;
            const int ix = fmtr_tap_index(X), iy = fmtr_tap_index(Y);
            const float wx1 = __fmul_rn((float)(X & 31), 1.f / 32.f), wx0 = __fsub_rn(1.f, wx1);
            const float wy1 = __fmul_rn((float)(Y & 31), 1.f / 32.f), wy0 = __fsub_rn(1.f, wy1);
            v = __fmul_rn(fmtr_cart_tap(p, S, iy, ix), __fmul_rn(wy0, wx0));
            v = __fadd_rn(v, __fmul_rn(fmtr_cart_tap(p, S, iy, ix + 1), __fmul_rn(wy0, wx1)));
            v = __fadd_rn(v, __fmul_rn(fmtr_cart_tap(p, S, iy + 1, ix), __fmul_rn(wy1, wx0)));
            v = __fadd_rn(v, __fmul_rn(fmtr_cart_tap(p, S, iy + 1, ix + 1), __fmul_rn(wy1, wx1)));
            if (rot_out) rot_out[(z * S + y) * S + x] = v;
        } else {
            v = p[(int64_t)y * S + x];
        }
        val = (double)__fmul_rn(rn_sqrtf((float)(win[y] * win[S + x])), v);
    }
    const int64_t plane = z < nb ? z : z + plane_gap;
    planes[(plane * M + y) * N + x] = val;
}

hipError_t launch_fmtr_cart(hipStream_t st, const FmtBatchSrc &src, int nimg, int rows, int cols, int Rc, float *cart)
{
    const int S = 2 * Rc;
    const dim3 g((S + FMTR_TILE_X - 1) / FMTR_TILE_X, (S + FMTR_TILE_Y - 1) / FMTR_TILE_Y, nimg);
    if (src.is_u8) hipLaunchKernelGGL(fmtr_cart_kernel<true>, g, dim3(FMTR_TILE_X, FMTR_TILE_Y), 0, st, src, rows, cols, Rc, cart);
    else hipLaunchKernelGGL(fmtr_cart_kernel<false>, g, dim3(FMTR_TILE_X, FMTR_TILE_Y), 0, st, src, rows, cols, Rc, cart);
    return hipGetLastError();
}

hipError_t launch_fmtr_rotate_window(hipStream_t st, const float *cart, int S, int M, int N, int nb, int64_t plane_gap, const double *Minv,
                                     const double *win, double *planes, float *rot_out)
{
    const dim3 g((N + FMTR_TILE_X - 1) / FMTR_TILE_X, (M + FMTR_TILE_Y - 1) / FMTR_TILE_Y, 2 * nb);
    hipLaunchKernelGGL(fmtr_rotate_window_kernel, g, dim3(FMTR_TILE_X, FMTR_TILE_Y), 0, st, cart, S, M, N, nb, plane_gap, Minv, win, planes,
                       rot_out);
    return hipGetLastError();
}
