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
// The polar map, the affine fixed point, the remap and the window product are cvmap.h's, the same definitions warppolar.hip,
// warpaffine.hip and pc_window_kernel call.  The correlation behind it is fft.hip's (roam_fmt_register_run): these kernels only fill
// its planes.  No atomics: every output element has one writer, and an image's result does not depend on its place in the batch.
// One thread per output pixel in a 32 x 8 tile, as warp_affine_kernel: a tile's taps lie in a compact patch of the source (a sector
// of the polar image, a turned rectangle of the Cartesian one), so its lines are shared through the L1 and the L2; stores are coalesced.
#include "cvmap.h"

#define FMTR_TILE_X 32
#define FMTR_TILE_Y 8

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
    float mx, my;
    cv_polar_inverse_map<false>(x, y, (float)Rc, (float)Rc, Kmag, Kangle, mx, my);
    const CvPolarTap<U8> tap = {p, rows, cols, s.row_stride, 0};
    cart[(z * S + y) * S + x] = cv_remap(tap, mx, my);
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
            int X, Y;
            cv_affine_fixed32(Minv + z * 6, x, y, X, Y);
            const CvCartTap tap = {p, S, S, (int64_t)S};
            v = cv_remap(tap, X, Y);
            if (rot_out) rot_out[(z * S + y) * S + x] = v;
        } else {
            v = p[(int64_t)y * S + x];
        }
        val = (double)cv_hanning_product(win[y], win[S + x], v);
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
