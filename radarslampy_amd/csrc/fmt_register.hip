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
//   fmtr_angle_matrix_kernel   the in-step pass only (roam_engine_set_auto_prior): what the host does between the two correlations of the
//                              blocking pass - the rotation correlation's shift as an angle, rotateImg's matrix for it, inverted - one
//                              thread per pair, float64, the host's operations in the host's order; only cos and sin are the device
//                              library's instead of the host's.
//   fmtr_prior_kernel          the in-step pass only: FMT.flowPriorFromFMT behind the second correlation, one thread per lane - the
//                              affine the lane's tracker starts from, its use byte and the lane's record.
// The polar map, the affine fixed point, the remap and the window product are cvmap.h's, the same definitions warppolar.hip,
// warpaffine.hip and pc_window_kernel call.  The correlation behind it is phasecorr.hip's, the driver fmt.hip's (roam_fmt_register_run): these kernels only fill
// its planes.  No atomics: every output element has one writer, and an image's result does not depend on its place in the batch.
// One thread per output pixel in a 32 x 8 tile, as warp_affine_kernel: a tile's taps lie in a compact patch of the source (a sector
// of the polar image, a turned rectangle of the Cartesian one), so its lines are shared through the L1 and the L2; stores are coalesced.
#include "cvmap.h"
#include "fmt.h"

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
// plane z + plane_gap (their planes lie behind the work planes of the transforms, phasecorr.hip).  win: the window factor per row (S
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

// pair i: rot3[3 i + 1] = the shift along the angle axis of the log-polar correlation.  FMT.py:84-90 for the angle (fmt.hip's blocking
// pass: the same expression), then roam_rotation_inverse_map's arithmetic about (c, c) with the device's cos / sin
__global__ __launch_bounds__(64) void fmtr_angle_matrix_kernel(const double *__restrict__ rot3, int n, int sz, double c, double *__restrict__ ang,
                                                               double *__restrict__ Minv)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double angle = roam_normalize_angle(-rot3[3 * i + 1] * 2.0 * M_PI / (double)sz);
    const double deg = angle * (180.0 / M_PI), rad = deg * M_PI / 180.0;
    double M[6], inv[6];
    cv_rotation_matrix(cos(rad), sin(rad), c, c, M);
    cv_invert_affine(M, inv);
    ang[i] = angle;
    for (int k = 0; k < 6; k++) Minv[6 * (int64_t)i + k] = inv[k];
}

// lane b: FMT.flowPriorFromFMT(angle, (dx, dy)) in float64 in its order - getRotationMatrix2D about (c, c), M[:, 2] = s (M[:, 2] + (dx, dy)),
// every entry rounded once to float32 - the gate (finite numbers, both responses at or above their minimum, roam_engine_set_motion_prior's
// limits on the affine) and the lane's record.  Plain stores, one writer per element
__global__ __launch_bounds__(64) void fmtr_prior_kernel(FmtPriorArgs a)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const int p = a.pair_of[b];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double v[7] = {nan, nan, nan, nan, nan, nan, nan};
    float f[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    bool use = false;
    if (p >= 0) {
        v[0] = a.rot3[3 * p]; v[1] = a.rot3[3 * p + 1]; v[2] = a.rot3[3 * p + 2];
        v[3] = a.ang[p];
        v[4] = a.trans3[3 * p]; v[5] = a.trans3[3 * p + 1]; v[6] = a.trans3[3 * p + 2];
        const double deg = v[3] * (180.0 / M_PI), rad = deg * M_PI / 180.0;
        double M[6];
        cv_rotation_matrix(cos(rad), sin(rad), a.c, a.c, M);
        M[2] = a.s * (M[2] + v[4]); M[5] = a.s * (M[5] + v[5]);
        use = v[2] >= a.min_rot && v[6] >= a.min_trans;
        for (int k = 0; k < 7; k++) use = use && isfinite(v[k]);
        for (int k = 0; k < 6; k++) {
            f[k] = (float)M[k];
            use = use && fabsf(f[k]) <= ((k % 3 == 2) ? ROAM_KLT_MAX_GUESS : ROAM_PRIOR_MAX_LINEAR);       // (NaN fails it too)
        }
    }
    float *slot = reinterpret_cast<float *>(a.prior_slot) + 6 * (int64_t)b;
    FmtPriorRec *r = a.rec + b;
    for (int k = 0; k < 7; k++) r->v[k] = v[k];
    for (int k = 0; k < 6; k++) { slot[k] = f[k]; r->affine[k] = f[k]; }
    a.prior_slot[24 * (int64_t)a.B + b] = use ? 1 : 0;
    r->source = use ? 1 : 0;
    for (int k = 0; k < 7; k++) r->pad[k] = 0;
}

hipError_t launch_fmtr_angle_matrix(hipStream_t st, const double *rot3, int n, int sz, double c, double *ang, double *Minv)
{
    hipLaunchKernelGGL(fmtr_angle_matrix_kernel, dim3((n + 63) / 64), dim3(64), 0, st, rot3, n, sz, c, ang, Minv);
    return hipGetLastError();
}

hipError_t launch_fmtr_prior(hipStream_t st, const FmtPriorArgs &a)
{
    hipLaunchKernelGGL(fmtr_prior_kernel, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
    return hipGetLastError();
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
