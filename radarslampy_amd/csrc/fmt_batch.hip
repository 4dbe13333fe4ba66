// Front end of the Fourier-Mellin rotation prior (FMT.getRotationUsingFMT, reference FMT.py:36-90), the only one: for 2 nb images at
// once (a single pair is nb = 1), the image in grid.z: the first nb are the sources of a chunk of pairs, the next nb their targets.
//   fmtb_resize_kernel    cv2.resize(img[:, :clip], (R, rows)), INTER_LINEAR, R = clip / downsample.  The source is a float32 polar
//                         image (row and image stride) or a u8 record read in place (float(u8) / 255.0f in float32,
//                         extractDataFromRadarImage's arithmetic; the engine's pool through a list of record indices).
//   fmtb_cart_kernel      inverse linear warpPolar to 2R x 2R, centre (R, R), maxRadius R (convertPolarImgToLogPolar, parseData.py:138-160)
//   fmtb_logpolar_kernel  forward semilog warpPolar to round(R) x round(pi R), [the image before the window -> lp_out,] times the
//                         cv2.createHanningWindow factor, rounded to float32, zero-padded into the float64 M x N plane of the FFT
// The maps, the remap and the window product are cvmap.h's, the same definitions warppolar.hip calls; like warppolar.hip the
// radius, cos / sin and window tables come from the host's libm, so that the log-polar image equals the oracle's bit for bit.
// The correlation behind it is phasecorr.hip's, the driver fmt.hip's (roam_fmt_batch_run): these kernels only fill its planes.  No atomics: every output element
// has one writer, and an image's result does not depend on its place in the batch.
#include "cvmap.h"
#include "fmt.h"

// grid (ceil(nw / 64), rows, images): out[z] = rows x nw, two taps per output column, rows untouched
template <bool U8>
__global__ __launch_bounds__(64) void fmtb_resize_kernel(FmtBatchSrc s, int rows, int clip, int nw, float *__restrict__ out)
{
    const int dx = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y, z = blockIdx.z;
    if (dx >= nw) return;
    const double scale = 1.0 / ((double)nw / (double)clip);
    float fx = (float)(((double)dx + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx = __fsub_rn(fx, (float)sx);
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= clip - 1) { fx = 0.f; sx = clip - 1; }
    const int sx1 = min(sx + 1, clip - 1);
    const int64_t img = s.index ? (int64_t)s.index[z] : (int64_t)z;
    float s0, s1;
    if (U8) {
        const uint8_t *p = (const uint8_t *)s.base + img * s.image_stride + (int64_t)r * s.row_stride + s.payload_off;
        s0 = __fdiv_rn((float)p[sx], 255.f); s1 = __fdiv_rn((float)p[sx1], 255.f);
    } else {
        const float *p = (const float *)s.base + img * s.image_stride + (int64_t)r * s.row_stride;
        s0 = p[sx]; s1 = p[sx1];
    }
    out[((int64_t)z * rows + r) * nw + dx] = __fadd_rn(__fmul_rn(s0, __fsub_rn(1.f, fx)), __fmul_rn(s1, fx));
}

// grid (ceil(2R / 64), 2R, images): small[z] (rows x R) -> cart[z] (2R x 2R); Kmag = maxRadius / cols = 1
__global__ __launch_bounds__(64) void fmtb_cart_kernel(const float *__restrict__ small, int rows, int R, float *__restrict__ cart)
{
    const int W = 2 * R;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int64_t z = blockIdx.z;
    const double Kangle = 6.283185307179586476925286766559 / (double)rows, Kmag = (double)R / (double)R;
    float mx, my;
    cv_polar_inverse_map<false>(x, y, (float)R, (float)R, Kmag, Kangle, mx, my);
    const CvPolarTap<false> tap = {small + z * rows * R, rows, R, (int64_t)R, 0};
    cart[(z * W + y) * W + x] = cv_remap(tap, mx, my);
}

// grid (ceil(N / 64), M, images): cart[z] -> the M x N plane of image z (zero outside dh x dw).  Image z < nb writes plane z, the others
// plane z + plane_gap (the targets' planes lie behind the work planes of the transforms, phasecorr.hip).  tab: cos, sin per row (2 dh
// doubles) | window factor per row (dh) | per column (dw); br: the radius per column (dw floats).  lp_out (optional): images x dh x dw.
__global__ __launch_bounds__(64) void fmtb_logpolar_kernel(const float *__restrict__ cart, int R, int dw, int dh, int M, int N, int nb,
                                                           int64_t plane_gap, const double *__restrict__ tab, const float *__restrict__ br,
                                                           double *__restrict__ planes, float *__restrict__ lp_out)
{
    const int rho = blockIdx.x * 64 + threadIdx.x, phi = blockIdx.y;
    if (rho >= N) return;
    const int64_t z = blockIdx.z;
    const int W = 2 * R;
    double val = 0.0;
    if (rho < dw && phi < dh) {
        const double *cs = tab, *wr = tab + 2 * dh, *wc = wr + dh;
        float mx, my;
        cv_polar_forward_map((double)br[rho], cs[2 * phi], cs[2 * phi + 1], (double)(float)R, (double)(float)R, mx, my);
        const CvCartTap tap = {cart + z * W * W, W, W, (int64_t)W};
        const float v = cv_remap(tap, mx, my);
        if (lp_out) lp_out[(z * dh + phi) * dw + rho] = v;
        val = (double)cv_hanning_product(wr[phi], wc[rho], v);
    }
    const int64_t plane = z < nb ? z : z + plane_gap;
    planes[(plane * M + phi) * N + rho] = val;
}

hipError_t launch_fmt_batch_front(hipStream_t st, const FmtBatchSrc &src, int nb, int rows, int clip, int R, int dw, int dh, int M, int N,
                                  const double *tab, const float *br, float *small, float *cart, double *planes, int64_t plane_gap,
                                  float *lp_out)
{
    const int W = 2 * R, nimg = 2 * nb;
    const dim3 g0((R + 63) / 64, rows, nimg);
    if (src.is_u8) hipLaunchKernelGGL(fmtb_resize_kernel<true>, g0, dim3(64), 0, st, src, rows, clip, R, small);
    else hipLaunchKernelGGL(fmtb_resize_kernel<false>, g0, dim3(64), 0, st, src, rows, clip, R, small);
    hipLaunchKernelGGL(fmtb_cart_kernel, dim3((W + 63) / 64, W, nimg), dim3(64), 0, st, small, rows, R, cart);
    hipLaunchKernelGGL(fmtb_logpolar_kernel, dim3((N + 63) / 64, M, nimg), dim3(64), 0, st, cart, R, dw, dh, M, N, nb, plane_gap, tab, br,
                       planes, lp_out);
    return hipGetLastError();
}
