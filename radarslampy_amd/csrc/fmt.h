// fmt.h - the Fourier-Mellin family: the front-end kernels' launchers (fmt_batch.hip, fmt_register.hip) and the passes that drive them
// and the correlation core (fmt.hip); internal, for fmt*.hip, the engine's units and the stand-alone sanitizer program.  Overview: fmt.hip.
#pragma once
#include "fft.h"

// fmt_batch.hip: the batched front end of the rotation prior.  Image z of a launch reads base + (index ? index[z] : z) * image_stride
// (+ payload_off for u8 records); strides in elements (floats or bytes); base and index are device pointers
struct FmtBatchSrc {
    const void *base;
    int64_t image_stride, row_stride;
    int32_t payload_off, is_u8;
    const int32_t *index;
};
// 2 nb images (nb sources, then nb targets): resize to rows x R, inverse warpPolar to 2R x 2R (cart), semilog warpPolar to dh x dw,
// window, zero-padded M x N float64 planes: image z < nb -> planes + z M N, the others -> planes + (z + plane_gap) M N.
// tab: roam_warp_polar_tables' cs (2 dh doubles) | roam_hanning_factors per row (dh) | per column (dw); br: its radius per column;
// small: 2 nb x rows x R floats, cart: 2 nb x 2R x 2R floats, lp_out (optional): 2 nb x dh x dw floats, the images before the window
hipError_t launch_fmt_batch_front(hipStream_t st, const FmtBatchSrc &src, int nb, int rows, int clip, int R, int dw, int dh, int M, int N,
                                  const double *tab, const float *br, float *small, float *cart, double *planes, int64_t plane_gap,
                                  float *lp_out);
// fmt.hip: FMT.getRotationUsingFMT for n pairs on ctx->stream, blocking (one stream synchronisation per chunk of pairs).  Either
// host float32 images (host_src / host_tgt, n each, strides in floats, `cols` columns per row) or resident u8 records (pool; pair i is
// the records prev_idx[i], curr_idx[i], host arrays).  clip = range bins kept, R = columns after the resize.  The caller has checked
// the arguments.  out3: n x 3 {angle_rad, scale, response}; logpolar_out: optional, 2 n x dh x dw
struct FmtBatchIn {
    const float *host_src = nullptr, *host_tgt = nullptr;
    int64_t row_stride = 0, image_stride = 0;
    int32_t cols = 0;
    const uint8_t *pool = nullptr;
    int64_t rec_bytes = 0, rec_stride = 0;
    int32_t payload_off = 0;
    const int32_t *prev_idx = nullptr, *curr_idx = nullptr;
};
int32_t roam_fmt_batch_run(roam_ctx *ctx, const FmtBatchIn &in, int n, int rows, int clip, int R, double *out3, float *logpolar_out);

// fmt_register.hip: the front end of the translation half of the Fourier-Mellin registration.  launch_fmtr_cart: nimg polar images
// (FmtBatchSrc, rows x cols, read in place) -> cart (nimg x 2Rc x 2Rc floats), the inverse linear warpPolar with centre (Rc, Rc) and
// maxRadius Rc.  launch_fmtr_rotate_window: cart = nb sources, then nb targets, S x S each; source z is turned by Minv + 6 z
// (destination -> source), [stored to rot_out, nb x S x S,] windowed (win: S row factors, then S column factors) and zero-padded into
// plane z of M x N doubles, target z into plane z + plane_gap.
hipError_t launch_fmtr_cart(hipStream_t st, const FmtBatchSrc &src, int nimg, int rows, int cols, int Rc, float *cart);
hipError_t launch_fmtr_rotate_window(hipStream_t st, const float *cart, int S, int M, int N, int nb, int64_t plane_gap, const double *Minv,
                                     const double *win, double *planes, float *rot_out);
// fmt.hip: the registration of n pairs on ctx->stream, blocking: per chunk of pairs the rotation half (one synchronisation: the
// angles come to the host, which makes the matrices), then the Cartesian images, the turn, the window and the second correlation (one
// more).  `in` as for roam_fmt_batch_run, in.cols = the polar width the Cartesian half reads (all of it); Rc = in.cols / cart_downsample.
// out6: n x 6 {angle_rad, scale, rot_response, dx, dy, trans_response}; cart_out: optional, 2 n x 2Rc x 2Rc (turned sources, targets)
int32_t roam_fmt_register_run(roam_ctx *ctx, const FmtBatchIn &in, int n, int rows, int clip, int R, int Rc, double *out6, float *cart_out);

// ---------------------------------------------------------------- the workspace of a pass
// The sizes of a pass: rotation only (Rc = 0), rotation + translation, or the in-step pass (lanes > 0: the per-pair results are kept for
// all lanes, and the index lists live in a ring of 4 slots of 3 lanes ints).  nin: floats of one host input image that the pass uploads
// (0: resident records, read through 2 chunk indices); lp / rot: the log-polar / turned-source images are kept for a copy to the host
struct FmtPass {
    int rows, R, Rc;
    size_t chunk, lanes, nin;
    bool lp, rot;
};
// every device buffer of a pass.  in: 2 chunk host images; tab: fmt.hip's rotation tables; win: 2 x 2Rc window factors; pc: the
// correlation workspace, planes and partial maxima sized for the larger half, pc.out = the rotation's results (blocking: the
// translation's too, once the host has the rotation's); small, cart_r / cart_t: the front ends' images of the two halves;
// trans3, ang: the in-step pass's translation results and angles; M: 6 doubles per pair.  Null: not in this pass
struct FmtWork {
    int32_t *idx;
    float *in;
    unsigned char *tab;
    double *win;
    PcWork pc;
    float *small, *cart_r, *cart_t, *lp, *rot;
    double *trans3, *ang, *M;
};
// lays the buffers out in `slab`, each on a 256-byte boundary, and returns the bytes of the slab; a null slab only counts
FFT_UNIT size_t fmt_carve(const FmtPass &s, uint8_t *slab, FmtWork *w);
// bytes of device memory per pair of the two halves, which decide the pairs per chunk.  nin as above (a half that reads images the
// other uploaded counts none), lp / rot as above
FFT_UNIT size_t fmt_rot_bytes_per_pair(int rows, int R, size_t nin, bool lp);
FFT_UNIT size_t fmt_trans_bytes_per_pair(int Rc, size_t nin, bool rot);

// ---------------------------------------------------------------- in-step motion prior (roam_engine_set_auto_prior)
// One record per lane and step, written by fmtr_prior_kernel: v = {shift_x, shift_y, rot_response, angle, dx, dy, trans_response}
// (NaN for a lane without a registration), the affine the tracker was given, source 0 = unseeded, 1 = in-step registration
struct FmtPriorRec {
    double v[7];
    float affine[6];
    uint8_t source, pad[7];
};
// fmt_register.hip: the two kernels that stand in for the host between and behind the two correlations of the in-step pass.
// launch_fmtr_angle_matrix: pair i of n reads rot3 + 3 i = {shift_x, shift_y, response} of the rotation correlation and writes its
// angle (ang + i; sz = the larger side of the log-polar image) and the inverse rotation about (c, c) (Minv + 6 i) that
// launch_fmtr_rotate_window reads.
hipError_t launch_fmtr_angle_matrix(hipStream_t st, const double *rot3, int n, int sz, double c, double *ang, double *Minv);
// launch_fmtr_prior: lane b of B with pair_of[b] = p >= 0 takes rot3 / ang / trans3 of pair p, makes FMT.flowPriorFromFMT's affine
// (rotation about (c, c), translation scaled by s) and writes it with its use byte into prior_slot (B x 6 f32, then B bytes: what
// launch_klt reads) and, with the numbers, into rec[b]; pair_of[b] < 0: the identity, use 0, NaN numbers
struct FmtPriorArgs {
    const int32_t *pair_of;
    const double *rot3, *ang, *trans3;
    int B;
    double c, s, min_rot, min_trans;
    uint8_t *prior_slot;
    FmtPriorRec *rec;
};
hipError_t launch_fmtr_prior(hipStream_t st, const FmtPriorArgs &a);

// fmt.hip: the in-step registration pass.  roam_fmt_auto_plan is host arithmetic only (sizes, bytes per pair, pairs per chunk, the
// bytes of the one device slab the pass lives in); roam_fmt_auto_init carves the caller's slab, uploads the host tables of both halves
// and makes the twiddle tables (blocking, on ctx->stream); roam_fmt_auto_enqueue only enqueues on st: the index lists of the step
// (staged in pinned memory of the pass, ring slot slot4), per chunk the rotation half, fmtr_angle_matrix_kernel and the translation
// half, then fmtr_prior_kernel for all lanes.
struct FmtAutoCfg {
    int rows, cols, clip, R, Rc, lanes;          // cols: the record's clipped width (the Cartesian half reads all of it)
    double min_rot, min_trans;
};
struct FmtAutoPlan {
    size_t per_pair, chunk, slab_bytes;
    int sz;                                      // larger side of the log-polar image: shift_y -> angle
    double log_base;                             // shift_x -> scale
};
struct FmtAuto;
int32_t roam_fmt_auto_plan(roam_ctx *ctx, const FmtAutoCfg &cfg, FmtAutoPlan *plan);
int32_t roam_fmt_auto_init(roam_ctx *ctx, const FmtAutoCfg &cfg, const FmtAutoPlan &plan, uint8_t *slab, FmtAuto **out);
void roam_fmt_auto_free(FmtAuto *a);
// prev / curr: npairs pool indices (host), pair_of: lanes (host); pool as FmtBatchIn describes it; rec_slot: lanes records (device)
int32_t roam_fmt_auto_enqueue(roam_ctx *ctx, FmtAuto *a, hipStream_t st, const FmtBatchIn &pool, int slot4, int npairs, const int32_t *prev,
                              const int32_t *curr, const int32_t *pair_of, uint8_t *prior_slot, FmtPriorRec *rec_slot);
// FMT.py:84-90 on the host, the blocking pass's own expressions: a record's raw shifts -> angle (what the device wrote) and scale
double roam_fmt_scale(double log_base, double shift_x);
