// Host drivers of the Fourier-Mellin family (fmt.h).  The kernels are elsewhere: the front ends that fill the planes in fmt_batch.hip
// and fmt_register.hip, the correlation in phasecorr.hip, the transform in fft.hip.
// The rotation prior (roam_fmt_rotation, roam_fmt_rotation_batch_f32, roam_engine_fmt_rotation) correlates the log-polar images of a
// pair: roam_fmt_batch_run; roam_fmt_rotation is n = 1 of it.
// The registration (roam_fmt_register_batch_f32, roam_engine_fmt_register) adds a second correlation, on the Cartesian images turned
// by the angle of the first: roam_fmt_register_run.
// Both halves are enqueue-only cores (fmt_rot_enqueue, fmt_trans_enqueue) that the blocking entries and the engine's in-step pass
// (roam_fmt_auto_enqueue, for roam_engine_set_auto_prior) share, and every pass lives in ONE slab of device memory that fmt_carve lays
// out before the first chunk: the blocking entries take it from one scratch slot, the in-step pass is given it by the engine.
#include "fmt.h"
#include <math.h>
#include <algorithm>
#include <new>

// ------------------------------------------------------------------------------------------------ sizes, tables, workspace
// the log-polar size of the rotation half and its DFT plane
struct FmtRotSize {
    int dw, dh, M, N, sz;
    size_t tab_bytes;
};
// FMT.py:84-90: the base of the log-polar radius and the scale of a shift along it
static double fmt_log_base(const FmtRotSize &g) { return exp(log((double)g.dh / 2.0) / (double)g.sz); }
static double fmt_scale(double log_base, double shift_x) { return pow(log_base, shift_x); }
static FmtRotSize fmt_rot_size(int R)
{
    FmtRotSize g;
    g.dw = (int)rint((double)R); g.dh = (int)rint((double)R * M_PI);
    g.M = optimal_dft_size(g.dh); g.N = optimal_dft_size(g.dw);
    g.sz = g.dh > g.dw ? g.dh : g.dw;
    g.tab_bytes = sizeof(double) * (3 * (size_t)g.dh + g.dw) + sizeof(float) * g.dw;
    return g;
}

// A registration holds the planes once, sized for the larger half, but counts them in both halves: its pairs per chunk were always
// reckoned so, and they stay what they were.
size_t fmt_rot_bytes_per_pair(int rows, int R, size_t nin, bool lp)
{
    const FmtRotSize g = fmt_rot_size(R);
    const size_t nsmall = (size_t)rows * R, ncart = (size_t)(2 * R) * (2 * R), nlp = lp ? (size_t)g.dh * g.dw : 0;
    return 7 * sizeof(double) * (size_t)g.M * g.N + 2 * sizeof(float) * (nsmall + ncart + nlp + nin) + 2 * sizeof(int32_t);
}
size_t fmt_trans_bytes_per_pair(int Rc, size_t nin, bool rot)
{
    const size_t S = 2 * (size_t)Rc, M = (size_t)optimal_dft_size((int)S), ncart = S * S;
    return 7 * sizeof(double) * M * M + sizeof(float) * (2 * ncart + (rot ? ncart : 0) + 2 * nin) + 6 * sizeof(double) + 2 * sizeof(int32_t);
}

size_t fmt_carve(const FmtPass &s, uint8_t *slab, FmtWork *w)
{
    const FmtRotSize g = fmt_rot_size(s.R);
    const size_t S = 2 * (size_t)s.Rc, Mt = (size_t)optimal_dft_size((int)S), L = s.lanes, per = L ? L : s.chunk;
    const size_t img2 = sizeof(float) * 2 * s.chunk;              // bytes of a chunk's 2 chunk images per float of one image
    const PcWorkBytes br = pc_work_bytes((size_t)g.M * g.N, s.chunk), bt = pc_work_bytes(Mt * Mt, s.chunk);
    const PcWorkBytes pb = {std::max(br.f, bt.f), std::max(br.pv, bt.pv), std::max(br.pi, bt.pi), sizeof(double) * 3 * per};
    Slab c{slab};
    FmtWork k;
    k.idx = c.take<int32_t>(sizeof(int32_t) * (L ? 4 * 3 * L : s.nin ? 0 : 2 * s.chunk));
    k.in = c.take<float>(img2 * s.nin);
    k.tab = c.take<unsigned char>(g.tab_bytes);
    k.win = c.take<double>(sizeof(double) * 2 * S);
    k.pc = pc_work_take(c, pb);
    k.small = c.take<float>(img2 * (size_t)s.rows * s.R);
    k.cart_r = c.take<float>(img2 * (size_t)(2 * s.R) * (2 * s.R));
    k.cart_t = c.take<float>(img2 * S * S);
    k.lp = c.take<float>(s.lp ? img2 * (size_t)g.dh * g.dw : 0);
    k.rot = c.take<float>(s.rot ? sizeof(float) * S * S * s.chunk : 0);
    k.trans3 = c.take<double>(sizeof(double) * 3 * L);
    k.ang = c.take<double>(sizeof(double) * L);
    k.M = c.take<double>(s.Rc ? sizeof(double) * 6 * per : 0);
    if (w) *w = k;
    return c.off;
}

// A blocking pass's slab: counted, taken from ONE scratch slot - once per call, before the first chunk - and carved
static int32_t fmt_scratch_slab(roam_ctx *ctx, const FmtPass &s, FmtWork *w)
{
    uint8_t *slab = (uint8_t *)roam_scratch(ctx, S_TMP2, fmt_carve(s, nullptr, nullptr));
    if (!slab) return ROAM_E_HIP;
    fmt_carve(s, slab, w);
    return ROAM_OK;
}

// OpenCV's host tables of the forward warpPolar (Kmag and Kangle from the destination size) and createHanningWindow's factors:
// cos, sin per row (2 dh doubles) | window per row (dh) | per column (dw) | radius per column (dw floats); and the window of the
// translation half: S row factors, then S column factors.  Host copies: they live until the stream has taken them
namespace {
struct FmtTables {
    std::vector<unsigned char> tab;
    std::vector<double> win;
};
}
static hipError_t fmt_tables_upload(hipStream_t st, const FmtRotSize &g, int R, int Rc, const FmtWork &w, FmtTables *t)
{
    const int S = 2 * Rc;
    t->tab.resize(g.tab_bytes); t->win.resize(2 * (size_t)S);
    double *cs = (double *)t->tab.data(), *wr = cs + 2 * g.dh, *wc = wr + g.dh;
    roam_warp_polar_tables(g.dw, g.dh, (double)(2 * R) / 2.0, true, (float *)(wc + g.dw), cs);
    roam_hanning_factors(g.dh, wr);
    roam_hanning_factors(g.dw, wc);
    roam_hanning_factors(S, t->win.data());
    roam_hanning_factors(S, t->win.data() + S);
    hipError_t e = hipMemcpyAsync(w.tab, t->tab.data(), g.tab_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && Rc) e = hipMemcpyAsync(w.win, t->win.data(), sizeof(double) * t->win.size(), hipMemcpyHostToDevice, st);
    return e;
}

// ------------------------------------------------------------------------------------------------ enqueue-only cores
// Both halves of the registration as work that is only enqueued: caller-owned device buffers, a caller-given stream, no host
// synchronisation and no allocation (the twiddle tables of the plane sizes excepted: they are made on first use, which the blocking
// entries accept and roam_fmt_auto_init forestalls).  The blocking entries below and the engine's in-step pass (roam_fmt_auto_enqueue)
// call these two and differ only in what stands between them: the host's libm or fmtr_angle_matrix_kernel.

// rotation half of nb pairs (src: nb sources, then nb targets): front end of fmt_batch.hip, correlation -> w.pc.out[3 b] = {shift_x,
// shift_y, response}.  w.tab: fmt_tables_upload's; w.pc.f: 7 nb planes of M x N doubles; w.lp optional
static int32_t fmt_rot_enqueue(roam_ctx *ctx, hipStream_t st, const FmtBatchSrc &src, int nb, int rows, int clip, int R, const FmtRotSize &g,
                               const FmtWork &w)
{
    const double *d_tabd = (const double *)w.tab;
    const float *d_br = (const float *)(d_tabd + 3 * (size_t)g.dh + g.dw);
    const PcPlanes p = pc_planes(w.pc.f, (size_t)g.M * g.N * nb);
    HIP_TRY(ctx, launch_fmt_batch_front(st, src, nb, rows, clip, R, g.dw, g.dh, g.M, g.N, d_tabd, d_br, w.small, w.cart_r, w.pc.f, (int64_t)4 * nb, w.lp));
    return pc_correlate(ctx, st, nb, g.M, g.N, w.pc, p.a, p.F[1][0]);                           // the windowed images: sources, targets
}

// translation half of nb pairs: the Cartesian images (2 nb x S x S, S = 2 Rc), the sources turned by w.M (6 doubles per pair,
// destination -> source), the window, the correlation on M x M planes -> w.pc.out[3 b] = {dx, dy, response}.  w.rot optional: the
// turned sources before the window
static int32_t fmt_trans_enqueue(roam_ctx *ctx, hipStream_t st, const FmtBatchSrc &src, int nb, int rows, int cols, int Rc, int M, const FmtWork &w)
{
    const PcPlanes p = pc_planes(w.pc.f, (size_t)M * M * nb);
    HIP_TRY(ctx, launch_fmtr_cart(st, src, 2 * nb, rows, cols, Rc, w.cart_t));
    HIP_TRY(ctx, launch_fmtr_rotate_window(st, w.cart_t, 2 * Rc, M, M, nb, (int64_t)4 * nb, w.M, w.win, w.pc.f, w.rot));
    return pc_correlate(ctx, st, nb, M, M, w.pc, p.a, p.F[1][0]);                               // the windowed images: turned sources, targets
}

// ------------------------------------------------------------------------------------------------ blocking passes
// the chunk's pairs of resident records: their index lists (host) go to d_idx, sources' then targets'
static int32_t fmt_pool_src(roam_ctx *ctx, hipStream_t st, const FmtBatchIn &in, size_t b0, int nb, int32_t *d_idx, FmtBatchSrc *src)
{
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, in.prev_idx + b0, sizeof(int32_t) * nb, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_idx + nb, in.curr_idx + b0, sizeof(int32_t) * nb, hipMemcpyHostToDevice, st));
    *src = {in.pool, in.rec_bytes, in.rec_stride, in.payload_off, 1, d_idx};
    return ROAM_OK;
}

// One chunk of the rotation half, blocking, on the buffers it is handed: the enqueue, the three numbers per pair (and the log-polar
// images, if the pass keeps them: the sources' to lp_out, the targets' lp_tgt_off floats behind) to the host, ONE stream synchronisation,
// then FMT.py:84-90 on the host: the shifts as an angle and a scale -> out3[3 i] = {angle_rad, scale, response}
static int32_t fmt_rot_chunk(roam_ctx *ctx, hipStream_t st, const FmtBatchSrc &src, int nb, int rows, int clip, int R, const FmtRotSize &g,
                             const FmtWork &w, float *lp_out, size_t lp_tgt_off, double *out3)
{
    const size_t nlp = (size_t)g.dh * g.dw * nb;
    std::vector<double> o(3 * (size_t)nb);
    FFT_TRY(fmt_rot_enqueue(ctx, st, src, nb, rows, clip, R, g, w));
    HIP_TRY(ctx, hipMemcpyAsync(o.data(), w.pc.out, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost, st));
    if (w.lp) {
        HIP_TRY(ctx, hipMemcpyAsync(lp_out, w.lp, sizeof(float) * nlp, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(lp_out + lp_tgt_off, w.lp + nlp, sizeof(float) * nlp, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const double log_base = fmt_log_base(g);
    for (int i = 0; i < nb; i++) {
        out3[3 * i] = roam_normalize_angle(-o[3 * i + 1] * 2.0 * M_PI / (double)g.sz);
        out3[3 * i + 1] = fmt_scale(log_base, o[3 * i]);
        out3[3 * i + 2] = o[3 * i + 2];
    }
    return ROAM_OK;
}

// FMT.getRotationUsingFMT for n pairs: the front end of fmt_batch.hip fills the planes, the correlation is phasecorr.hip's.  Per chunk of
// nb pairs, 7 nb planes: sources' windowed images | work re, im | F1 re, im | F2 re, im - the targets' windowed images wait in the
// F2 re planes, which nothing touches before their own row pass has consumed them.  One stream synchronisation per chunk.
int32_t roam_fmt_batch_run(roam_ctx *ctx, const FmtBatchIn &in, int n, int rows, int clip, int R, double *out3, float *logpolar_out)
{
    const FmtRotSize g = fmt_rot_size(R);
    ARG_CHECK(ctx, g.M <= FFT_MAX_N && g.N <= FFT_MAX_N);
    const bool host = in.host_src != nullptr;
    // a host image travels as whole rows when they are contiguous (one copy per image, or one per chunk), else as its first clip columns
    const bool whole_rows = host && in.row_stride == in.cols;
    const size_t in_w = whole_rows ? (size_t)in.cols : (size_t)clip, nin = host ? (size_t)rows * in_w : 0, nlp = (size_t)g.dh * g.dw;
    const size_t chunk = pc_chunk(fmt_rot_bytes_per_pair(rows, R, nin, logpolar_out != nullptr), n, 32767, true);   // 2 chunk images in grid.z
    hipStream_t st = ctx->stream;
    FmtWork w;
    FmtTables tables;
    FFT_TRY(fmt_scratch_slab(ctx, {rows, R, 0, chunk, 0, nin, logpolar_out != nullptr, false}, &w));
    HIP_TRY(ctx, fmt_tables_upload(st, g, R, 0, w, &tables));
    for (size_t b0 = 0; b0 < (size_t)n; b0 += chunk) {
        const int nb = (int)(((size_t)n - b0) < chunk ? ((size_t)n - b0) : chunk);
        FmtBatchSrc src = {w.in, (int64_t)nin, (int64_t)in_w, 0, 0, nullptr};
        if (host) {
            const float *h[2] = {in.host_src, in.host_tgt};
            for (int k = 0; k < 2; k++)
                HIP_TRY(ctx, roam_upload_packed_f32(st, w.in + (size_t)k * nb * nin, h[k] + (int64_t)b0 * in.image_stride, nb, (int)in_w, rows,
                                                    in.row_stride, in.image_stride));
        } else {
            FFT_TRY(fmt_pool_src(ctx, st, in, b0, nb, w.idx, &src));
        }
        FFT_TRY(fmt_rot_chunk(ctx, st, src, nb, rows, clip, R, g, w, logpolar_out ? logpolar_out + b0 * nlp : nullptr, (size_t)n * nlp, out3 + 3 * b0));
    }
    return ROAM_OK;
}

// what the host entries of the rotation prior check alike: the image size and the downsampling, then clip = the range bins kept
// (clip_px <= 0 or >= cols: all of them) and R = clip / downsample, the columns after the resize
static int32_t fmt_clip_radius(roam_ctx *ctx, int rows, int cols, int clip_px, int downsample, int *clip, int *R)
{
    ARG_CHECK(ctx, rows >= 8 && rows <= 16384 && cols >= 2 && downsample >= 1);
    *clip = (clip_px > 0 && clip_px < cols) ? clip_px : cols;
    *R = *clip / downsample;
    ARG_CHECK(ctx, *R >= ROAM_FMT_MIN_R && *R <= ROAM_FMT_MAX_R);
    return ROAM_OK;
}

extern "C" int32_t roam_fmt_rotation_batch_f32(roam_ctx *ctx, const float *src, const float *tgt, int32_t n, int32_t rows, int32_t cols,
                                               int64_t row_stride, int64_t image_stride, int32_t clip_px, int32_t downsample, double *out3,
                                               float *logpolar_out)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, src && tgt && out3 && n >= 1);
    int clip, R;
    FFT_TRY(fmt_clip_radius(ctx, rows, cols, clip_px, downsample, &clip, &R));
    ARG_CHECK(ctx, row_stride >= cols && (n == 1 || image_stride >= (int64_t)(rows - 1) * row_stride + cols));
    FmtBatchIn in;
    in.host_src = src; in.host_tgt = tgt; in.row_stride = row_stride; in.image_stride = n == 1 ? (int64_t)rows * row_stride : image_stride;
    in.cols = cols;
    return roam_fmt_batch_run(ctx, in, n, rows, clip, R, out3, logpolar_out);
}

// one contiguous pair: n = 1 of the batch call
extern "C" int32_t roam_fmt_rotation(roam_ctx *ctx, const float *src_polar, const float *tgt_polar, int32_t rows, int32_t cols,
                                     int32_t clip_px, int32_t downsample, double *angle_rad, double *scale, double *response)
{
    if (!ctx) return ROAM_E_ARG;
    ARG_CHECK(ctx, src_polar && tgt_polar && angle_rad);
    int clip, R;
    FFT_TRY(fmt_clip_radius(ctx, rows, cols, clip_px, downsample, &clip, &R));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    FmtBatchIn in;
    in.host_src = src_polar; in.host_tgt = tgt_polar; in.row_stride = cols; in.image_stride = (int64_t)rows * cols;
    in.cols = cols;
    double out3[3];
    FFT_TRY(roam_fmt_batch_run(ctx, in, 1, rows, clip, R, out3, nullptr));
    *angle_rad = out3[0];
    if (scale) *scale = out3[1];
    if (response) *response = out3[2];
    return ROAM_OK;
}

// Rotation, then translation, for n pairs (FMT.py:211-250, then rotateImg(prevImgCart, rotDeg) and a phase correlation of the turned
// source with the target).  Per chunk of nb pairs: fmt_rot_chunk gives the angles and brings them to the host (first synchronisation);
// the host makes the nb inverse rotation matrices with its libm, as roam_warp_affine_f32 does; the kernels of fmt_register.hip make
// the 2 nb Cartesian images and fill the planes, laid out as in roam_fmt_batch_run; the correlation and the peak search are the same
// (second synchronisation).  Host images go up once, whole, and both halves read them on the device.
int32_t roam_fmt_register_run(roam_ctx *ctx, const FmtBatchIn &in, int n, int rows, int clip, int R, int Rc, double *out6, float *cart_out)
{
    const int S = 2 * Rc;
    ARG_CHECK(ctx, S >= 2 && S <= FFT_MAX_N);
    const FmtRotSize g = fmt_rot_size(R);
    ARG_CHECK(ctx, g.M <= FFT_MAX_N && g.N <= FFT_MAX_N);
    const int M = optimal_dft_size(S);
    const bool host = in.host_src != nullptr;
    const size_t ncart = (size_t)S * S, nin = host ? (size_t)rows * in.cols : 0;
    // the rotation half reads the images this half uploads: it counts as on resident records
    const size_t per_pair = fmt_rot_bytes_per_pair(rows, R, 0, false) + fmt_trans_bytes_per_pair(Rc, nin, cart_out != nullptr);
    const size_t chunk = pc_chunk(per_pair, n, 32767, true);                 // 2 chunk images in grid.z
    hipStream_t st = ctx->stream;
    FmtWork w;
    FmtTables tables;
    FFT_TRY(fmt_scratch_slab(ctx, {rows, R, Rc, chunk, 0, nin, false, cart_out != nullptr}, &w));
    HIP_TRY(ctx, fmt_tables_upload(st, g, R, Rc, w, &tables));
    std::vector<double> o3(3 * chunk), o(3 * chunk), Mh(6 * chunk);
    for (size_t b0 = 0; b0 < (size_t)n; b0 += chunk) {
        const int nb = (int)(((size_t)n - b0) < chunk ? ((size_t)n - b0) : chunk);
        FmtBatchSrc src = {w.in, (int64_t)nin, (int64_t)in.cols, 0, 0, nullptr};
        if (host) {
            const float *h[2] = {in.host_src, in.host_tgt};
            for (int k = 0; k < 2; k++)
                HIP_TRY(ctx, roam_upload_packed_f32(st, w.in + (size_t)k * nb * nin, h[k] + (int64_t)b0 * in.image_stride, nb, in.cols, rows,
                                                    in.row_stride, in.image_stride));
        } else {
            FFT_TRY(fmt_pool_src(ctx, st, in, b0, nb, w.idx, &src));
        }
        FFT_TRY(fmt_rot_chunk(ctx, st, src, nb, rows, clip, R, g, w, nullptr, 0, o3.data()));       // synchronises: the angles are here
        const double c = (double)(float)Rc;                  // getRotationMatrix2D's centre (w / 2, h / 2) as a cv::Point2f
        for (int i = 0; i < nb; i++) roam_rotation_inverse_map(c, c, o3[3 * i] * (180.0 / M_PI), &Mh[6 * (size_t)i]);
        HIP_TRY(ctx, hipMemcpyAsync(w.M, Mh.data(), sizeof(double) * 6 * nb, hipMemcpyHostToDevice, st));
        FFT_TRY(fmt_trans_enqueue(ctx, st, src, nb, rows, in.cols, Rc, M, w));
        HIP_TRY(ctx, hipMemcpyAsync(o.data(), w.pc.out, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost, st));
        if (cart_out) {
            HIP_TRY(ctx, hipMemcpyAsync(cart_out + b0 * ncart, w.rot, sizeof(float) * ncart * nb, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(cart_out + ((size_t)n + b0) * ncart, w.cart_t + (size_t)nb * ncart, sizeof(float) * ncart * nb,
                                        hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (int i = 0; i < nb; i++) {
            double *q = out6 + 6 * (b0 + i);
            q[0] = o3[3 * i]; q[1] = o3[3 * i + 1]; q[2] = o3[3 * i + 2];
            q[3] = o[3 * i]; q[4] = o[3 * i + 1]; q[5] = o[3 * i + 2];
        }
    }
    return ROAM_OK;
}

extern "C" int32_t roam_fmt_register_batch_f32(roam_ctx *ctx, const float *src, const float *tgt, int32_t n, int32_t rows, int32_t cols,
                                               int64_t row_stride, int64_t image_stride, int32_t clip_px, int32_t downsample,
                                               int32_t cart_downsample, double *out6, float *cart_out)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, src && tgt && out6 && n >= 1);
    int clip, R;
    FFT_TRY(fmt_clip_radius(ctx, rows, cols, clip_px, downsample, &clip, &R));
    ARG_CHECK(ctx, cols <= 16384 && cart_downsample >= 1);
    ARG_CHECK(ctx, row_stride >= cols && (n == 1 || image_stride >= (int64_t)(rows - 1) * row_stride + cols));
    const int Rc = cols / cart_downsample;
    ARG_CHECK(ctx, 2 * Rc >= 2 && 2 * Rc <= FFT_MAX_N);
    FmtBatchIn in;
    in.host_src = src; in.host_tgt = tgt; in.row_stride = row_stride; in.image_stride = n == 1 ? (int64_t)rows * row_stride : image_stride;
    in.cols = cols;
    return roam_fmt_register_run(ctx, in, n, rows, clip, R, Rc, out6, cart_out);
}

// ------------------------------------------------------------------------------------------------ in-step registration
// The registration as a part of roam_engine_step (roam_engine_set_auto_prior): the two cores above with fmtr_angle_matrix_kernel between
// them and fmtr_prior_kernel behind them, on a stream the engine gives, in the slab the engine allocated.  Nothing here synchronises
// or allocates once roam_fmt_auto_init has returned.
struct FmtAuto {
    FmtAutoCfg cfg;
    FmtAutoPlan plan;
    FmtRotSize g;
    int Mt;                             // DFT side of the translation half
    int32_t *h_idx = nullptr;           // pinned: 4 slots of 3 lanes ints (the chunks' index lists, then pair_of); w.idx: the same ring
    FmtWork w;
};

static FmtPass fmt_auto_pass(const FmtAutoCfg &c, size_t chunk) { return {c.rows, c.R, c.Rc, chunk, (size_t)c.lanes, 0, false, false}; }

int32_t roam_fmt_auto_plan(roam_ctx *ctx, const FmtAutoCfg &c, FmtAutoPlan *plan)
{
    // what roam_engine_fmt_register refuses
    ARG_CHECK(ctx, c.lanes >= 1 && c.rows >= 8 && c.rows <= 16384 && c.cols >= 2 && c.cols <= 16384 && c.clip >= 1 && c.clip <= c.cols);
    ARG_CHECK(ctx, c.R >= ROAM_FMT_MIN_R && c.R <= ROAM_FMT_MAX_R && c.Rc >= 1 && 2 * c.Rc <= FFT_MAX_N);
    ARG_CHECK(ctx, c.min_rot >= 0.0 && c.min_rot <= 1e300 && c.min_trans >= 0.0 && c.min_trans <= 1e300);       // (NaN fails them too)
    const FmtRotSize g = fmt_rot_size(c.R);
    ARG_CHECK(ctx, g.M <= FFT_MAX_N && g.N <= FFT_MAX_N);
    // as roam_fmt_register_run counts a pair on resident records
    plan->per_pair = fmt_rot_bytes_per_pair(c.rows, c.R, 0, false) + fmt_trans_bytes_per_pair(c.Rc, 0, false);
    plan->chunk = pc_chunk(plan->per_pair, (size_t)c.lanes, 32767, true);
    plan->slab_bytes = fmt_carve(fmt_auto_pass(c, plan->chunk), nullptr, nullptr);
    plan->sz = g.sz;
    plan->log_base = fmt_log_base(g);
    return ROAM_OK;
}

double roam_fmt_scale(double log_base, double shift_x) { return fmt_scale(log_base, shift_x); }

void roam_fmt_auto_free(FmtAuto *a)
{
    if (!a) return;
    if (a->h_idx) (void)hipHostFree(a->h_idx);
    delete a;
}

int32_t roam_fmt_auto_init(roam_ctx *ctx, const FmtAutoCfg &c, const FmtAutoPlan &plan, uint8_t *slab, FmtAuto **out)
{
    FmtAuto *a = new (std::nothrow) FmtAuto();
    if (!a) { ROAM_SET_ERR(ctx, "auto prior: out of host memory"); return ROAM_E_HIP; }
    a->cfg = c; a->plan = plan;
    a->g = fmt_rot_size(c.R); a->Mt = optimal_dft_size(2 * c.Rc);
    fmt_carve(fmt_auto_pass(c, plan.chunk), slab, &a->w);
    FmtTables tables;
    hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&a->h_idx), sizeof(int32_t) * 4 * 3 * (size_t)c.lanes, hipHostMallocDefault);
    if (e == hipSuccess) e = fmt_tables_upload(ctx->stream, a->g, c.R, c.Rc, a->w, &tables);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ROAM_SET_ERR(ctx, "auto prior: staging or table upload failed: %s", hipGetErrorString(e));
        roam_fmt_auto_free(a);
        return ROAM_E_HIP;
    }
    for (int n : {a->g.M, a->g.N, a->Mt})                  // now, not at the first step
        if (!fft_twiddles(ctx, n)) { roam_fmt_auto_free(a); return ROAM_E_HIP; }
    *out = a;
    return ROAM_OK;
}

int32_t roam_fmt_auto_enqueue(roam_ctx *ctx, FmtAuto *a, hipStream_t st, const FmtBatchIn &pool, int slot4, int npairs, const int32_t *prev,
                              const int32_t *curr, const int32_t *pair_of, uint8_t *prior_slot, FmtPriorRec *rec_slot)
{
    const FmtAutoCfg &c = a->cfg;
    const size_t L = (size_t)c.lanes, chunk = a->plan.chunk;
    int32_t *h = a->h_idx + (size_t)slot4 * 3 * L, *d = a->w.idx + (size_t)slot4 * 3 * L;
    for (size_t p0 = 0; p0 < (size_t)npairs; p0 += chunk) {          // chunk by chunk: the sources' records, then the targets'
        const size_t nb = std::min(chunk, (size_t)npairs - p0);
        memcpy(h + 2 * p0, prev + p0, sizeof(int32_t) * nb);
        memcpy(h + 2 * p0 + nb, curr + p0, sizeof(int32_t) * nb);
    }
    memcpy(h + 2 * L, pair_of, sizeof(int32_t) * L);
    HIP_TRY(ctx, hipMemcpyAsync(d, h, sizeof(int32_t) * 3 * L, hipMemcpyHostToDevice, st));
    const double cc = (double)(float)c.Rc;                   // getRotationMatrix2D's centre (w / 2, h / 2) as a cv::Point2f
    for (size_t p0 = 0; p0 < (size_t)npairs; p0 += chunk) {
        const int nb = (int)std::min(chunk, (size_t)npairs - p0);
        const FmtBatchSrc src = {pool.pool, pool.rec_bytes, pool.rec_stride, pool.payload_off, 1, d + 2 * p0};
        FmtWork w = a->w;                                    // the chunk's rows of the per-lane arrays
        w.pc.out += 3 * p0; w.ang += p0; w.M += 6 * p0;
        FFT_TRY(fmt_rot_enqueue(ctx, st, src, nb, c.rows, c.clip, c.R, a->g, w));
        HIP_TRY(ctx, launch_fmtr_angle_matrix(st, w.pc.out, nb, a->plan.sz, cc, w.ang, w.M));
        w.pc.out = a->w.trans3 + 3 * p0;
        FFT_TRY(fmt_trans_enqueue(ctx, st, src, nb, c.rows, c.cols, c.Rc, a->Mt, w));
    }
    // the tracker's grid against the registration's: FMT.flowPriorFromFMT's s = (cols // 2) / (cols // cart_downsample)
    FmtPriorArgs pa = {d + 2 * L, a->w.pc.out, a->w.ang, a->w.trans3, c.lanes, cc, (double)(c.cols / 2) / (double)c.Rc, c.min_rot, c.min_trans,
                       prior_slot, rec_slot};
    HIP_TRY(ctx, launch_fmtr_prior(st, pa));
    return ROAM_OK;
}
