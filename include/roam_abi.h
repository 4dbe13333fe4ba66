/* roam_abi.h — C ABI of libroam_hip.so, the MI355X-native (gfx950, hand-written HIP)
 * replacement for the per-scan hot path of Samleo8/RadarSLAMPy ("RAW-ROAM").
 *
 * The reference has no FFI: its "plugin API" is a set of Python call signatures.  Each
 * entry point below states the reference callable it replaces (file:line, relative to the
 * reference repo).  radarslampy_amd/_ffi.py binds exactly these symbols with ctypes;
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Every function returns int32 status:
 *     ROAM_OK (0) or a negative ROAM_E_* code; roam_last_error(ctx) has the text.
 *   - The caller owns every host buffer.  Outputs go into caller-allocated, capacity-
 *     checked arrays.  Device memory is owned by the context.
 *   - Arrays are row-major contiguous.  Coordinates are [x, y] float32 pixels; poses are
 *     [x, y, theta] float64; 3x3 transforms are row-major float64[9].
 *   - One context = one GPU + one HIP stream; a context is single-threaded, distinct
 *     contexts are independent.  No global mutable state.
 *   - "stage" entry points take host arrays (H2D, kernel(s), D2H) and mirror one reference
 *     function each.  "engine" entry points keep B independent sequences ("lanes")
 *     resident in HBM and advance all of them by one scan pair per call without touching
 *     the host (the throughput path measured by bench.py).
 */
#ifndef ROAM_ABI_H
#define ROAM_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct roam_ctx roam_ctx;

enum {
    ROAM_OK = 0,
    ROAM_E_ARG = -1,        /* bad argument (null pointer, size out of range)       */
    ROAM_E_HIP = -2,        /* a HIP runtime call failed                              */
    ROAM_E_CAPACITY = -3,   /* caller-provided output capacity too small             */
    ROAM_E_NODEVICE = -4,   /* no usable gfx950 device                                */
    ROAM_E_STATE = -5       /* engine call in the wrong state                         */
};

/* limits of this build */
#define ROAM_MAX_FEATURES 1024      /* K_max per lane (KLT / graph / LM)                */
#define ROAM_MAX_COLS 4096          /* longest polar row the peak kernel accepts        */
#define ROAM_PYR_LEVELS 4           /* LK maxLevel=3 (getTransformKLT.py:77-81)         */

/* ---- context ------------------------------------------------------------------------ */
int32_t roam_create(int32_t device_id, roam_ctx **out);
int32_t roam_destroy(roam_ctx *ctx);
const char *roam_last_error(const roam_ctx *ctx);
const char *roam_version(void);
/* name_cap bytes for the device name; any out pointer may be NULL */
int32_t roam_device_info(roam_ctx *ctx, char *name, int32_t name_cap, int32_t *cu_count,
                         int64_t *hbm_bytes, char *arch, int32_t arch_cap);
int32_t roam_synchronize(roam_ctx *ctx);
/* pinned (page-locked) host memory for asynchronous record uploads */
int32_t roam_host_alloc(roam_ctx *ctx, int64_t bytes, void **out);
int32_t roam_host_free(roam_ctx *ctx, void *p);

/* ---- f2: record ingest from PNG files (parseData.py:160-226: cv2.imread(path, IMREAD_GRAYSCALE) at :178; the reference decodes
 * frame k inside its loop, RawROAMSystem.py:162-165).  Host code only - no device, no context.  The one format of the data set:
 * 8-bit greyscale, non-interlaced; anything else (and a corrupt file) is ROAM_E_ARG.  The image is written row by row into out
 * (out_stride bytes between rows, 0 = the image width; ROAM_E_CAPACITY when (rows - 1) * out_stride + cols > out_bytes) - typically
 * a slot of a roam_host_alloc ring, so that a decoded record is uploaded from where it was decoded.  rows / cols may be NULL. */
int32_t roam_png_decode_gray8(const uint8_t *png, int64_t png_bytes, uint8_t *out, int64_t out_bytes, int64_t out_stride,
                              int32_t *rows, int32_t *cols);
int32_t roam_png_decode_file(const char *path, uint8_t *out, int64_t out_bytes, int64_t out_stride, int32_t *rows, int32_t *cols);
/* a pool of host threads decoding files ahead of the consumer.  submit() queues one file for one destination and returns at once; the
 * caller names the job with a ticket of its choice (unique among the jobs in flight) and wait(ticket) blocks until THAT job is done and
 * returns its status (tickets complete in any order; every submitted ticket must be waited for before its destination is reused).
 * destroy() drops the jobs that have not started and joins the threads. */
typedef struct roam_png_pool roam_png_pool;
int32_t roam_png_pool_create(int32_t workers, roam_png_pool **out);
int32_t roam_png_pool_submit(roam_png_pool *pool, const char *path, uint8_t *dst, int64_t dst_bytes, int64_t dst_stride, int64_t ticket);
int32_t roam_png_pool_wait(roam_png_pool *pool, int64_t ticket, int32_t *rows, int32_t *cols);
int32_t roam_png_pool_destroy(roam_png_pool *pool);

/* ---- a2: getPointCloud.getPointCloudPolarInd (getPointCloud.py:11-54) ------------------
 * polar: rows x cols float32.  out: (cap,2) int32 rows [azimuthIdx, rangeIdx], azimuth-
 * major, range ascending.  *n_out = number of peaks found; if it exceeds cap the call
 * returns ROAM_E_CAPACITY (the first cap pairs are valid). */
int32_t roam_peaks_polar_f32(roam_ctx *ctx, const float *polar, int32_t rows, int32_t cols,
                             int32_t *out, int64_t cap, int64_t *n_out);
/* a1+a2 fused: raw Oxford record rows (parseData.extractDataFromRadarImage, parseData.py:17-53):
 * value = rec[r*stride + payload_off + i] / 255 (float32), i < clip. */
int32_t roam_peaks_record_u8(roam_ctx *ctx, const uint8_t *rec, int32_t rows, int64_t stride,
                             int32_t payload_off, int32_t clip, int32_t *out, int64_t cap,
                             int64_t *n_out);
/* the same two with scipy.signal.find_peaks' distance / prominence conditions - getPointCloudPolarInd(polarImage, peakDistance,
 * peakProminence) (getPointCloud.py:11-54, the find_peaks call at :33-35).  Per row, in find_peaks' order: local maxima; distance:
 * d = ceil(distance), priority = np.argsort of the heights as NumPy 1.22.3 (the reference's pin) orders them, walked from the highest
 * priority down, a kept peak suppresses every peak closer than d; prominence (wlen=None) of the survivors in float64, kept if
 * prom_min <= prominence <= prom_max; then the reference's mean + std threshold.  distance == 0: no distance condition (any other
 * value below 1 is ROAM_E_ARG; NaN suppresses nothing, as in find_peaks); a NaN bound is no bound, two NaN bounds no prominence condition; with no condition at all
 * the call is roam_peaks_polar_f32 / roam_peaks_record_u8.  out, *n_out and the capacity rule as there. */
int32_t roam_peaks_polar_f32_cond(roam_ctx *ctx, const float *polar, int32_t rows, int32_t cols,
                                  double distance, double prom_min, double prom_max,
                                  int32_t *out, int64_t cap, int64_t *n_out);
int32_t roam_peaks_record_u8_cond(roam_ctx *ctx, const uint8_t *rec, int32_t rows, int64_t stride,
                                  int32_t payload_off, int32_t clip, double distance, double prom_min,
                                  double prom_max, int32_t *out, int64_t cap, int64_t *n_out);

/* ---- a3: parseData.convertPolarImageToCartesian (parseData.py:100-135) -------------------
 * polar rows x cols f32 -> (2R x 2R), R = cols/2.  cart_f32 and/or cart_u8 may be NULL;
 * cart_u8 is the (img*255).astype(uint8) of getTransformKLT.py:356-357. */
int32_t roam_polar_to_cart_f32(roam_ctx *ctx, const float *polar, int32_t rows, int32_t cols,
                               float *cart_f32, uint8_t *cart_u8);
int32_t roam_polar_to_cart_record_u8(roam_ctx *ctx, const uint8_t *rec, int32_t rows, int64_t stride,
                                     int32_t payload_off, int32_t clip, float *cart_f32,
                                     uint8_t *cart_u8);

/* ---- cv2.warpPolar(src, (dw, dh), (cx, cy), max_radius, INTER_LINEAR | WARP_FILL_OUTLIERS | flags) on float32 images
 * (parseData.py:69-157: convertCartesianImageToPolar, convertPolarImageToCartesian, convertPolarImgToLogPolar).
 * flags: ROAM_WARP_POLAR_LOG (semilog) and / or ROAM_WARP_POLAR_INVERSE (polar rows x cols -> Cartesian dh x dw; without it
 * Cartesian rows x cols -> dh rows of angle x dw columns of radius).  n images of one geometry: image i starts src_image_stride
 * floats after image i - 1, its rows src_row_stride floats apart; dst is n x dh x dw, contiguous.  dsize arrives resolved
 * (OpenCV's defaults for a zero size are the caller's).  ROAM_E_ARG: a size <= 0 or > 16384, max_radius <= 0 (<= 1 with
 * ROAM_WARP_POLAR_LOG) or not finite, a centre that is not finite, unknown flags. */
#define ROAM_WARP_POLAR_LOG     1
#define ROAM_WARP_POLAR_INVERSE 2
int32_t roam_warp_polar_f32(roam_ctx *ctx, const float *src, int32_t n, int32_t rows, int32_t cols, int64_t src_row_stride,
                            int64_t src_image_stride, float *dst, int32_t dw, int32_t dh, float cx, float cy,
                            double max_radius, int32_t flags);

/* cv2.warpAffine(src, M, (dw, dh), INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT 0) on float32 images
 * (FMT.rotateImg, FMT.py:93-100).  n images of one shape; M: m_count x 6 doubles (row-major 2 x 3),
 * m_count == 1 (one matrix for all images) or m_count == n (one per image).  Image i starts src_image_stride floats after
 * image i - 1, its rows src_row_stride floats apart; dst is n x dh x dw, contiguous.  Without ROAM_WARP_AFFINE_INVERSE_MAP M maps
 * source to destination and is inverted on the host as OpenCV inverts it (a singular M becomes all zeros: every output pixel is
 * src[0, 0]); with it M maps destination to source.  OpenCV's fixed-point coordinates: 1/1024 px per term, summed in int32, 1/32 px
 * for the bilinear weights, tap indices saturated to int16 - exact while the source coordinates stay below 2^20 px (the caller's
 * check; _ffi.warp_affine_args).  ROAM_E_ARG: a null pointer, n < 1, a side < 1 or > 16384, m_count not in {1, n}, unknown flags,
 * src_row_stride < cols, src_image_stride smaller than one image's extent (n > 1). */
#define ROAM_WARP_AFFINE_INVERSE_MAP 1
int32_t roam_warp_affine_f32(roam_ctx *ctx, const float *src, int32_t n, int32_t rows, int32_t cols,
                             int64_t src_row_stride, int64_t src_image_stride, const double *M, int32_t m_count,
                             float *dst, int32_t dw, int32_t dh, int32_t flags);
/* measurement aid: average milliseconds (HIP events, two warm runs first) of the warp_affine_kernel launch that warps n resident
 * rows x cols images (zeros) by the forward matrix M (6 doubles) into n images of the same size; no host transfer is timed */
int32_t roam_time_warp_affine(roam_ctx *ctx, int32_t n, int32_t rows, int32_t cols, const double *M, int32_t reps,
                              float *ms_per_rep);

/* ---- a7: cv2.calcOpticalFlowPyrLK as used by getTransformKLT.getTrackedPointsKLT
 * (getTransformKLT.py:317-381; LK_PARAMS :77-81: winSize 15, maxLevel 3, 10 iter, eps 0.03).
 * Images are w x h; *_f32 variants quantise (img*255 -> u8, :356-357) on the device.
 * pts (K,2) f32 -> next_pts (K,2) f32, status (K) u8, err (K) f32.  The reference's
 * `status &= err < ERR_THRESHOLD` (:365) is applied by the caller. */
int32_t roam_klt_track_u8(roam_ctx *ctx, const uint8_t *prev_img, const uint8_t *next_img,
                          int32_t w, int32_t h, const float *pts, int32_t K,
                          float *next_pts, uint8_t *status, float *err);
int32_t roam_klt_track_f32(roam_ctx *ctx, const float *prev_img, const float *next_img,
                           int32_t w, int32_t h, const float *pts, int32_t K,
                           float *next_pts, uint8_t *status, float *err);
/* The same with cv2's OPTFLOW_USE_INITIAL_FLOW: init_pts (K,2) f32 is where the search for each feature STARTS in next_img (a motion
 * prior).  OpenCV's rule: only the top pyramid level differs - there the start is init_pts * 2^-maxLevel instead of pts * 2^-maxLevel;
 * the window and its derivatives are taken at pts as before, lower levels start at twice the level above, status and err follow
 * the same rules.  init_pts == NULL is roam_klt_track_u8 / _f32, bit for bit; init_pts == pts gives those bits as well.
 * ROAM_E_ARG before any device work: a guess coordinate that is not finite or whose magnitude exceeds ROAM_KLT_MAX_GUESS px
 * (2^20, the bound of roam_warp_affine_f32's coordinates: the tracker's float -> int conversions of the window origin stay
 * defined far beyond any image the pyramid accepts). */
#define ROAM_KLT_MAX_GUESS 1048576.0f
int32_t roam_klt_track_u8_flow(roam_ctx *ctx, const uint8_t *prev_img, const uint8_t *next_img,
                               int32_t w, int32_t h, const float *pts, const float *init_pts, int32_t K,
                               float *next_pts, uint8_t *status, float *err);
int32_t roam_klt_track_f32_flow(roam_ctx *ctx, const float *prev_img, const float *next_img,
                                int32_t w, int32_t h, const float *pts, const float *init_pts, int32_t K,
                                float *next_pts, uint8_t *status, float *err);
/* pyrDown (5x5 Gaussian, REFLECT_101): src w x h -> dst ((w+1)/2 x (h+1)/2) */
int32_t roam_pyr_down_u8(roam_ctx *ctx, const uint8_t *src, int32_t w, int32_t h, uint8_t *dst);

/* ---- a8: outlierRejection.rejectOutliers (outlierRejection.py:16-95) --------------------
 * prev/next (K,2) f32.  mask_out (K) u8 = membership of the maximum clique of the
 * |d_prev - d_next| <= thr_px consistency graph; when several maximum cliques exist, the one
 * the reference returns: the first strictly-largest clique in networkx.find_cliques order
 * (outlierRejection.py:63-75; CPython set order restated on the device, csrc/clique.hip).
 * node_limit bounds the search nodes counted over the whole call (0 = default, 300 000): first the search for the
 * clique number and one maximum clique (the witness), then the existence queries that single out the reference's
 * clique.  *flags_out bit0 = search completed: the mask is proven maximum and equal to the reference's.  Bit0 clear,
 * the budget ran out: inside the first search the mask is the largest clique completed so far - EMPTY (n_inliers 0)
 * when no descent had reached a leaf yet; after it the mask is the witness, a maximum clique that need not be the
 * reference's.  The mask is a clique of the graph and *n_inliers its count in every case
 * (tests/clique_budget_model.py).  adj_out (optional) receives the K x ((K+63)/64) uint64 adjacency bit rows. */
int32_t roam_reject_outliers(roam_ctx *ctx, const float *prev, const float *next, int32_t K,
                             double thr_px, int64_t node_limit, uint8_t *mask_out,
                             int32_t *n_inliers, int32_t *flags_out, uint64_t *adj_out);

/* measurement aid: the same correspondence set replicated `copies` times (one problem each, as in an engine step);
 * average ms per launch of the consistency-graph and the maximum-clique kernel over `reps` launches */
int32_t roam_time_reject_outliers(roam_ctx *ctx, const float *prev, const float *next, int32_t K, int32_t copies,
                                  double thr_px, int64_t node_limit, int32_t reps, float *graph_ms, float *clique_ms,
                                  int32_t *n_inliers, int32_t *proven);

/* ---- a10: getTransformKLT.calculateTransformSVD (getTransformKLT.py:129-162) -------------
 * src ~= R tgt + h over N pairs of float64 [x,y]; R row-major [4], h [2]. */
int32_t roam_kabsch2d(roam_ctx *ctx, const double *src, const double *tgt, int32_t N,
                      double *R, double *h);

/* ---- a11-a14: motionDistortion.MotionDistortionSolver (motionDistortion.py:70-205,295-325)
 * update_problem + optimize_library in one call.  sigma5 = [sp_x, sp_y, sv_x, sv_y, sv_th]
 * (covariance diagonals; residual weights are 1/sigma as in :96-99).  out6 = [v(3), pose(3)].
 * x0_out (6) and r0_out (2N+3) are optional: start vector and error_vector(x0). */
int32_t roam_mds_solve(roam_ctx *ctx, const double *T_wj0, const double *p_w, const double *p_jt,
                       int32_t N, const double *T_wj_init, const double *sigma5, double period,
                       double *out6, int32_t *nfev, int32_t *info, double *x0_out, double *r0_out);
/* MotionDistortionSolver.undistort (:126-153) / compute_time_deltas (:107-124): pts (N,2) f64 */
int32_t roam_mds_undistort(roam_ctx *ctx, const double *v3, const double *pts, int32_t N,
                           double period, double *out_xy, double *dT_out);

/* ---- a5: ANMS.ssc (ANMS.py:5-102) ----------------------------------------------------------
 * kp (B,3) f64 rows [row, col, sigma] in priority order; sel_out (cap >= B) receives the
 * selected indices in input order. */
int32_t roam_ssc(roam_ctx *ctx, const double *kp, int32_t B, int32_t num_ret, double tol,
                 int32_t cols, int32_t rows, int32_t *sel_out, int32_t *n_sel);

/* ---- a4: getFeatures.getBlobsFromCart (skimage blob_doh, getFeatures.py:22-53) ------------
 * image-scale part of blob_doh: float64 integral image, box-filter Hessian determinant for
 * every sigma, 3x3x3 local maxima above `threshold`.  img w x h f32.  out_rcs (cap,3) int32 rows
 * [row, col, sigma_index] in C (row, col, sigma) order, out_val (cap) the determinant values.
 * Ordering by response and overlap pruning (_prune_blobs) are host bookkeeping. */
int32_t roam_doh_maxima(roam_ctx *ctx, const float *img, int32_t w, int32_t h, const double *sigmas,
                        int32_t num_sigma, double threshold, int32_t *out_rcs, double *out_val,
                        int32_t cap, int32_t *n_out);

/* ---- getFeatures.getBlobsFromCart(method="log") (skimage blob_log, getFeatures.py:22-53) -------------------------------
 * image-scale part of blob_log: per sigma s, the float64 layer -gaussian_laplace(img, s) * scale[s] (scipy.ndimage: separable
 * correlations, mode 'reflect', symmetric-kernel arithmetic), then the 3x3x3 maxima of the (row, col, sigma) cube above
 * `threshold` (peak_local_max: outside the cube counts as 0; no peaks in a trivial cube).  img w x h, f32 (img_bytes_per_px 4,
 * widened exactly) or f64 (8).  radius[s] in [0, 800]; kernels = for each s the order-0 then the order-2 weights of
 * scipy's gaussian_filter1d (2 radius[s] + 1 each, symmetric; the caller computes them); scale[s] = sigma^2.
 * out_rcs (cap,3) int32 [row, col, sigma_index] in C order, out_val (cap) the layer values; beyond cap ROAM_E_CAPACITY with the
 * true count in n_out.  out_layers (optional, may be NULL): num_sigma x h x w f64, the layers. */
int32_t roam_log_maxima(roam_ctx *ctx, const void *img, int32_t img_bytes_per_px, int32_t w, int32_t h, int32_t num_sigma,
                        const int32_t *radius, const double *kernels, const double *scale, double threshold, int32_t *out_rcs,
                        double *out_val, int32_t cap, int32_t *n_out, double *out_layers);

/* ---- a4/a5 bookkeeping whose ORDER the reference's pinned third-party stack fixes (host code, no GPU; the engine's
 * device-side retrack runs the same functions on the GPU):
 * roam_prune_blobs   = skimage.feature.blob._prune_blobs as blob_doh / blob_log call it (getFeatures.py:47-51): candidate pairs in
 *                      the iteration order of the Python set that scipy cKDTree.query_pairs fills.  blobs (n,3) f64 rows
 *                      [row, col, sigma] in peak_local_max order, integer rows / cols in [0, 32767]; keep_out (n) u8.  Any
 *                      number of points and pairs (beyond 32767 of either: a 32-bit host instantiation of the same code).
 * roam_argsort_np122 = np.argsort of the pinned NumPy 1.22.3 (unstable introsort) that adaptiveNMS applies to the
 *                      two-valued sigmas (getFeatures.py:69); order_out (n) i32. */
int32_t roam_prune_blobs(const double *blobs, int32_t n, double overlap, uint8_t *keep_out);
/* test: the candidate pairs behind roam_prune_blobs (its 16-bit form: n <= 32767 blobs, at most 32767 pairs), i << 16 | j with i < j, in
 * the order scipy's cKDTree.query_pairs emits them.  ROAM_E_CAPACITY: more pairs than that, or than cap. */
int32_t roam_debug_prune_pairs(const double *blobs, int32_t n, uint32_t *pairs_out, int32_t cap, int32_t *n_pairs);
int32_t roam_argsort_np122(const double *keys, int32_t n, int32_t *order_out);

/* ---- f4: FMT.getRotationUsingFMT (FMT.py:36-90; called first by Tracker.track, Tracker.py:62-63) ---------------------
 * Fourier-Mellin rotation prior between two contiguous polar images (rows x cols float32): range clip (clip_px bins, <= 0 or >= cols:
 * none), cv2.resize to R = clip / downsample columns, polar -> Cartesian -> log-polar, Hanning-windowed phase correlation.
 * angle_rad: R(angle) src = target; scale and response are optional.  This is n = 1 of roam_fmt_rotation_batch_f32 below
 * (row_stride = cols), the same pass and the same numbers bit for bit.  ROAM_E_ARG, before any device call: a null src_polar /
 * tgt_polar / angle_rad, rows outside [8, 16384], cols < 2, downsample < 1, R outside [ROAM_FMT_MIN_R, ROAM_FMT_MAX_R] = [4, 1303].
 * (The separate direct-DFT implementation this entry had before took any rows >= 8 and R up to 2048.) */
int32_t roam_fmt_rotation(roam_ctx *ctx, const float *src_polar, const float *tgt_polar, int32_t rows, int32_t cols,
                          int32_t clip_px, int32_t downsample, double *angle_rad, double *scale, double *response);

/* FMT.getTranslationUsingPhaseCorrelation (FMT.py:13-33): cv2.phaseCorrelate(src, tgt, createHanningWindow((cols, rows), CV_32F))
 * for `batch` pairs of rows x cols float32 images (row_stride / image_stride in elements).  hanning = 0: no window
 * (cv2.phaseCorrelate(src, tgt)).  out_dxdy (batch, 2) f64 [dx, dy], out_response (batch) f64 (may be NULL).
 * The images are zero-padded to the optimal DFT size (2^a 3^b 5^c) and transformed by the mixed-radix FFT of csrc/fft.hip (the
 * correlation on top of it: csrc/phasecorr.hip); a large batch is processed in chunks that keep the device scratch under 2 GB.  ROAM_E_ARG: rows or cols outside [2, 4096], batch < 1,
 * a null src / tgt / out_dxdy, row_stride < cols, image_stride smaller than one image's extent (batch > 1). */
int32_t roam_phase_correlate_f32(roam_ctx *ctx, const float *src, const float *tgt, int32_t batch, int32_t rows, int32_t cols,
                                 int64_t row_stride, int64_t image_stride, int32_t hanning, double *out_dxdy, double *out_response);

/* FMT.getRotationUsingFMT for n pairs in one device pass, the one implementation of the estimate: the front end batched over the
 * 2 n images (csrc/fmt_batch.hip) and the correlation through the mixed-radix FFT of roam_phase_correlate_f32, so the plane may be as
 * large as 4096 x 1350 (downsample 1 or 2).  src / tgt: n float32 polar images each, rows x cols, row_stride / image_stride in
 * elements.  R = clip / downsample columns after the resize, clip = clip_px (<= 0 or >= cols: cols).  out3 (n, 3) f64
 * {angle_rad, scale, response}.  logpolar_out: NULL, or (2 n, round(pi R), R) f32: the log-polar images before the window, all sources
 * first, then all targets (for tests).  A large batch is processed in chunks that keep the device scratch under 2 GB, with one stream
 * synchronisation per chunk; the result of a pair does not depend on the batch it is in.  ROAM_E_ARG: a null src / tgt / out3, n < 1,
 * rows outside [8, 16384], cols < 2, downsample < 1, R outside [ROAM_FMT_MIN_R, ROAM_FMT_MAX_R] (round(pi R) must fit the FFT's 4096),
 * row_stride < cols, image_stride smaller than one image's extent (n > 1). */
#define ROAM_FMT_MIN_R 4
#define ROAM_FMT_MAX_R 1303
int32_t roam_fmt_rotation_batch_f32(roam_ctx *ctx, const float *src, const float *tgt, int32_t n, int32_t rows, int32_t cols,
                                    int64_t row_stride, int64_t image_stride, int32_t clip_px, int32_t downsample, double *out3,
                                    float *logpolar_out);

/* Fourier-Mellin registration of n pairs, rotation and then translation, in one device pass (FMT.py:211-250 estimates the rotation;
 * plotCartPolarWithRotation, FMT.py:134-168, applies it as rotateImg(prevImgCart, rotDeg); the method cited at FMT.py:79 ends with a
 * second phase correlation, of the de-rotated Cartesian images).  Per pair: {angle_rad, scale, rot_response} exactly as
 * roam_fmt_rotation_batch_f32 gives them; srcCart, tgtCart = convertPolarImageToCartesian(., downsampleFactor = cart_downsample) of the
 * full-width polar images (FMT.py:191, 213: 2Rc x 2Rc, Rc = cols / cart_downsample; roam_warp_polar_f32's arithmetic);
 * srcRot = rotateImg(srcCart, degrees(angle_rad)) (FMT.py:93-100; roam_warp_affine_f32's arithmetic, the matrix made and inverted on
 * the host in float64); {(dx, dy), trans_response} = cv2.phaseCorrelate(srcRot, tgtCart, Hanning window) (FMT.py:13-33;
 * roam_phase_correlate_f32's arithmetic), dx, dy in pixels of the 2Rc x 2Rc image.  out6 (n, 6) f64
 * {angle_rad, scale, rot_response, dx, dy, trans_response}.  cart_out: NULL, or (2 n, 2Rc, 2Rc) f32: the turned sources, then the target
 * Cartesian images, before the window (for tests).  Chunks as roam_fmt_rotation_batch_f32, two stream synchronisations per chunk
 * (the angles come to the host, whose libm makes the matrices); the result of a pair does not depend on the batch it is in.
 * ROAM_E_ARG: whatever roam_fmt_rotation_batch_f32 refuses, cols > 16384, cart_downsample < 1, 2Rc outside [2, 4096]. */
int32_t roam_fmt_register_batch_f32(roam_ctx *ctx, const float *src, const float *tgt, int32_t n, int32_t rows, int32_t cols,
                                    int64_t row_stride, int64_t image_stride, int32_t clip_px, int32_t downsample,
                                    int32_t cart_downsample, double *out6, float *cart_out);

/* ---- PoseGraphLib.PoseGraphOptimization (PoseGraphLib.py: g2o SparseOptimizer + OptimizationAlgorithmLevenberg; add_vertex, add_edge,
 * optimize, get_pose), in SE(2) like the rest of the project: n_graphs independent pose graphs optimised in one device pass, one
 * workgroup per graph, the whole Levenberg-Marquardt loop inside the kernel (csrc/posegraph.hip).  Graph g owns the vertices
 * vertex_off[g] .. vertex_off[g + 1] (poses [x, y, theta], float64, updated in place; fixed[v] != 0: a constant) and the edges
 * edge_off[g] .. edge_off[g + 1]: (i, j) indices WITHIN the graph in either order, duplicates summed, measurement z = (dx, dy, dtheta),
 * information {xx xy xt yy yt tt} of the symmetric 3 x 3 matrix, and a Huber width (0 = no kernel).  g2o's EdgeSE2:
 *   e = [R(z_th)^T (R(th_i)^T (t_j - t_i) - z_t); normalize(th_j - th_i - z_th)], its analytic Jacobians, the additive update with
 * the angle normalised (VertexSE2::oplus); Huber: s2 = e^T O e <= delta^2: rho = s2, w = 1, else rho = 2 delta sqrt(s2) - delta^2,
 * w = delta / sqrt(s2); H += w J^T O J, b -= w J^T O e, chi2 = sum rho.  The minimiser is g2o's Levenberg-Marquardt:
 * lambda_0 = lambda_init or 1e-5 max diag H, ni = 2; per iteration one linearisation, then trials: solve (H + lambda I) d = b by the
 * block envelope Cholesky (a pivot that is not positive or not finite: the trial's chi2 is +inf), apply d,
 * rho = (chi2 - chi2_trial) / (d^T (lambda d + b) + 1e-3); accepted (rho > 0, chi2_trial finite): lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)),
 * ni = 2; rejected: lambda *= ni, ni *= 2, poses restored; the trials of an iteration end when one is accepted, when rho == 0, after
 * max_trials, or when lambda is not finite, and the optimisation ends after max_iterations or with the first iteration without an
 * accepted trial.  PARITY UNPINNED against g2o (not installed; the contract is tests/pose_graph_model.py, checked against SciPy).
 * No reordering: the free vertices keep their order and block row k is stored from its lowest-numbered free neighbour to the diagonal,
 * so a graph costs its envelope - about the vertex count plus the sum of j - i over its non-consecutive edges, 144 bytes per block.
 * Graphs are processed in chunks that keep the device scratch under 2000 MiB (ROAM_POSE_GRAPH_CHUNK_BYTES in the environment, read per
 * call, lowers where a batch is cut - for tests; the refusal of a single graph stays at 2000 MiB); a graph's result is the same bits alone, anywhere in a
 * batch and in any chunk.  A graph whose vertices are all fixed, or without edges, comes back unchanged with its chi2; a component
 * without a fixed vertex is no error (the damping keeps the system definite).
 * ROAM_E_ARG before any device call, the text naming graph and edge: n_graphs outside [1, 65535]; a graph with no vertex or more than
 * 32768; an edge index out of range or i == j; a pose, measurement, information entry or Huber width that is not finite; a negative
 * Huber width; a graph without a fixed vertex; max_iterations outside [0, 1000], max_trials outside [0, 1000], lambda_init negative
 * or not finite; a single graph whose scratch exceeds a chunk (the text has its index and its envelope). */
typedef struct roam_pose_graph_opts {
    int32_t max_iterations;   /* 0 ... 1000; 0 = evaluate chi2 only, poses untouched */
    int32_t max_trials;       /* 0 = 10 */
    double  lambda_init;      /* 0 = 1e-5 * max diag(H) */
} roam_pose_graph_opts;
typedef struct roam_pose_graph_stats {
    int32_t iterations, trials, rejected, stop;   /* stop: 0 max_iterations, 1 trials exhausted or rho == 0, 2 lambda not finite */
    double chi2_initial, chi2_final, lambda_final;
} roam_pose_graph_stats;
/* host only: envelope blocks per graph and the scratch bytes of the call (its largest chunk).  The structural checks of
 * roam_pose_graph_optimize (sizes, indices, a fixed vertex, the chunk limit): ROAM_E_ARG */
int32_t roam_pose_graph_plan(int32_t n_graphs, const int32_t *vertex_off, const uint8_t *fixed, const int32_t *edge_off,
                             const int32_t *edge_ij, int64_t *envelope_blocks, int64_t *scratch_bytes);
int32_t roam_pose_graph_optimize(roam_ctx *ctx, int32_t n_graphs, const int32_t *vertex_off /* n + 1 */, double *poses /* V x 3, in and out */,
                                 const uint8_t *fixed /* V */, const int32_t *edge_off /* n + 1 */, const int32_t *edge_ij /* E x 2, indices within the graph */,
                                 const double *edge_meas /* E x 3 */, const double *edge_info /* E x 6: xx xy xt yy yt tt */,
                                 const double *edge_huber /* E or NULL; 0 = no kernel on that edge */,
                                 const roam_pose_graph_opts *opts, roam_pose_graph_stats *stats /* n */);

/* ---- loop-closure candidates: radar scan context (Kim et al., MulRan).  The reference has no place recognition (Mapping.py:7 is a
 * commented-out "import m2dp", :61-62 an unused Keyframe.pointCloud): PARITY UNPINNED, the contract is tests/scan_context_model.py.
 * Bins (integer arithmetic): clip = clip_px if 0 < clip_px < cols else cols; sector s = rows [floor(s rows / S), floor((s + 1) rows / S)),
 * ring r = columns [floor(r clip / R), floor((r + 1) clip / R)); rows >= S and clip >= R, so no bin is empty.
 * Descriptor D[s][r], float32: u8 record codes k with an integer floor f: (float)((double)sum max(k - f, 0) / (255.0 count)), the sum an
 * exact integer; float32 values v with a float floor f >= 0: (float)(sum max((double)v - (double)f, 0) / count), summed in float64 in
 * a fixed order (within 1 float32 ulp of any other order).  floor = 0 is the plain area mean.
 * Distance of descriptors q, c: sector s is valid at shift k when |q[s]| |c[(s + k) mod S]| > 0 (float64 norms over the rings);
 * d_k = 1 - (1 / count_k) sum over valid s of q[s] . c[(s + k) mod S] / (|q[s]| |c[(s + k) mod S]|), d_k = 1 when count_k = 0;
 * distance = min_k d_k, shift = the lowest k of the minimum; yaw(query) - yaw(candidate) ~ 2 pi shift / S for rows = atan2(y, x) rows / 2 pi.
 * The device sums normalised columns in float64 in one order per (S, R): the same pair gives the same bits wherever the candidate
 * sits, whatever the database size, the number of queries and the chunk.
 * Candidates of query i: the k smallest by (distance, then index) among the entries j < max_index[i] with distance <= max_distance;
 * unused slots hold index -1, distance +inf, shift 0. */
#define ROAM_SCAN_CONTEXT_MAX_SECTORS 256
#define ROAM_SCAN_CONTEXT_MAX_RINGS 128
#define ROAM_SCAN_CONTEXT_MAX_CLIP 4096     /* range bins kept (the sector's column sums live in LDS) */
#define ROAM_LOOP_MAX_K 32
typedef struct roam_loop_db roam_loop_db;
/* host only, no context: the argument checks of the describing entries and the bin edges (either array may be NULL).  ROAM_E_ARG:
 * sectors outside [2, 256], rings outside [1, 128], rows < sectors or > 65536, cols < 1, clip < rings or > 4096 */
int32_t roam_scan_context_plan(int32_t rows, int32_t cols, int32_t clip_px, int32_t sectors, int32_t rings, int32_t *row_edges /* S + 1 */,
                               int32_t *col_edges /* R + 1 */);
/* stateless: n host float32 images (strides in floats, as roam_fmt_rotation_batch_f32) -> desc_out (n, S, R) float32.  Images are
 * uploaded in chunks under 2000 MiB.  ROAM_E_ARG before any device call, the text naming the argument: null pointers, n < 1, what
 * roam_scan_context_plan refuses, row_stride < cols, image_stride below an image's extent (n > 1), floor negative or not finite */
int32_t roam_scan_context_f32(roam_ctx *ctx, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride,
                              int64_t image_stride, int32_t clip_px, int32_t sectors, int32_t rings, double floor, float *desc_out);
/* a database of descriptors in HBM: per entry the float32 descriptor, its columns divided by their float64 norms (what a query
 * reads: stored entries are never normalised again) and a validity flag per sector.  ROAM_E_ARG: sectors / rings outside the limits,
 * capacity < 1 or more than fits 2000 MiB */
int32_t roam_loop_db_create(roam_ctx *ctx, int32_t capacity, int32_t sectors, int32_t rings, roam_loop_db **out);
int32_t roam_loop_db_destroy(roam_ctx *ctx, roam_loop_db *db);
int32_t roam_loop_db_count(const roam_loop_db *db, int32_t *count);
/* describe n host float32 images as roam_scan_context_f32 does and append them on the device (the descriptor never visits the host);
 * first_index_out (optional) = the index of the first new entry.  ROAM_E_CAPACITY when they do not fit: the database is unchanged */
int32_t roam_loop_db_add_f32(roam_ctx *ctx, roam_loop_db *db, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride,
                             int64_t image_stride, int32_t clip_px, double floor, int32_t *first_index_out);
/* append n ready-made descriptors (n, S, R) float32 (finite values: ROAM_E_ARG otherwise) */
int32_t roam_loop_db_add_desc(roam_ctx *ctx, roam_loop_db *db, const float *desc, int32_t n, int32_t *first_index_out);
/* the stored descriptors first .. first + n - 1 -> desc_out (n, S, R) */
int32_t roam_loop_db_get(roam_ctx *ctx, roam_loop_db *db, int32_t first, int32_t n, float *desc_out);
/* describe n resident u8 records of the engine's pool (pool_idx[n], host) in place and append them: the integer form above with
 * floor_code in [0, 254], clip = min(clip_px, cfg.clip), clip_px <= 0: cfg.clip.  Runs on the compute stream behind every step
 * enqueued so far and the pool's pending uploads, blocks until done and leaves the engine's bookkeeping alone.  ROAM_E_ARG: null
 * pointers, n < 1, a pool index out of range, cfg.rows < sectors, clip < rings or > 4096, floor_code outside [0, 254] */
int32_t roam_engine_loop_db_add(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t clip_px, int32_t floor_code,
                                int32_t *first_index_out);
/* queries are entries of the database (add first, then ask): for query_index[i], i < n_query, the distance and shift to every entry
 * and its k candidates as defined above.  max_index[i] is clamped to [0, count].  dist_full / shift_full (optional, for tests):
 * (n_query, count) float64 / int32, every pair whatever max_index says.  Queries are processed in chunks that keep the device scratch
 * under 2000 MiB (ROAM_LOOP_CHUNK_BYTES in the environment, read per call, lowers where a batch is cut - for tests).
 * ROAM_E_ARG before any device call: null pointers, n_query < 1, k outside [1, 32], max_distance NaN, a query index outside the
 * database */
int32_t roam_loop_db_query(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index, int32_t k,
                           double max_distance, int32_t *cand_index /* n k */, double *cand_dist /* n k */, int32_t *cand_shift /* n k */,
                           double *dist_full, int32_t *shift_full);
/* measurement: HIP events on the context stream around `reps` launches, two warm ones first -> milliseconds per launch.
 * roam_engine_time_loop_describe: the describing kernel of roam_engine_loop_db_add on the same n records, written into the free
 * entries of db (they must fit; nothing is appended).  roam_time_loop_db_query: the distance kernel (with the max_index mask, as a
 * query without the full outputs runs it) and the selection kernel of roam_loop_db_query, which must fit one launch */
int32_t roam_engine_time_loop_describe(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t clip_px, int32_t floor_code,
                                       int32_t reps, float *ms_per_rep);
int32_t roam_time_loop_db_query(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index, int32_t k,
                                double max_distance, int32_t reps, float *distance_ms, float *select_ms);

/* ---- loop-closure verification: batched trimmed point-to-point ICP in the plane (csrc/icp.hip).  The reference has no such step
 * (its Keyframe.pointCloud, Mapping.py:61-62, is never read): PARITY UNPINNED, the contract is tests/icp_model.py.
 * Pair p aligns src (the points src_off[p] .. src_off[p + 1], float64 metres, x y interleaved) to dst (dst_off likewise) from the pose
 * init[p] = (theta, tx, ty) and returns the pose with dst ~ R(theta) src + t.  One workgroup per pair, the iteration loop inside the
 * kernel.  Iteration k, gate g_k (g_0 = gate_start, g_{k+1} = max(gate_end, g_k gate_decay)):
 *   q_i = R(theta) src_i + t in float64, rounded to float32; dst rounded to float32; the partner j(i) minimises
 *   d2 = fl32(fl32(dx dx) + fl32(dy dy)) over the float32 differences (no fused multiply-add), the lowest j of the minimum, by
 *   exhaustive search; pair i is kept when d2 <= fl32(g_k g_k).  Fewer than min_pairs kept: FEW_PAIRS, the pose stays, the loop ends.
 *   Over the kept pairs, float64, from the float64 coordinates: the centroids am, bm, then S_cos = sum (a - am) . (b - bm) and
 *   S_sin = sum (a - am) x (b - bm) in a second pass; theta' = atan2(S_sin, S_cos), or theta when both sums are exactly 0;
 *   t' = bm - R(theta') am.  After the update: OK when g_k == gate_end, |wrap(theta' - theta)| < eps_rot and |t' - t| < eps_trans;
 *   MAX_ITERATIONS after max_iterations updates.
 * One scoring pass at the final pose with gate_end (also after FEW_PAIRS): n_inliers = the kept pairs, rms = sqrt(mean d2) with d2 in
 * float64 between the float64 transformed point and its partner's float64 coordinates, +inf when n_inliers = 0.  An empty src or dst:
 * FEW_PAIRS, the initial pose, 0 inliers.  iterations = the updates made; n_pairs_last = the pairs kept by the loop's last search.
 * Sums run in one order per pair (a lane over its points i = lane, lane + 512, ...; the wave's xor butterfly; the waves in order), no
 * floating-point atomics: a pair's result is the same bits alone, anywhere in a batch, in any chunk and in any call.  Pairs are
 * processed in chunks that keep the device scratch under 2000 MiB (ROAM_ICP_CHUNK_BYTES in the environment, read per call, lowers
 * where a batch is cut - for tests).
 * Limits: 1 .. 65535 pairs, 0 .. 8192 points per cloud, coordinates, translations and gates within 1e6 m (float32 then holds every
 * squared distance), max_iterations in [1, 1000].
 * ROAM_E_ARG before any device call: a null pointer (opts may be NULL: the defaults 3.0 m, 0.5 m, 0.8, 40, 1e-4 m, 1e-5 rad, 3),
 * a limit exceeded, a negative first or a decreasing offset, a coordinate or pose that is not finite, gates not
 * 0 < gate_end <= gate_start, gate_decay outside (0, 1], min_pairs < 2, a negative or NaN eps. */
#define ROAM_ICP_MAX_PAIRS 65535
#define ROAM_ICP_MAX_POINTS 8192
#define ROAM_ICP_MAX_COORD 1e6
#define ROAM_ICP_ITERATION_LIMIT 1000
enum { ROAM_ICP_OK = 0, ROAM_ICP_MAX_ITERATIONS = 1, ROAM_ICP_FEW_PAIRS = 2 };
typedef struct roam_icp_opts {
    double  gate_start, gate_end;   /* metres */
    double  gate_decay;
    int32_t max_iterations;
    double  eps_trans, eps_rot;     /* metres, radians */
    int32_t min_pairs;
} roam_icp_opts;
typedef struct roam_icp_stats {
    int32_t status, iterations, n_pairs_last, n_inliers;
    double  rms;
} roam_icp_stats;
int32_t roam_icp2d_batch(roam_ctx *ctx, int32_t n_pairs, const int32_t *src_off /* n + 1 */, const double *src /* N x 2 */,
                         const int32_t *dst_off /* n + 1 */, const double *dst /* M x 2 */, const double *init /* n x 3: theta tx ty */,
                         const roam_icp_opts *opts, double *pose_out /* n x 3: theta tx ty */, roam_icp_stats *stats /* n */);
/* measurement: the pairs are uploaded once, then HIP events on the context stream around `reps` launches of the kernel, two warm
 * ones first -> milliseconds per launch.  The pairs must fit one launch */
int32_t roam_time_icp2d_batch(roam_ctx *ctx, int32_t n_pairs, const int32_t *src_off, const double *src, const int32_t *dst_off,
                              const double *dst, const double *init, const roam_icp_opts *opts, int32_t reps, float *ms_per_rep);

/* ---- loop database with resident peak clouds: verification from the store (csrc/loop_cloud.hip, csrc/loop_verify.hip, csrc/icp.hip).  PARITY UNPINNED as
 * the two sections above; the contract is tests/loop_cloud_model.py on top of tests/icp_model.py.
 * A database that keeps clouds stores beside every descriptor the scan's polar peaks in metres.  The peaks are those of
 * roam_peaks_record_u8 / roam_peaks_polar_f32 in their azimuth-major order (a record: the engine's cfg.clip columns; an image: all its
 * columns, whatever clip_px the descriptor uses), N of them.  step = max(point_stride, ceil(N / max_points)); the entry keeps the peaks
 * q = 0, step, 2 step, ... (ceil(N / step) points) as x = fl64(fl64(r range_resolution_m) cos_t[theta]), y likewise with sin_t, every
 * multiply rounded once; N stays readable.  cos_t / sin_t are roam_polar_cloud_table's: the host's libm, the device only multiplies.
 * What is stored depends on the scan alone - not on the batch, the position or the chunk (ROAM_LOOP_CHUNK_BYTES also cuts these).
 *
 * roam_polar_cloud_table: host only, no context.  phi_t = (2.0 * M_PI * t) / rows in float64 (two rounded operations), t < rows <=
 * 65536; ROAM_E_ARG outside the limits or for a null pointer.
 * roam_loop_db_keep_clouds: once, on an empty database; every later roam_loop_db_add_f32 / roam_engine_loop_db_add must have `rows`
 * azimuths (and at most ROAM_MAX_COLS columns) and stores the cloud with the descriptor; roam_loop_db_add_desc stores an empty cloud.
 * ROAM_E_ARG, the text naming the argument: db not empty or keeping clouds already, max_points outside [1, ROAM_ICP_MAX_POINTS],
 * point_stride < 1, range_resolution_m not finite or <= 0, rows outside [1, 65536], capacity x max_points x 16 bytes beyond 2000 MiB.
 * A failed add leaves descriptors and clouds as they were.
 * roam_loop_db_set_cloud replaces the cloud of a stored entry from the host (n <= max_points points, coordinates within
 * ROAM_ICP_MAX_COORD; the entry's peak count becomes n); roam_loop_db_get_cloud reads it back: *n_out points stored, *n_peaks_out
 * peaks the scan had, the first min(n, cap) points in xy_out, ROAM_E_CAPACITY when n > cap.  roam_loop_db_cloud_counts: the two counts
 * of the entries first .. first + n - 1 from the host's copy, no device call.  ROAM_E_STATE: the database keeps no clouds. */
int32_t roam_polar_cloud_table(int32_t rows, double *cos_out /* rows */, double *sin_out /* rows */);
int32_t roam_loop_db_keep_clouds(roam_ctx *ctx, roam_loop_db *db, int32_t rows, int32_t max_points, int32_t point_stride,
                                 double range_resolution_m);
int32_t roam_loop_db_set_cloud(roam_ctx *ctx, roam_loop_db *db, int32_t index, const double *xy /* n x 2 */, int32_t n);
int32_t roam_loop_db_get_cloud(roam_ctx *ctx, roam_loop_db *db, int32_t index, double *xy_out /* cap x 2 */, int32_t cap, int32_t *n_out,
                               int32_t *n_peaks_out);
int32_t roam_loop_db_cloud_counts(const roam_loop_db *db, int32_t first, int32_t n, int32_t *n_out, int32_t *n_peaks_out);
/* roam_icp2d_batch's iteration on pairs of stored clouds: pair p aligns the cloud of entry src_index[p] to that of entry dst_index[p]
 * from init[p]; an empty cloud on either side is FEW_PAIRS with the pose equal to the seed.  Options, their checks and every bit of
 * a pair's result are roam_icp2d_batch's on the same clouds.  The partner scratch is per pair, so one entry may be the source of any
 * number of pairs of a call.  1 .. 65535 pairs, cut into launches under 2000 MiB of scratch (ROAM_LOOP_CHUNK_BYTES lowers it).
 * ROAM_E_ARG before any device call: null pointers, an index outside the stored entries, a seed that is not finite, bad options.
 *
 * roam_loop_db_query_verify: roam_loop_db_query's distance and selection kernels, a kernel that turns slot (i, s) into the pair
 * (source = entry query_index[i], destination = candidate (i, s), seed (yaw, 0, 0) with yaw = (6.283185307179586 shift) / S, minus
 * 6.283185307179586 when that exceeds 3.141592653589793) and the ICP kernel, enqueued on the context's stream with no host
 * synchronisation between them, then one read-back.  cand_* are what roam_loop_db_query returns for the same arguments; pose_out /
 * stats row i k + s belongs to slot (i, s), an unused slot (index -1) is FEW_PAIRS at its seed (0, 0, 0). */
int32_t roam_loop_db_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_pairs, const int32_t *src_index, const int32_t *dst_index,
                            const double *init /* n x 3 */, const roam_icp_opts *opts, double *pose_out /* n x 3 */, roam_icp_stats *stats /* n */);
int32_t roam_loop_db_query_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                  int32_t k, double max_distance, const roam_icp_opts *opts, int32_t *cand_index /* n k */,
                                  double *cand_dist /* n k */, int32_t *cand_shift /* n k */, double *pose_out /* n k 3 */,
                                  roam_icp_stats *stats /* n k */);
/* measurement, as roam_engine_time_loop_describe / roam_time_icp2d_batch: HIP events on the context's stream, two warm launches, `reps`
 * timed -> milliseconds per launch.  roam_engine_time_loop_cloud: the cloud build of n resident records into the free entries of db
 * (nothing is appended), its two kernels apart - the peak row kernel and the cloud gather.  roam_time_loop_db_verify: the ICP launch
 * on these stored pairs, which must fit one launch */
int32_t roam_engine_time_loop_cloud(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t reps, float *rows_ms,
                                    float *gather_ms);
int32_t roam_time_loop_db_verify(roam_ctx *ctx, roam_loop_db *db, int32_t n_pairs, const int32_t *src_index, const int32_t *dst_index,
                                 const double *init, const roam_icp_opts *opts, int32_t reps, float *ms_per_rep);
/* motion compensation of the stored clouds (csrc/cloud_motion.h, cloud_gather_motion_kernel in csrc/loop_cloud.hip).  PARITY UNPINNED as
 * the clouds; the contract is tests/loop_cloud_motion_model.py, which is the reference's MotionDistortionSolver.undistort with the time
 * of a point taken from its azimuth row instead of atan2.
 * A scan sweeps its `rows` azimuths over `period` seconds.  With the scan's velocity v = (vx, vy, vtheta) - m/s, m/s, rad/s in the
 * sensor frame of the stored points, roam_keyframe_hdr.velocity - the peak of row t is stored where mid-scan would have seen it:
 *   tau_t = period ((2 t - rows) / (2 rows))   (-period / 2 at row 0, 0 at mid-scan), a = vtheta tau_t, C = cos a, S = sin a by the
 *   host's libm, DX = vx tau_t, DY = vy tau_t;   with (x0, y0) the plain stored point above:
 *   x = ((C x0) - (S y0)) + DX, y = ((S x0) + (C y0)) + DY, every operation one float64 operation rounded once.
 * The selection of the peaks is unchanged.  roam_cloud_motion_table: host only, no context; out (n, rows, 4) = C S DX DY of every row
 * of n scans, velocities (n, 3); a scan whose vx is NaN has NO velocity - its rows are NaN, and an add stores its plain cloud, bit for
 * bit.  ROAM_E_ARG: rows outside [1, 65536], n < 1, a null pointer, period not finite or <= 0, a component that is not finite (other
 * than that marker).  The device only multiplies and adds with the table, which follows the chunks of an add (32 bytes per row beside
 * the staging): what is stored depends on the scan and its velocity alone.
 * roam_loop_db_add_f32_motion / roam_engine_loop_db_add_motion: roam_loop_db_add_f32 / roam_engine_loop_db_add with velocities
 * (n, 3), one row per scan, or NULL - then they ARE those entries, which call them so, and period is not read.  ROAM_E_ARG before any
 * device call, the text naming the argument, beyond what those entries refuse: velocities for a database that keeps no clouds; period
 * not finite or <= 0; a velocity component that is not finite (other than the marker); a velocity for which hypot(vx, vy) period / 2
 * plus the largest range cols range_resolution_m exceeds ROAM_ICP_MAX_COORD.  A failed add leaves the database as it was.
 * roam_engine_time_loop_cloud_motion: roam_engine_time_loop_cloud with such velocities - the gather's motion form, its table
 * uploaded once before the launches. */
int32_t roam_cloud_motion_table(int32_t rows, double period, int32_t n, const double *velocities /* n x 3 */,
                                double *out /* n x rows x 4: C S DX DY */);
int32_t roam_loop_db_add_f32_motion(roam_ctx *ctx, roam_loop_db *db, const float *polar, int32_t n, int32_t rows, int32_t cols,
                                    int64_t row_stride, int64_t image_stride, int32_t clip_px, double floor,
                                    const double *velocities /* n x 3 or NULL */, double period, int32_t *first_index_out);
int32_t roam_engine_loop_db_add_motion(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t clip_px,
                                       int32_t floor_code, const double *velocities /* n x 3 or NULL */, double period,
                                       int32_t *first_index_out);
int32_t roam_engine_time_loop_cloud_motion(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx,
                                           const double *velocities /* n x 3 or NULL */, double period, int32_t reps, float *rows_ms,
                                           float *gather_ms);

/* ---- origin-shifted scan contexts: revisits metres off the stored place (csrc/loop_offset.hip; the augmentation of Scan Context++,
 * Kim, Choi, Kim, T-RO 2021).  PARITY UNPINNED as the sections above; the contract is tests/scan_context_offset_model.py.
 * A scan is described again as seen from n_offsets virtual origins o (metres, the sensor frame x = r cos phi, y = r sin phi; in range
 * bins o / range_resolution_m, one float64 division).  Every sample (a, c), a < rows, c < clip, sits at its centre: rho = c + 0.5,
 * (C_a, S_a) = (cos, sin)((2.0 * M_PI * (a + 0.5)) / rows) by the host's libm; x = rho C_a - ox, y = rho S_a - oy, q = x x + y y, each
 * operation rounded once in float64.  Ring r: E_r^2 <= q < E_{r+1}^2 with roam_scan_context_plan's column edges; q >= clip^2 is dropped.
 * Sector: b_s = (cos, sin)((2.0 * M_PI * row_edges[s]) / rows) by the host's libm, k_s = b_s.x y - b_s.y x, the lowest s with k_s >= 0
 * and k_{(s + 1) mod S} < 0; none: dropped.  A bin holds the mean of max(value - floor, 0) over the samples that landed in it (u8: the
 * exact integer sum / (255.0 count); float32: summed in float64 in one order per (rows, clip, S, R), within 1 float32 ulp of any other and
 * the same bits whatever the batch and the chunk), 0 when none did.  roam_scan_context_offset_table (host only, no context) returns
 * the four tables; ROAM_E_ARG outside roam_scan_context_plan's limits or for a null pointer.
 * Variant 0 of an entry is its plain descriptor, variant a >= 1 the one of offsets_m[a - 1].  roam_loop_db_keep_offsets: once, on an
 * empty database; every later roam_loop_db_add_f32 / roam_engine_loop_db_add also stores the n_offsets variants of each new entry
 * (descriptor, normalised columns, validity - as an entry's own), roam_loop_db_add_desc stores them all zero (invalid: distance 1).
 * ROAM_E_ARG before any device call, the text naming the argument: n_offsets outside [1, ROAM_LOOP_MAX_OFFSETS], an offset that is not
 * finite, beyond ROAM_ICP_MAX_COORD or (0, 0), range_resolution_m not finite or <= 0, a database that is not empty or keeps offsets
 * already, capacity x n_offsets variants beyond 2000 MiB.  roam_loop_db_set_variants / _get_variants move the n_offsets descriptors
 * (n_offsets, S, R) of one stored entry from and to the host (valid_out optional: (n_offsets, S)); ROAM_E_STATE: no offsets kept.
 * roam_scan_context_offsets_f32: stateless, roam_scan_context_f32's arguments and checks -> desc_out (n, 1 + n_offsets, S, R).
 * Queries.  D(i, j) = min over the variants a of query i of d(variant a of i, entry j), d as defined above; ties take the lowest a,
 * the shift is that variant's; candidates by the rule above on D.  roam_loop_db_query_offsets: roam_loop_db_query's arguments and
 * checks plus cand_offset (n k) and offset_full (optional, (n_query, count)): the winning variant a, 0 for an unused slot.  On a
 * database without offsets it is roam_loop_db_query with all variants 0, and roam_loop_db_query is unchanged on every database.
 * Verification.  On a database that keeps offsets roam_loop_db_query_verify runs the query over the variants and seeds slot (i, s)
 * with (yaw, -R(yaw) o) for the winning offset o (metres; (yaw, 0, 0) for variant 0), still without a host round trip;
 * roam_loop_db_query_verify_offsets also returns the winning variants.
 * Measurement, as above: roam_engine_time_loop_offsets - the variants of n resident records into the free entries of db (the clear
 * of the sums, the binning kernel and the finishing kernel as one launch); roam_time_loop_db_query_offsets - the plain distance
 * kernel, the variants' distance kernel with the fold, and the selection kernel. */
#define ROAM_LOOP_MAX_OFFSETS 48
int32_t roam_scan_context_offset_table(int32_t rows, int32_t sectors, double *cos_row /* rows */, double *sin_row /* rows */,
                                       double *cos_edge /* S */, double *sin_edge /* S */);
int32_t roam_loop_db_keep_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n_offsets, const double *offsets_m /* n x 2 */,
                                  double range_resolution_m);
int32_t roam_loop_db_set_variants(roam_ctx *ctx, roam_loop_db *db, int32_t index, const float *desc /* n_offsets x S x R */);
int32_t roam_loop_db_get_variants(roam_ctx *ctx, roam_loop_db *db, int32_t index, float *desc_out, int32_t *valid_out);
int32_t roam_scan_context_offsets_f32(roam_ctx *ctx, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride,
                                      int64_t image_stride, int32_t clip_px, int32_t sectors, int32_t rings, double floor,
                                      int32_t n_offsets, const double *offsets_m, double range_resolution_m, float *desc_out);
int32_t roam_loop_db_query_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                   int32_t k, double max_distance, int32_t *cand_index, double *cand_dist, int32_t *cand_shift,
                                   int32_t *cand_offset, double *dist_full, int32_t *shift_full, int32_t *offset_full);
int32_t roam_loop_db_query_verify_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index,
                                          const int32_t *max_index, int32_t k, double max_distance, const roam_icp_opts *opts,
                                          int32_t *cand_index, double *cand_dist, int32_t *cand_shift, int32_t *cand_offset,
                                          double *pose_out, roam_icp_stats *stats);
int32_t roam_engine_time_loop_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n, const int32_t *pool_idx, int32_t clip_px,
                                      int32_t floor_code, int32_t reps, float *ms_per_rep);
int32_t roam_time_loop_db_query_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n_query, const int32_t *query_index,
                                        const int32_t *max_index, int32_t k, double max_distance, int32_t reps, float *plain_ms,
                                        float *variants_ms, float *select_ms);

/* ---- global map: the resident peak clouds binned at given poses (csrc/loop_map.hip).  The reference's Map.mapPoints is an empty list
 * with a TODO beside it (Mapping.py: "a big array of map points in global coordinates") and Map.plot scatters global feature points;
 * nothing there computes a map, so PARITY UNPINNED as the sections above; the contract is tests/global_map_model.py.
 * In: a database that keeps clouds, `count` entries; poses (count, 3) rows x, y, theta - finite, |x| and |y| <= ROAM_ICP_MAX_COORD;
 * use (count) int8, 0 leaves the entry out, NULL = every entry; the cell size res in metres; the extent: origin (ox, oy), W x H cells.
 * Every operation below is one float64 operation rounded once.
 * Pose table.  roam_map_pose_table (host only, no context): cs_out (n, 2) = (cos theta, sin theta) by the host's libm, as
 * roam_polar_cloud_table; the device only multiplies with these values.  ROAM_E_ARG: n < 0, a null pointer, a theta that is not finite.
 * World point of the stored point (px, py) of entry e: wx = ((c px) - (s py)) + x, wy = ((s px) + (c py)) + y.
 * Cell.  dx = (wx - ox) / res, dy = (wy - oy) / res; the point is inside when 0 <= dx < W and 0 <= dy < H, compared in float64 before
 * any conversion; then u = floor(dx), v = floor(dy), otherwise the point counts in n_outside.  dx - u is exact, and the sub-cell
 * position is qx = floor((dx - u) * 65536.0) in [0, 65535]; qy likewise.
 * Per cell, integers all, so that the result does not depend on the order of arrival: hits (uint32) the points that landed in it,
 * views (uint32) the distinct entries that put at least one point there, sx, sy (uint64) the sums of qx and qy.
 * Map points.  A cell qualifies when hits >= min_hits and views >= min_views (both >= 1); the qualifying cells in row-major order, v
 * major, each as (cx, cy, hits, views): m = (2 sx + hits) / (131072.0 hits) (the numerator an exact integer below 2^53),
 * cx = ox + res * (u + m), cy likewise.  More of them than cap: ROAM_E_CAPACITY, no point is written and *n_points_out is the count
 * required.
 * Automatic extent.  roam_loop_db_map_bounds: bounds_out = {min wx, max wx, min wy, max wy} over the used entries' points, exactly (a
 * zero bound is +0), and *n_points_out their number; with no point the bounds are {+inf, -inf, +inf, -inf}.  roam_map_plan (host only,
 * no context): ox = (floor(minx / res) - 1) * res, W = floor((maxx - ox) / res) + 2, the y side likewise - one cell of margin on each
 * side, so that the rounding of ox cannot push a bounding point outside: with a planned extent n_outside is 0.  ROAM_E_ARG: a null
 * pointer, bounds that are not finite, min > max, res not finite or <= 0, |floor(min / res)| > ROAM_MAP_MAX_INDEX (a cell so fine
 * against the coordinates that the margin's two operations are no longer nearly exact).  ROAM_E_CAPACITY: W H > ROAM_MAP_MAX_CELLS
 * (at 24 bytes per cell the grid stays under the 2000 MiB every other stage keeps to).
 * roam_loop_db_map_render: the grid's clear, the splat (one workgroup per entry: the entry's cell keys sorted in LDS, a run of equal
 * keys adds its length and its sums once and one view; integer atomics only), the compaction (a count per chunk of the row-major
 * grid, an exclusive scan, the write) - enqueued on the context's stream with no host synchronisation between them - and the
 * read-back: the two counters with hits_out / views_out ((H, W) each, either may be NULL), then the *n_points_out records the counters
 * announce.  The grid is scratch of the call: the database keeps no map, and a database never asked for one is untouched.
 * ROAM_E_STATE: the database keeps no clouds.  ROAM_E_ARG before any device call, the text naming the argument: null pointers
 * (points_out, point_hits_out, point_views_out may be NULL when cap is 0), a pose that is not finite or beyond the limit, res not
 * finite or <= 0, an origin that is not finite, W or H < 1, W H > ROAM_MAP_MAX_CELLS, a threshold < 1, cap < 0.  An empty database, or
 * one with nothing used, gives an all-zero grid and no points.
 * roam_time_loop_db_map: measurement as above (HIP events, two warm launches, `reps` timed) -> ms[3]: the clear, the splat and the
 * compaction apart. */
#define ROAM_MAP_MAX_CELLS (1 << 26)
#define ROAM_MAP_MAX_INDEX 1125899906842624.0 /* 2^50 */
int32_t roam_map_pose_table(int32_t n, const double *poses /* n x 3 */, double *cs_out /* n x 2 */);
int32_t roam_map_plan(double minx, double maxx, double miny, double maxy, double res, double *ox, double *oy, int32_t *W, int32_t *H);
int32_t roam_loop_db_map_bounds(roam_ctx *ctx, roam_loop_db *db, const double *poses /* count x 3 */, const int8_t *use /* count or NULL */,
                                double *bounds_out /* 4 */, int64_t *n_points_out);
int32_t roam_loop_db_map_render(roam_ctx *ctx, roam_loop_db *db, const double *poses, const int8_t *use, double res, double ox, double oy,
                                int32_t W, int32_t H, int32_t min_hits, int32_t min_views, uint32_t *hits_out /* H x W */,
                                uint32_t *views_out /* H x W */, double *points_out /* cap x 2 */, uint32_t *point_hits_out /* cap */,
                                uint32_t *point_views_out /* cap */, int32_t cap, int32_t *n_points_out, int64_t *n_outside_out);
int32_t roam_time_loop_db_map(roam_ctx *ctx, roam_loop_db *db, const double *poses, const int8_t *use, double res, double ox, double oy,
                              int32_t W, int32_t H, int32_t min_hits, int32_t min_views, int32_t reps, float *ms /* 3 */);

/* ---- map matching: a scan localised in a rendered global map by correlative scan-to-map matching (csrc/map_match.hip; the host-only
 * half is csrc/map_match.h).  The reference left Map.mapPoints a TODO and computes none of this, so PARITY UNPINNED as the sections
 * above; the contract is tests/map_match_model.py.  Every floating-point step below is one float64 operation rounded once; everything
 * accumulated is an integer, so the result is bit-reproducible and no order of arrival can show.
 * Table.  roam_map_field_table (host only, no context): the side is 2 radius + 1,
 * T[dv + r][du + r] = (uint8) floor(255 * exp(-(double)(du du + dv dv) / (2 sigma sigma)) + 0.5) by the host's libm - the device never
 * calls exp.  ROAM_E_ARG: radius outside [0, ROAM_MATCH_MAX_RADIUS], sigma_cells not finite or <= 0, a null pointer.
 * Field.  roam_map_field_create: hits, views (H, W) uint32 on the host (what roam_loop_db_map_render gave), the extent as there.  A
 * cell is occupied when hits >= min_hits and views >= min_views; F[v][u] = the maximum over |dv|, |du| <= radius, (v + dv, u + du) inside
 * the grid and occupied, of T[dv + r][du + r], 0 without such a cell.  One byte per cell, built by mm_field_kernel from the uploaded
 * grids (scratch of the call) and resident in the handle until roam_map_field_destroy; roam_map_field_read copies it out, (H, W).
 * ROAM_E_ARG before any device call, the text naming the argument: a null pointer, res not finite or <= 0, an origin that is not
 * finite, W or H < 1, W H > ROAM_MAP_MAX_CELLS, a threshold < 1, radius outside [0, ROAM_MATCH_MAX_RADIUS].
 * Match.  roam_map_match_clouds: n_query (1 ... 65535) clouds concatenated in xy ((total, 2) float64 metres, sensor frame, |coord| <=
 * ROAM_ICP_MAX_COORD), cloud q the rows [offsets[q], offsets[q + 1]) (offsets (n_query + 1) int64, ascending from 0, at most
 * ROAM_ICP_MAX_POINTS rows each); priors (n_query, 3) rows x0, y0, th0 (limits of the render's poses); the window: n_theta odd in
 * [1, ROAM_MATCH_MAX_ANGLES] angles step_rad apart (finite, >= 0), kx, ky in [0, ROAM_MATCH_MAX_SHIFT] cells of shift to either side.
 * Angles.  c = (n_theta - 1) / 2, th_i = th0 + (double)(i - c) * step_rad; roam_map_match_angles (host only, no context): cs_out
 * (n_query, n_theta, 2) = (cos th_i, sin th_i) by the host's libm - what the device multiplies with.
 * Cell of a point (px, py) at angle i: wx = ((c_i px) - (s_i py)) + x0, wy = ((s_i px) + (c_i py)) + y0 (the global map's world
 * point); dx = (wx - ox) / res, dy likewise; the point is far when not -2^30 <= dx < 2^30 (dy likewise) and never scores; otherwise
 * u = (int32) floor(dx), v = (int32) floor(dy).
 * Score.  score(i, b, a) = the sum over the not-far points of F[v + (b - ky)][u + (a - kx)], positions outside the grid counting 0: a
 * translation is an exact shift of the cell index, not a re-binning of a translated point.  A uint32 (8192 x 255 fits).
 * Best.  The largest score, among ties the lowest flat index (i (2 ky + 1) + b) (2 kx + 1) + a - through an integer maximum of
 * (score << 32 | ~flat), so no order shows.  pose_out (n_query, 3): x0 + (double)(a - kx) * res, y0 + (double)(b - ky) * res, th_i;
 * info_out (n_query, 6) int32: score, i, b, a, n_points, n_inside (the not-far points whose shifted cell is inside the grid at the
 * best candidate).  A score of 0: nothing matched (the best is then flat index 0).  scores_out (NULL, or (n_query, n_theta, 2 ky + 1,
 * 2 kx + 1) uint32, at most ROAM_MATCH_MAX_VOLUME entries): the whole score volume.
 * roam_loop_db_map_match: the same with cloud q = the resident cloud of entry index[q] of a cloud-keeping database; no cloud crosses
 * the host.  ROAM_E_STATE: the database keeps no clouds.  ROAM_E_ARG, before any device call and with the text naming the argument:
 * null pointers, a database and a field of different contexts (or not of ctx), an index out of range, and what the clouds entry refuses.
 * roam_map_match_plan (host only, no context): how a call of n_query queries with this window is cut on a device of cu_count compute
 * units: one workgroup per (query, angle, block of *rows_out of the 2 ky + 1 shift rows), *n_blk_out blocks - at most 2048 candidates
 * to a workgroup, fewer rows while fewer than about four workgroups per unit would result, never fewer than fill 256 lanes.  The cut
 * changes no result.  ROAM_E_ARG: a null pointer, cu_count < 1, n_query or a window that the match refuses.
 * roam_time_map_match: measurement only (HIP events, two warm launches, `reps` timed): ms[0] the field's build from the uploaded grids
 * into scratch (the handle's field is untouched), ms[1] the match kernels of this call's window on the handle's field. */
#define ROAM_MATCH_MAX_RADIUS 8
#define ROAM_MATCH_MAX_ANGLES 1025
#define ROAM_MATCH_MAX_SHIFT 128
#define ROAM_MATCH_MAX_VOLUME (1 << 26)
typedef struct roam_map_field roam_map_field;
int32_t roam_map_field_table(double sigma_cells, int32_t radius, uint8_t *table_out /* (2 radius + 1)^2 */);
int32_t roam_map_field_create(roam_ctx *ctx, double ox, double oy, double res, int32_t W, int32_t H, const uint32_t *hits /* H x W */,
                              const uint32_t *views /* H x W */, int32_t min_hits, int32_t min_views, int32_t radius,
                              const uint8_t *table /* (2 radius + 1)^2 */, roam_map_field **field_out);
int32_t roam_map_field_read(roam_ctx *ctx, roam_map_field *field, uint8_t *out /* H x W */);
int32_t roam_map_field_destroy(roam_ctx *ctx, roam_map_field *field);
int32_t roam_map_match_angles(int32_t n_query, const double *priors /* n x 3 */, int32_t n_theta, double step_rad,
                              double *cs_out /* n x n_theta x 2 */);
int32_t roam_map_match_plan(int32_t cu_count, int32_t n_query, int32_t n_theta, int32_t kx, int32_t ky, int32_t *rows_out, int32_t *n_blk_out);
int32_t roam_map_match_clouds(roam_ctx *ctx, roam_map_field *field, int32_t n_query, const double *xy /* total x 2 */,
                              const int64_t *offsets /* n_query + 1 */, const double *priors /* n_query x 3 */, int32_t n_theta,
                              double step_rad, int32_t kx, int32_t ky, double *pose_out /* n_query x 3 */,
                              int32_t *info_out /* n_query x 6 */, uint32_t *scores_out /* NULL or the volume */);
int32_t roam_loop_db_map_match(roam_ctx *ctx, roam_loop_db *db, roam_map_field *field, int32_t n_query, const int32_t *index,
                               const double *priors, int32_t n_theta, double step_rad, int32_t kx, int32_t ky, double *pose_out,
                               int32_t *info_out, uint32_t *scores_out);
int32_t roam_time_map_match(roam_ctx *ctx, roam_map_field *field, const uint32_t *hits, const uint32_t *views, int32_t min_hits,
                            int32_t min_views, int32_t radius, const uint8_t *table, int32_t n_query, const double *xy,
                            const int64_t *offsets, const double *priors, int32_t n_theta, double step_rad, int32_t kx, int32_t ky,
                            int32_t reps, float *ms /* 2 */);

/* ---- engine: B resident lanes, one scan pair per lane per step ---------------------------
 * Replaces the body of the RawROAMSystem.run loop (RawROAMSystem.py:162-298) minus plotting:
 * a1/a2 ingest+peaks, a3 warp+quantise, pyramid, a7 KLT against the lane's previous
 * pyramid, status &= err<10, a8 outlier rejection, a10 Kabsch, a15 glue, a11-a14 LM,
 * keyframe bookkeeping (Mapping.py:37-66,118-125,149-174). */
typedef struct roam_engine_cfg {
    int32_t lanes;            /* B                                                       */
    int32_t rows;             /* 400; 2 ... 1020 (ROAM_E_ARG outside: the warp's zero-weight tap row rows + 1 wraps to row 1) */
    int32_t stride;           /* 3779 bytes per record row                                */
    int32_t payload_off;      /* 11                                                       */
    int32_t clip;             /* 2025                                                     */
    int32_t pool_scans;       /* number of raw records kept resident in HBM               */
    int32_t peaks_cap;        /* per-lane capacity of the peak list                       */
    int32_t reject_outliers;  /* paramFlags["rejectOutliers"] (Tracker.py:93)             */
    int32_t motion_distortion;/* 1: LM pose (RawROAMSystem.py:208-237); 0: Kabsch dead reckoning (:236,301-317) */
    int64_t clique_node_limit;/* roam_reject_outliers' node_limit for every lane (0 = default): a lane short of nodes takes
                                 the unproven mask - possibly empty - as its inliers, bit0 of its flags clear */
    double sigma5[5];
    int32_t retrack_on_device;/* 1: lanes that run out of features (<= 60 inliers, RawROAMSystem.py:250-271) re-detect
                                 (appendNewFeatures: DoH blobs + ANMS, getFeatures.py:74-118) inside roam_engine_step */
    int32_t retrack_slots;    /* lanes whose detection scratch (33 MB each) is resident at once; 0 = min(lanes, 2048) */
    /* Map.isGoodKeyframe (Mapping.py:149-174): a keyframe is added when the pose moved this far from the last one.  <= 0: the
     * reference's constants, TRANS_THRESHOLD = 2.0 m and ROT_THRESHOLD = 0.2 rad (Mapping.py:13-15).  (The pictures the reference keeps
     * of its data/tiny run were made with a keyframe on EVERY frame - DESIGN.md section 4; 1e-9 reproduces that.) */
    double keyframe_trans_m;
    double keyframe_rot_rad;
} roam_engine_cfg;

typedef struct roam_lane_result {
    double pose[3];           /* latest pose [x,y,th]                                    */
    double velocity[3];
    double kabsch_R[4];
    double kabsch_h[2];       /* metres                                                   */
    int32_t n_tracked;        /* K fed to KLT                                             */
    int32_t n_good;           /* after status & err<10                                    */
    int32_t n_inliers;        /* after outlier rejection                                  */
    int32_t n_peaks;          /* polar peaks of the current scan                          */
    int32_t lm_nfev;
    int32_t lm_info;
    int32_t flags;            /* bit0 clique proven, bit1 keyframe added, bit2 retrack wanted (features ran out),
                                 bit3 retrack done on the device in this step; bits 8..11 detection overflows
                                 (candidates > 2048, k-d tree, pairs > 32767, features > 1024): never set on real scans */
    int32_t n_after_retrack;  /* feature count after the device-side append (bit3), else 0 */
} roam_lane_result;

int32_t roam_engine_create(roam_ctx *ctx, const roam_engine_cfg *cfg);
int32_t roam_engine_destroy(roam_ctx *ctx);
/* copy one raw record (rows x stride u8) into pool slot idx */
int32_t roam_engine_upload_scan(roam_ctx *ctx, int32_t pool_idx, const uint8_t *rec);
/* raw-record ingest (reference parseData.py:160-226 loads one PNG per frame; here n records of rows x stride u8,
 * `host_stride` bytes apart in PINNED host memory, are copied to pool slots pool_idx0.. (only the payload_off + clip
 * bytes of every row that the path reads cross PCIe) on a copy stream that
 * overlaps the compute stream).  roam_engine_step waits for the uploads that wrote the pool slots IT reads (the newest of them; not for
 * uploads of other slots enqueued meanwhile - those may themselves be waiting, behind a fence, for earlier steps);
 * roam_engine_fence makes later uploads wait for the steps enqueued so far (double-buffered pools). */
/* host_records must be pinned / registered host memory (the copy kernel reads it from the GPU): a pageable pointer is refused
 * with ROAM_E_ARG */
int32_t roam_engine_upload_scans_async(roam_ctx *ctx, int32_t pool_idx0, int32_t n, const uint8_t *host_records, int64_t host_stride);
int32_t roam_engine_fence(roam_ctx *ctx);
/* device-to-device copy of a resident record (lets a benchmark give every lane its own copy of a
 * scan so that input reads are real HBM traffic rather than L2 / Infinity-Cache hits) */
int32_t roam_engine_copy_scan(roam_ctx *ctx, int32_t dst_idx, int32_t src_idx);
/* initialise a lane from a pool scan: pyramid of that scan becomes "previous", features =
 * pts (K,2) f32 pixel [x,y], pose = pose3.  (First-frame feature detection is a4/a5.) */
int32_t roam_engine_init_lane(roam_ctx *ctx, int32_t lane, int32_t pool_idx, const float *pts,
                              int32_t K, const double *pose3);
/* advance every lane by one scan pair: lane i consumes pool scan scan_idx[i] as its current
 * scan.  Asynchronous: the call only enqueues work (scan_idx is copied before it returns).  Steps
 * enqueued back to back are pipelined on the device - peaks / warp of step N+2, the pyramid of step
 * N+1 and the tracking + pose solve of step N run concurrently - with results identical to
 * synchronised execution; roam_engine_results and the other blocking accessors return the state
 * after the LAST enqueued step.  The host may run at most three steps ahead of the device. */
int32_t roam_engine_step(roam_ctx *ctx, const int32_t *scan_idx);
/* Motion prior of the NEXT roam_engine_step only (consumed by that step, then gone): affine (lanes, 6) f32, row-major
 * [a00 a01 a02 a10 a11 a12] per lane - the predicted position in the lane's current full-size Cartesian image, in pixels, of a
 * feature at p = (x, y) in the previous one: (a00 x + a01 y) + a02, (a10 x + a11 y) + a12, evaluated on the device in float32 with every
 * operation rounded.  The lane's tracker starts its search there (roam_klt_track_*_flow's rule) instead of at p.  use (lanes) u8,
 * may be NULL = every lane: lanes with use[i] == 0 run unseeded, bit for bit.  affine == NULL withdraws a prior that no step has
 * consumed yet.  A lane that starts a new sequence on that step has no features and ignores its prior.  The call does not touch the
 * device: the values are staged in pinned memory of the engine (a ring of four slots; a slot is reused only after the tracker
 * of the step that read it has finished, which the step pipeline's own three-step limit already guarantees) and roam_engine_step
 * copies them asynchronously on the compute stream, ahead of its tracker.  ROAM_E_ARG: an entry that is not finite, a linear
 * coefficient (a00 a01 a10 a11) above ROAM_PRIOR_MAX_LINEAR in magnitude, a translation (a02 a12) above ROAM_KLT_MAX_GUESS px - with
 * features inside a 16384 px image the start then stays below 2^22 px.  ROAM_E_STATE: no engine. */
#define ROAM_PRIOR_MAX_LINEAR 64.0f
int32_t roam_engine_set_motion_prior(roam_ctx *ctx, const float *affine, const uint8_t *use);
/* The motion prior as a mode of the engine: while it is on, every roam_engine_step registers each lane's previous scan against its
 * current one (roam_engine_fmt_register's pass, FMT.py:211-250, 134-168, 13-33, on the raw pool records) and hands the affine of
 * FMT.flowPriorFromFMT to the lane's tracker, all on the device: the pass is enqueued on a stream of its own beside the warp of its
 * step, the tracker waits for it, and no call synchronises the host.  Pair i of a step is (the scan lane i consumed in its previous
 * step, scan_idx[i]); a lane without a previous step or with ROAM_STEP_NEW_SEQUENCE is not registered and runs unseeded.
 * clip_px, downsample, cart_downsample: as roam_engine_fmt_register (0, 0, 0 = 1012, 10, 20).  min_rot_response, min_trans_response:
 * a lane whose rotation or translation correlation answers below its minimum runs unseeded, bit for bit; 0 = no gate.  A lane also
 * runs unseeded when a number of its registration is not finite or its affine is beyond roam_engine_set_motion_prior's limits.
 * roam_engine_set_auto_prior is the only blocking part: it waits for the enqueued steps, allocates the pass's buffers (one device
 * allocation, sized for chunks of floor(2000 MiB / bytes per pair) pairs, at most `lanes`; ROAM_FMT_BATCH_CHUNK in the environment
 * is read here, once, and caps the chunk), uploads the host tables and makes the FFT's twiddle tables.  cfg == NULL switches the mode
 * off and frees everything.  ROAM_E_ARG, before any device call: whatever roam_engine_fmt_register refuses, a minimum that is
 * negative or not finite.  ROAM_E_HIP: the memory cannot be had; the mode stays off.
 * A prior set with roam_engine_set_motion_prior still belongs to the next step only and wins for that whole step: no registration
 * is enqueued for it.
 * The previous record must still be in its pool slot: the engine counts the writes to every slot (roam_engine_upload_scan,
 * _upload_scans_async, _copy_scan) and remembers the count of the slot each lane consumed.  A step that finds the previous slot of a
 * lane written since returns ROAM_E_STATE (the message names lane and slot) before it enqueues anything.  It is said once: the lane's
 * next step trusts the slot, so the caller restores the record and steps again. */
typedef struct roam_auto_prior_cfg {
    int32_t clip_px, downsample, cart_downsample;   /* as roam_engine_fmt_register; 0, 0, 0 = 1012 / 10 / 20 clipped to cfg.clip */
    double min_rot_response, min_trans_response;    /* lanes below either run unseeded; 0 = no gate */
} roam_auto_prior_cfg;
int32_t roam_engine_set_auto_prior(roam_ctx *ctx, const roam_auto_prior_cfg *cfg);   /* NULL: off */
/* the prior of step `step` (0-based, as roam_engine_step_results, which it waits like: for that step only; ROAM_E_STATE once the step
 * has left the ring of 8, or if the mode was off when the step was enqueued or has been switched off since).  Row i of n <= lanes:
 * out6 {angle_rad, scale, rot_response, dx, dy, trans_response} in roam_engine_fmt_register's column order (the scale is made on the
 * host from the record's raw shift, with the blocking pass's expression), NaN for a lane that was not registered; affine (n, 6) f32,
 * the prior the lane's tracker was offered; source (n) u8: 0 = unseeded, 1 = in-step registration, 2 = the caller's
 * roam_engine_set_motion_prior.  Any of the three may be NULL. */
int32_t roam_engine_step_prior(roam_ctx *ctx, int64_t step, double *out6, float *affine, uint8_t *source, int32_t n);
/* scan_idx[i] | ROAM_STEP_NEW_SEQUENCE: lane i starts a NEW sequence on this scan - its features are dropped before the pair,
 * nothing is tracked, the pose stays, and the first-frame detection (appendNewFeatures(prevImgCart, empty),
 * RawROAMSystem.py:150) runs on this scan inside the step (needs cfg.retrack_on_device).  A stream of finite sequences
 * per lane without any host synchronisation between them. */
#define ROAM_STEP_NEW_SEQUENCE 0x40000000
/* blocking: fetch the per-lane results of the last step */
int32_t roam_engine_results(roam_ctx *ctx, roam_lane_result *out, int32_t n);
/* per-step results without draining the pipeline: every step's records are copied to pinned host memory right behind the step
 * on the compute stream (ring of the last 8 steps); this call waits for step `step` only (0-based count of roam_engine_step calls) - poses and
 * flags of step N can be consumed while steps N+1.. are still running.  ROAM_E_STATE if the step left the ring. */
int32_t roam_engine_step_results(roam_ctx *ctx, int64_t step, roam_lane_result *out, int32_t n);
int32_t roam_engine_steps_enqueued(roam_ctx *ctx, int64_t *nstep);
/* device-side retrack of the following steps: 0 = suspended (flags are still raised), 1 = lanes that ran out of features
 * (default), 2 = every lane in every step (measurement of the detection cost) */
int32_t roam_engine_set_retrack(roam_ctx *ctx, int32_t mode);
/* like roam_engine_init_lane, but the initial features are DETECTED on the device from the pool scan
 * (appendNewFeatures(prevImgCart, empty), RawROAMSystem.py:150); needs cfg.retrack_on_device */
int32_t roam_engine_init_lane_detect(roam_ctx *ctx, int32_t lane, int32_t pool_idx, const double *pose3);
/* the same for the n lanes lane0 .. lane0 + n - 1 in one pass (pool_idx[n], poses3[n][3]): one warp / pyramid launch and one
 * detection pass over all of them instead of n single-lane passes */
int32_t roam_engine_init_lanes_detect(roam_ctx *ctx, int32_t lane0, int32_t n, const int32_t *pool_idx, const double *poses3);
/* blocking: current feature set of a lane (cap rows), and its peak list */
int32_t roam_engine_lane_features(roam_ctx *ctx, int32_t lane, float *pts, int32_t cap, int32_t *K);
int32_t roam_engine_lane_peaks(roam_ctx *ctx, int32_t lane, int32_t *out, int64_t cap, int64_t *n);
/* a4 on a resident scan: DoH maxima of the float32 Cartesian warp of pool scan `pool_idx`
 * (appendNewFeatures(currImgCart, ...) of RawROAMSystem.py:264 without moving image data) */
int32_t roam_engine_doh_maxima(roam_ctx *ctx, int32_t pool_idx, const double *sigmas, int32_t num_sigma, double threshold,
                               int32_t *out_rcs, double *out_val, int32_t cap, int32_t *n_out);
/* the Fourier-Mellin rotation prior of Tracker.track (Tracker.py:62-63) on resident scans: roam_fmt_rotation_batch_f32's pass for the
 * n pairs of pool records (prev_pool_idx[i], curr_pool_idx[i]), read in place as float(u8) / 255.0f (no float32 polar image is
 * made).  Blocking: waits for the steps enqueued so far and for the uploads of the pool, and leaves the engine's state alone.
 * The range clip is min(clip_px, cfg.clip), clip_px <= 0: cfg.clip.  out3 (n, 3) f64 {angle_rad, scale, response}.
 * ROAM_E_ARG: null pointers, n < 1, a pool index out of range, cfg.rows < 8, downsample < 1, R = clip / downsample outside
 * [ROAM_FMT_MIN_R, ROAM_FMT_MAX_R]. */
int32_t roam_engine_fmt_rotation(roam_ctx *ctx, int32_t n, const int32_t *prev_pool_idx, const int32_t *curr_pool_idx, int32_t clip_px,
                                 int32_t downsample, double *out3);
/* roam_fmt_register_batch_f32's pass (FMT.py:211-250, 134-168, 13-33) for the n pairs of pool records (prev_pool_idx[i],
 * curr_pool_idx[i]), read in place as float(u8) / 255.0f by both halves.  Blocking and read-only like roam_engine_fmt_rotation.  The
 * rotation half clips at min(clip_px, cfg.clip); the Cartesian half reads the record's full clipped width, Rc = cfg.clip /
 * cart_downsample.  out6 (n, 6) f64 {angle_rad, scale, rot_response, dx, dy, trans_response}.  ROAM_E_ARG: whatever
 * roam_engine_fmt_rotation refuses, cart_downsample < 1, 2Rc outside [2, 4096]. */
int32_t roam_engine_fmt_register(roam_ctx *ctx, int32_t n, const int32_t *prev_pool_idx, const int32_t *curr_pool_idx, int32_t clip_px,
                                 int32_t downsample, int32_t cart_downsample, double *out6);
/* blocking: level `level` (0..3) of the lane's most recent Cartesian u8 pyramid (w*h bytes, row-major) */
int32_t roam_engine_lane_image(roam_ctx *ctx, int32_t lane, int32_t level, uint8_t *out, int64_t cap);
/* replace a lane's feature set (retrack append, getFeatures.appendNewFeatures getFeatures.py:98-118) */
int32_t roam_engine_set_features(roam_ctx *ctx, int32_t lane, const float *pts, int32_t K);

/* ---- device-resident keyframe map (reference Mapping.Map.keyframes / addKeyframe,
 * Mapping.py:118-147; keyframes are created at RawROAMSystem.py:186-190 and :250-270).
 * Every keyframe of a lane stays in HBM.  The LIVE keyframe is the one the tracker prunes each frame
 * (Keyframe.pruneFeaturePoints, Mapping.py:118-125); when it is replaced - inside roam_engine_step when
 * the pose moved >= 0.2 rad / 2 m or the features ran out, or by roam_engine_set_features - its final
 * state {pose, velocity at creation, undistorted pruned locals, pool scan it was created on} is copied
 * device-to-device into the lane's ring.  Index 0 is the oldest keyframe, count-1 the live one.
 * A full ring drops further keyframes (count stays at keyframes_per_lane + 1). */
int32_t roam_engine_map_reserve(roam_ctx *ctx, int32_t keyframes_per_lane);
int32_t roam_engine_map_count(roam_ctx *ctx, int32_t lane, int32_t *count);
/* blocking read-back of one keyframe: locals_xy receives n (x, y) pairs in metres (prunedUndistortedLocals) */
int32_t roam_engine_map_get(roam_ctx *ctx, int32_t lane, int32_t index, double *pose3, double *vel3, double *locals_xy,
                            int32_t cap_pts, int32_t *n_out, int32_t *scan_out);
/* per-stage device time of the last step in milliseconds (hipEvent pairs on the stream);
 * names_out receives n pointers to static strings. */
int32_t roam_engine_stage_times(roam_ctx *ctx, float *ms_out, const char **names_out, int32_t cap,
                                int32_t *n);
/* the timestamp events behind roam_engine_stage_times and the "doh_*" figures of roam_engine_kernel_avg / _kernel_chunk_ms: recorded by
 * default (on = 1).  Thirteen timestamp packets in the back end's chain of dependent launches are nothing in a batch step and ~50 us of a
 * single-sequence pair (1 600 -> 1 740 scan-pairs/s without motion distortion): the streaming driver switches them off (on = 0), after which
 * those calls return ROAM_E_STATE.  ROAM_STAGE_EVENTS=0 / 1 in the environment of roam_engine_create overrides this call. */
int32_t roam_engine_set_stage_events(roam_ctx *ctx, int32_t on);
/* average in-step launch time (ms) of a front-end kernel ("ingest_peaks" | "warp_quantise" | "pyramid") over the
 * last `last_steps` steps (<= 64), from HIP event pairs recorded on the stream the kernel runs on; no
 * synchronisation happens inside the steps themselves.  "doh_integral" | "doh_det_maxima" (engines with
 * retrack_on_device): the image-scale kernels of the FIRST detection chunk of each of those steps, i.e. of
 * min(retrack_slots, lanes that re-detected in the step) detections; n_used counts the steps that had device-side
 * detection switched on */
int32_t roam_engine_kernel_avg(roam_ctx *ctx, const char *name, int32_t last_steps, float *avg_ms, int32_t *n_used);
/* "doh_integral" | "doh_det_maxima", chunk by chunk: ms_out[s * *chunks + c] = launch duration of chunk c in the s-th of the last
 * *steps_out (<= last_steps, <= 64) steps, oldest first; -1 for a step without device-side detection.  A step launches
 * ceil(lanes / retrack_slots) chunks (the first 16 are traced) whatever the number n of lanes that re-detect - only the device
 * knows it; chunk c holds clamp(n - c * retrack_slots, 0, retrack_slots) detections, n is in the step's result records.
 * cap (floats) >= last_steps * 16 always suffices.  "doh_integral": a chunk of fewer than 200 detections ran the two-pass kernels
 * (three times the one-sweep kernel's traffic; both forms are launched, the one whose regime it is not returns at once) - leave such
 * chunks out of a roofline average, as bench.py does */
int32_t roam_engine_kernel_chunk_ms(roam_ctx *ctx, const char *name, int32_t last_steps, float *ms_out, int32_t cap, int32_t *chunks,
                                    int32_t *steps_out);
/* detections per launch ("chunk") of a detection kernel inside a step: retrack_slots - or 1 024 when an engine of >= 2 048 lanes and
 * slots runs the determinants of a chunk on a second stream beside the next chunk's integral images (the default there; ROAM_DET_SIDE=0
 * in the environment of roam_engine_create: off).  The chunks of roam_engine_kernel_chunk_ms are these */
int32_t roam_engine_detect_chunk(roam_ctx *ctx, int32_t *chunk);
/* time `reps` launches of the dominant streaming kernel (warp+quantise of all lanes) with
 * HIP events on the context stream; returns average ms per launch. */
int32_t roam_engine_time_kernel(roam_ctx *ctx, const char *name, int32_t reps, float *avg_ms,
                                double *algo_bytes_per_launch);
/* diagnostics of the device-side detector (getFeatures.py:39-51: integral image -> Hessian determinants -> 3 x 3 x 3 maxima): runs the
 * image-scale kernels for n_slots detections (scratch slot i = the scan lane i % lanes stepped last) as two kernels (fused = 0: image in HBM)
 * or as the fused kernel (fused = 1: image never leaves the CU) and returns, per slot, the candidate count and the first cap_per_slot
 * candidates in (row, column, layer) order (rc = row << 16 | column << 2 | layer, val = determinant); S_out (optional, W x W float64) =
 * the integral image of slot s_slot as that form computed it.  Needs retrack_on_device and one step; n_slots <= retrack_slots, lanes. */
int32_t roam_engine_debug_detect(roam_ctx *ctx, int32_t fused, int32_t n_slots, int32_t cap_per_slot, uint32_t *rc_out, double *val_out,
                                 int32_t *n_out, int32_t s_slot, double *S_out);
/* test: the detector's blob bookkeeping alone (candidate order, skimage's _prune_blobs in its pair order, the sigma argsort of NumPy
 * 1.22, SSC) on the caller's candidate lists, through the engine's own scratch and the one launch call a step makes, so that P picks the
 * launch form (one kernel below 256 problems, three classes of kernels from 256, longest list first from 512).  P <= lanes problems;
 * cand_rc / cand_val (host): P x rows_given, rows_given <= 2048; rc = row << 16 | col << 2 | layer with row, col < the Cartesian size W,
 * layer 1 | 2 and distinct keys, in any order; cand_n[p] = the count a detection would have left, > rows_given only beyond 2048 (with
 * rows_given = 2048: RT_F_CAND_OVERFLOW).  Bad arguments are refused (ROAM_E_ARG) before any device call.  Out, per problem: kp_n, kp
 * (2048 x 3 float64 [row, col, sigma] in adaptiveNMS priority order), the flags (1 candidate, 2 tree / task, 4 pair overflow), sel_n
 * and sel (2048 indices into kp); what a kernel left alone holds 0xff bytes (kp: NaN) or 0x7f bytes (the int32 arrays).  Needs
 * retrack_on_device; leaves the scratch as a detection expects it.  pairs_out (optional, P x 32768): the candidate pairs i << 16 | j
 * (i < j: indices in response order) in the order query_pairs emits them, from entry 0 on; the caller knows their number (at most
 * 32767 are kept); not meaningful after a tree / task overflow. */
int32_t roam_engine_debug_blobs(roam_ctx *ctx, int32_t P, int32_t rows_given, const uint32_t *cand_rc, const double *cand_val,
                                const int32_t *cand_n, int32_t *kp_n_out, double *kp_out, int32_t *flags_out, int32_t *sel_n_out,
                                int32_t *sel_out, uint32_t *pairs_out);

/* ---- multi-GPU.  One process per GPU, sequences sharded by rank, no data-path collective.  The only exchange
 * of the path is handing a keyframe to a global map (reference Mapping.Map.addKeyframe, Mapping.py:118-147; BASELINE
 * config 5): the owning rank broadcasts the DEVICE-RESIDENT keyframe of one lane with ncclBroadcast (RCCL over xGMI).
 * RCCL is bound at run time (librccl.so); without it these calls return ROAM_E_STATE.
 * Rendezvous is the caller's business: rank 0 obtains the id, ships the 128 bytes to the other ranks by any means
 * (bench.py: a file), then every rank calls roam_comm_init collectively. */
#define ROAM_COMM_ID_BYTES 128
/* 1 if librccl.so can be bound in this process (nothing is initialised): lets the ranks agree on a fallback BEFORE any of them
 * enters the collective roam_comm_init */
int32_t roam_comm_available(void);
int32_t roam_comm_unique_id(uint8_t *id_out /* [ROAM_COMM_ID_BYTES] */);
int32_t roam_comm_init(roam_ctx *ctx, const uint8_t *id, int32_t rank, int32_t world);
int32_t roam_comm_destroy(roam_ctx *ctx);
/* rank / size as RCCL reports them (ncclCommUserRank / ncclCommCount) */
int32_t roam_comm_info(roam_ctx *ctx, int32_t *rank, int32_t *world);
/* blocking in-place all-reduce of n <= 8 doubles, op 0 = max, 1 = sum (max-over-ranks wall time); barrier = sum of ones */
int32_t roam_comm_allreduce_f64(roam_ctx *ctx, double *inout, int32_t n, int32_t op);
int32_t roam_comm_barrier(roam_ctx *ctx);

typedef struct roam_keyframe_hdr {
    double pose[3];           /* keyframe pose [x,y,th]                                   */
    double velocity[3];       /* velocity the keyframe's points were undistorted with      */
    int32_t n_features;       /* rows of locals_xy (prunedUndistortedLocals, metres)       */
    int32_t n_peaks;          /* rows of the polar point cloud [azimuthIdx, rangeIdx]      */
    int32_t scan;             /* pool scan the keyframe was created on                     */
    int32_t lane;             /* lane of the root rank it belongs to                       */
} roam_keyframe_hdr;

/* collective: every rank of the communicator calls it with the same root and lane.  The root packs the LIVE keyframe of
 * its lane `lane` {pose, velocity, prunedUndistortedLocals, latest polar peaks} on the device, all ranks receive it in a
 * device buffer (two ncclBroadcast calls: header + features, then the peak list), then copy it to the caller's arrays:
 * locals_xy (cap_pts, 2) f64, peaks (peaks_cap, 2) i32.  Either array may be NULL (its part is then not copied out). */
int32_t roam_bcast_keyframe(roam_ctx *ctx, int32_t root, int32_t lane, roam_keyframe_hdr *hdr_out, double *locals_xy,
                            int32_t cap_pts, int32_t *peaks, int64_t peaks_cap);

/* BASELINE config 5 as a loop (reference RawROAMSystem.py:250-262 + Mapping.Map.addKeyframe, Mapping.py:176-180: "after each
 * keyframe the owning GPU broadcasts"): collective and NON-BLOCKING, called by every rank once after each roam_engine_step with
 * its own lane.  Which rank has a new keyframe in a given step is only known on that rank's device, so the schedule is fixed: every
 * rank contributes ONE fixed-size record per step - its lane's new keyframe {header, prunedUndistortedLocals, up to 32768 polar
 * peaks} if the step made one (result flag bit 1), an empty record otherwise - to one ncclAllGather on the engine's exchange
 * stream, and appends every non-empty record it receives to its remote map on the device, in rank order.  Nothing waits on the host
 * and the step pipeline is not drained; roam_remote_map_count / _get wait for the exchange stream.  Needs roam_comm_init and
 * roam_remote_map_reserve; do not mix with roam_bcast_keyframe on one engine. */
int32_t roam_keyframe_exchange(roam_ctx *ctx, int32_t lane);

/* The consumer of that broadcast: Map.addKeyframe (Mapping.py:118-147) on EVERY rank.  After roam_remote_map_reserve(n) each
 * roam_bcast_keyframe also appends the received payload {header, prunedUndistortedLocals, polar peaks} device-to-device to a
 * ring of n keyframes in this rank's HBM (the oldest is overwritten); the sending rank included, so all ranks hold the same
 * global map.  count: keyframes received so far / resident now; get: index 0 = the oldest resident one. */
int32_t roam_remote_map_reserve(roam_ctx *ctx, int32_t keyframes);
/* test / debug: the receive half of roam_keyframe_exchange on ONE GPU, without a communicator.  recv (host) = `world` records as the
 * all-gather of a `world`-rank job leaves them in a rank's receive buffer (record r = rank r's; *rec_bytes apart; roam_keyframe_hdr at
 * 0, n_features x 2 float64 at *locals_off, n_peaks x 2 int32 at *peaks_off; n_features < 0 = "no keyframe in this step").  The records
 * go through the kernel the exchange runs (Map.addKeyframe in rank order, Mapping.py:176-180) into this context's remote map: read it
 * back with roam_remote_map_count / _get.  recv == NULL: only the layout is returned.  Needs roam_remote_map_reserve(>= world). */
int32_t roam_debug_keyframe_append(roam_ctx *ctx, const uint8_t *recv, int32_t world, int64_t *rec_bytes, int32_t *locals_off,
                                   int32_t *peaks_off, int32_t *max_peaks);
/* test / measurement: the 2-D FFT alone.  roam_debug_fft2_f64: rows x cols float64 planes (host; im_in may be NULL), both sizes
 * 2^a 3^b 5^c in [1, 4096]; inverse != 0: the unscaled inverse.  roam_time_fft2: average milliseconds (HIP events, two warm runs
 * first) of `what` on zero planes of that size (sizes from 2). */
int32_t roam_debug_fft2_f64(roam_ctx *ctx, const double *re_in, const double *im_in, int32_t rows, int32_t cols, int32_t inverse,
                            double *re_out, double *im_out);
/* test: the engine's batched SSC kernel alone (the stage call roam_ssc runs the same body with a 64 KB cell bitmap, this one with
 * 16 KB).  kp (host): P problems as the engine lays them out, kp_cap rows of 3 float64 [row, col, sigma] each; count[p] live rows
 * (clamped to kp_cap by the kernel); problems p with first + p >= n_active are skipped.  One launch with (num_ret, tol, cols, rows,
 * first).  sel_out (P x kp_cap) and n_sel_out (P) are prefilled with -1 on the device before the launch. */
int32_t roam_debug_ssc_batch(roam_ctx *ctx, const double *kp, const int32_t *count, int32_t P, int32_t kp_cap, int32_t n_active,
                             int32_t first, int32_t num_ret, double tol, int32_t cols, int32_t rows, int32_t *sel_out,
                             int32_t *n_sel_out);
/* test: the motion-distortion solve as the engine launches it.  B problems in the engine's layout: T_wj0 / T_wj_init (B x 9), p_w /
 * p_jt (B x nstride x 2), count[b] live points (clamped to nmax by the kernels; fewer than 2: info -1, nfev 0, a zero solution), nmax
 * <= nstride the host-side bound that picks the kernels.  use_big != 0: with the list through which the one-wavefront kernel leaves
 * its large problems to the workgroup kernel (two slots, zeroed here).  The solve is launched `repeat` (1..8) times in a row on the
 * context's stream, the list's slot alternating as in roam_engine_step.  out6 (repeat x B x 6), nfev and info (repeat x B) are
 * prefilled with 0xff bytes on the device.  big_out (optional, 2 x (1 + B)): the list's two slots [n, ids...] after the last solve
 * (zeros without the list). */
int32_t roam_debug_mds_solve_batch(roam_ctx *ctx, const double *T_wj0, const double *p_w, const double *p_jt, const int32_t *count,
                                   int32_t B, int32_t nstride, int32_t nmax, const double *T_wj_init, const double *sigma5,
                                   double period, int32_t use_big, int32_t repeat, double *out6, int32_t *nfev, int32_t *info,
                                   int32_t *big_out);
/* test: More's lmpar alone, as each of the two solve kernels carries it.  n = 6; R (6 x 6 row-major, upper triangle read), ipvt (6),
 * qtb (6), diag = 1, trust radius delta > 0, incoming par_in >= 0.  form 0: the workgroup kernel's copy on one thread -> par_out[1],
 * x_out[6], sdiag_out[6].  form 1: the one-wavefront kernel's copy, every lane computing alike; lanes 0 and 63 both store ->
 * par_out[2], x_out[12], sdiag_out[12].  sdiag is 0 where lmpar accepts the Gauss-Newton step (par = 0). */
int32_t roam_debug_lm_lmpar(roam_ctx *ctx, int32_t n, const double *R, const int32_t *ipvt, const double *qtb, double delta,
                            double par_in, int32_t form, double *par_out, double *x_out, double *sdiag_out);
#define ROAM_TIME_FFT_FIVE      0   /* the five 2-D transforms of one phase correlation (two real forward, one inverse), transposes included */
#define ROAM_TIME_DFT_FIVE      1   /* the same five as direct DFTs, a baseline only (rows * cols <= 131072) */
#define ROAM_TIME_FFT_ROWS      2   /* one row pass: `rows` transforms of length cols, in place */
#define ROAM_TIME_FFT_TRANSPOSE 3   /* one transpose rows x cols -> cols x rows */
#define ROAM_TIME_FFT_COLS      4   /* one column pass on the transposed plane: `cols` transforms of length rows, in place */
int32_t roam_time_fft2(roam_ctx *ctx, int32_t rows, int32_t cols, int32_t what, int32_t reps, float *ms_per_rep);
int32_t roam_remote_map_count(roam_ctx *ctx, int64_t *received, int32_t *resident);
int32_t roam_remote_map_get(roam_ctx *ctx, int32_t index, roam_keyframe_hdr *hdr_out, int32_t *root_out, double *locals_xy,
                            int32_t cap_pts, int32_t *peaks, int64_t peaks_cap);

#ifdef __cplusplus
}
#endif
#endif /* ROAM_ABI_H */
