// Adaptive non-maximal suppression, "suppression via square covering" (a5).
//
// Replaces ANMS.ssc (reference ANMS.py:5-102): binary search over the square width; per
// width a greedy pass over the keypoints in priority order.  One wavefront per call: the
// 64 lanes test 64 consecutive keypoints against the covered-cell bitmap (LDS) with one
// load each, conflicts inside the chunk are resolved in priority order with ballots and
// lane broadcasts (wave-uniform loop over the surviving lanes), accepted lanes cover their
// 5x5 cell block with LDS atomic ORs.  When the grid would not fit the LDS bitmap (very
// small widths, i.e. B < ~400) the equivalent pairwise test against the accepted list is
// used (see oracle/c/ssc.c for the equivalence argument).  Binary-search arithmetic is
// float64 and identical to the reference (Python round == rint, half-to-even).
#include "roam_internal.h"

#include "ssc_body.inc"

__global__ __launch_bounds__(64) void ssc_kernel(const double *__restrict__ kp, int B, int num_ret, double tol,
                                                 int cols, int rows, int32_t *__restrict__ work,
                                                 int32_t *__restrict__ sel, int32_t *__restrict__ n_sel)
{
    extern __shared__ uint32_t bitmap[];
    ssc_body(kp, B, num_ret, tol, cols, rows, work, sel, n_sel, bitmap, SSC_BITMAP_BYTES);
}

// batched: problem p = blockIdx.x (skipped when first + p >= *n_active): kp + p * kp_stride (rows of 3 doubles), count[p]
// keypoints, work + p * 4 * kp_cap, sel + p * kp_cap
__global__ __launch_bounds__(64) void ssc_batch_kernel(const double *__restrict__ kp, int64_t kp_stride, const int32_t *__restrict__ count,
                                                       int kp_cap, int num_ret, double tol, int cols, int rows,
                                                       int32_t *__restrict__ work, int32_t *__restrict__ sel,
                                                       int32_t *__restrict__ n_sel, const int32_t *__restrict__ n_active, int first)
{
    extern __shared__ uint32_t bitmap[];
    const int p = blockIdx.x;
    if (first + p >= *n_active) return;
    const int B = min(count[p], kp_cap);
    if (B <= 0) { if (threadIdx.x == 0) n_sel[p] = 0; return; }
    ssc_body(kp + (int64_t)p * kp_stride, B, num_ret, tol, cols, rows, work + (int64_t)p * 4 * kp_cap, sel + (int64_t)p * kp_cap,
             n_sel + p, bitmap, SSC_BATCH_BITMAP_BYTES);
}

hipError_t launch_ssc_batch(hipStream_t st, const double *kp, int64_t kp_stride, const int32_t *count, int kp_cap, int P,
                            int num_ret, double tol, int cols, int rows, int32_t *work, int32_t *sel, int32_t *n_sel,
                            const int32_t *n_active, int first)
{
    hipLaunchKernelGGL(ssc_batch_kernel, dim3(P), dim3(64), SSC_BATCH_BITMAP_BYTES, st, kp, kp_stride, count, kp_cap, num_ret, tol, cols,
                       rows, work, sel, n_sel, n_active, first);
    return hipGetLastError();
}

hipError_t launch_ssc(hipStream_t st, const double *kp, int B, int num_ret, double tol, int cols,
                      int rows, int32_t *work, int32_t *sel, int32_t *n_sel)
{
    hipLaunchKernelGGL(ssc_kernel, dim3(1), dim3(64), SSC_BITMAP_BYTES, st, kp, B, num_ret, tol, cols, rows, work, sel, n_sel);
    return hipGetLastError();
}

extern "C" int32_t roam_ssc(roam_ctx *ctx, const double *kp, int32_t B, int32_t num_ret, double tol,
                            int32_t cols, int32_t rows, int32_t *sel_out, int32_t *n_sel)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, B >= 0 && num_ret >= 2 && cols > 0 && rows > 0 && sel_out && n_sel && (B == 0 || kp));
    if (B == 0) { *n_sel = 0; return ROAM_OK; }
    double *dkp = (double *)roam_scratch(ctx, S_IN0, sizeof(double) * 3 * (size_t)B);
    int32_t *dwork = (int32_t *)roam_scratch(ctx, S_TMP0, sizeof(int32_t) * 4 * (size_t)B);
    int32_t *dsel = (int32_t *)roam_scratch(ctx, S_OUT0, sizeof(int32_t) * ((size_t)B + 1));
    if (!dkp || !dwork || !dsel) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(dkp, kp, sizeof(double) * 3 * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch_ssc(ctx->stream, dkp, B, num_ret, tol, cols, rows, dwork, dsel + 1, dsel));
    int32_t n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&n, dsel, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(sel_out, dsel + 1, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    *n_sel = n;
    return ROAM_OK;
}

// test entry: ssc_batch_kernel alone, on P problems laid out as the engine lays them out (problem p: kp_cap rows of 3 doubles at
// kp + p * 3 * kp_cap, count[p] of them live) - one launch_ssc_batch with the caller's parameters.  sel_out (P x kp_cap) and n_sel_out (P)
// are prefilled with -1 on the device, so what the kernel left alone (a skipped problem, the rows past n_sel) stays visible.
extern "C" int32_t roam_debug_ssc_batch(roam_ctx *ctx, const double *kp, const int32_t *count, int32_t P, int32_t kp_cap, int32_t n_active,
                                        int32_t first, int32_t num_ret, double tol, int32_t cols, int32_t rows, int32_t *sel_out,
                                        int32_t *n_sel_out)
{
    if (!ctx) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ARG_CHECK(ctx, kp && count && sel_out && n_sel_out && P >= 1 && P <= 65535 && kp_cap >= 1 && (int64_t)P * kp_cap <= (1 << 24));
    ARG_CHECK(ctx, num_ret >= 2 && cols > 0 && rows > 0 && first >= 0);
    const size_t rows_all = (size_t)P * kp_cap;
    double *dkp = (double *)roam_scratch(ctx, S_IN0, sizeof(double) * 3 * rows_all);
    int32_t *dcnt = (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * ((size_t)P + 1));       // count[P], then the n_active word
    int32_t *dwork = (int32_t *)roam_scratch(ctx, S_TMP0, sizeof(int32_t) * 4 * rows_all);
    int32_t *dsel = (int32_t *)roam_scratch(ctx, S_OUT0, sizeof(int32_t) * rows_all);
    int32_t *dnsel = (int32_t *)roam_scratch(ctx, S_OUT1, sizeof(int32_t) * (size_t)P);
    if (!dkp || !dcnt || !dwork || !dsel || !dnsel) return ROAM_E_HIP;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(dkp, kp, sizeof(double) * 3 * rows_all, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dcnt, count, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dcnt + P, &n_active, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(dsel, 0xff, sizeof(int32_t) * rows_all, st));
    HIP_TRY(ctx, hipMemsetAsync(dnsel, 0xff, sizeof(int32_t) * (size_t)P, st));
    HIP_TRY(ctx, launch_ssc_batch(st, dkp, (int64_t)kp_cap * 3, dcnt, kp_cap, P, num_ret, tol, cols, rows, dwork, dsel, dnsel, dcnt + P, first));
    HIP_TRY(ctx, hipMemcpyAsync(sel_out, dsel, sizeof(int32_t) * rows_all, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(n_sel_out, dnsel, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return ROAM_OK;
}
