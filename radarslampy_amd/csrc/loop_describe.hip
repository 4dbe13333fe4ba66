// Loop-closure candidates by radar scan context (Kim et al., the MulRan data set): the descriptor.  Map of the family: loop.h.
//
// Descriptor (scan_context_kernel).  The polar scan is area-averaged to S sectors x R rings with integer bin edges
// (floor(s rows / S), floor(r clip / R)).  One workgroup per (image, sector): the 256 lanes walk the clipped row, each summing its
// columns over the sector's rows (reads coalesced along range), the column sums go to LDS, then wave w adds the columns of the rings
// w, w + 4, ... with a fixed butterfly - no atomics, one order whatever the batch.  u8 record codes are summed as integers (exact);
// float32 images in float64.  The workgroup owns a whole sector column, so it also writes what a query needs: the column divided by
// its float64 norm (zero-padded to a multiple of four rings) and a validity flag, the norm taken by sc_sector_norm - the one
// function that roam_loop_db_add_desc's kernel runs on ready-made descriptors, so that an entry's stored bits depend on its
// descriptor alone.
#include "loop.h"
#include <math.h>
#include <type_traits>

// ---------------------------------------------------------------------------------------------------------------- device
// (sc_sector_norm and sc_normalised: loop.h - the offset unit stores its variants through them too)
template <bool U8>
__global__ __launch_bounds__(SC_THREADS) void scan_context_kernel(ScSrc src, int rows, int clip, int S, int R, int Rp, double floor_v,
                                                                  int floor_code, float *__restrict__ desc, double *__restrict__ nrm,
                                                                  int32_t *__restrict__ valid)
{
    extern __shared__ __align__(16) unsigned char sc_lds[];
    typedef typename std::conditional<U8, uint32_t, double>::type ColT;
    typedef typename std::conditional<U8, unsigned long long, double>::type SumT;
    double *nv = (double *)sc_lds;                        // the norm of the sector's descriptor column
    ColT *col = (ColT *)(nv + 1);                         // clip column sums of this sector
    float *dv = (float *)(col + clip);                    // R: the descriptor column
    const int64_t z = blockIdx.x;
    const int s = blockIdx.y;
    const int y0 = (int)((int64_t)s * rows / S), y1 = (int)((int64_t)(s + 1) * rows / S);
    const int64_t img = src.index ? src.index[z] : z;
    for (int c = threadIdx.x; c < clip; c += SC_THREADS) {
        ColT a = 0;
        if constexpr (U8) {
            const uint8_t *p = (const uint8_t *)src.base + img * src.image_stride + src.payload_off + c;
            for (int y = y0; y < y1; ++y) a += (ColT)max((int)p[y * src.row_stride] - floor_code, 0);
        } else {
            const float *p = (const float *)src.base + img * src.image_stride + c;
            for (int y = y0; y < y1; ++y) a += (ColT)fmax((double)p[y * src.row_stride] - floor_v, 0.0);
        }
        col[c] = a;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < R; r += SC_THREADS / 64) {
        const int c0 = (int)((int64_t)r * clip / R), c1 = (int)((int64_t)(r + 1) * clip / R);
        SumT sum = 0;
        for (int c = c0 + lane; c < c1; c += 64) sum += (SumT)col[c];
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == 0) {
            const double cells = (double)((int64_t)(y1 - y0) * (c1 - c0));
            dv[r] = U8 ? (float)((double)sum / (255.0 * cells)) : (float)((double)sum / cells);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) nv[0] = sc_sector_norm(dv, R);
    __syncthreads();
    const double norm = nv[0];
    const int64_t row = z * S + s;
    for (int r = threadIdx.x; r < Rp; r += SC_THREADS) {
        if (r < R) desc[row * R + r] = dv[r];
        if (nrm) nrm[row * Rp + r] = r < R ? sc_normalised(dv[r], norm) : 0.0;
    }
    if (threadIdx.x == 0 && valid) valid[row] = norm > 0.0;
}

// ready-made descriptors: one lane per (entry, sector)
__global__ __launch_bounds__(SC_THREADS) void scan_context_norm_kernel(const float *__restrict__ desc, int64_t n_rows, int R, int Rp,
                                                                       double *__restrict__ nrm, int32_t *__restrict__ valid)
{
    const int64_t row = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (row >= n_rows) return;
    const float *d = desc + row * R;
    const double norm = sc_sector_norm(d, R);
    for (int r = 0; r < Rp; ++r) nrm[row * Rp + r] = r < R ? sc_normalised(d[r], norm) : 0.0;
    valid[row] = norm > 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- host
int32_t sc_check_geometry(char *err, size_t cap, int32_t rows, int32_t cols, int32_t clip_px, int32_t sectors, int32_t rings, int *clip_out)
{
    if (sectors < 2 || sectors > ROAM_SCAN_CONTEXT_MAX_SECTORS) SC_FAIL(err, cap, "scan context: sectors in [2, %d], not %d", ROAM_SCAN_CONTEXT_MAX_SECTORS, sectors);
    if (rings < 1 || rings > ROAM_SCAN_CONTEXT_MAX_RINGS) SC_FAIL(err, cap, "scan context: rings in [1, %d], not %d", ROAM_SCAN_CONTEXT_MAX_RINGS, rings);
    if (rows < sectors || rows > SC_MAX_ROWS) SC_FAIL(err, cap, "scan context: rows in [sectors = %d, %d], not %d", sectors, SC_MAX_ROWS, rows);
    if (cols < 1) SC_FAIL(err, cap, "scan context: cols >= 1, not %d", cols);
    const int clip = (clip_px > 0 && clip_px < cols) ? clip_px : cols;
    if (clip < rings || clip > ROAM_SCAN_CONTEXT_MAX_CLIP)
        SC_FAIL(err, cap, "scan context: clip_px (the range bins kept) in [rings = %d, %d], not %d", rings, ROAM_SCAN_CONTEXT_MAX_CLIP, clip);
    *clip_out = clip;
    return ROAM_OK;
}

extern "C" int32_t roam_scan_context_plan(int32_t rows, int32_t cols, int32_t clip_px, int32_t sectors, int32_t rings, int32_t *row_edges,
                                          int32_t *col_edges)
{
    int clip;
    LOOP_TRY(sc_check_geometry(nullptr, 0, rows, cols, clip_px, sectors, rings, &clip));
    for (int s = 0; s <= sectors && row_edges; ++s) row_edges[s] = (int32_t)((int64_t)s * rows / sectors);
    for (int r = 0; r <= rings && col_edges; ++r) col_edges[r] = (int32_t)((int64_t)r * clip / rings);
    return ROAM_OK;
}

static size_t sc_describe_lds(bool u8, int clip, int R) { return sizeof(double) + (size_t)clip * (u8 ? 4 : 8) + sizeof(float) * R; }

hipError_t sc_launch_describe(hipStream_t st, bool u8, const ScSrc &src, int n, int rows, int clip, int S, int R, double floor_v,
                              int floor_code, float *desc, double *nrm, int32_t *valid, int64_t first)
{
    const int Rp = (R + 3) & ~3;
    float *d = desc + first * S * R;
    double *nn = nrm ? nrm + first * S * Rp : nullptr;
    int32_t *vv = valid ? valid + first * S : nullptr;
    if (u8)
        hipLaunchKernelGGL(scan_context_kernel<true>, dim3(n, S), dim3(SC_THREADS), sc_describe_lds(true, clip, R), st, src, rows, clip, S, R, Rp,
                           floor_v, floor_code, d, nn, vv);
    else
        hipLaunchKernelGGL(scan_context_kernel<false>, dim3(n, S), dim3(SC_THREADS), sc_describe_lds(false, clip, R), st, src, rows, clip, S, R, Rp,
                           floor_v, floor_code, d, nn, vv);
    return hipGetLastError();
}

hipError_t sc_launch_norm_rows(hipStream_t st, const float *desc, int64_t n_rows, int R, int Rp, double *nrm, int32_t *valid)
{
    hipLaunchKernelGGL(scan_context_norm_kernel, dim3((unsigned)((n_rows + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, st, desc, n_rows, R,
                       Rp, nrm, valid);
    return hipGetLastError();
}

hipError_t sc_launch_norm(hipStream_t st, const roam_loop_db *db, int64_t first, int n)
{
    return sc_launch_norm_rows(st, db->desc + first * db->S * db->R, (int64_t)n * db->S, db->R, db->Rp, db->nrm + first * db->S * db->Rp,
                               db->valid + first * db->S);
}

int32_t sc_describe_host_f32(roam_ctx *ctx, const float *polar, int n, int rows, int64_t row_stride, int64_t image_stride, int clip, int S,
                             int R, double floor_v, float *desc, double *nrm, int32_t *valid, int64_t first, const roam_loop_db *cloud_db,
                             int cols, const ScOffsets *offs, const double *h_motion)
{
    const hipStream_t st = ctx->stream;
    const int width = cloud_db ? cols : clip;
    const int64_t per = (int64_t)sizeof(float) * rows * width + (cloud_db ? sc_stage_bytes(rows, cols) : 0) +
                        (offs ? sc_offset_part_bytes(false, rows, S, R, offs->n_off) : 0) + (h_motion ? sc_motion_bytes(rows) : 0);
    int64_t chunk = roam_chunk_limit(SC_CHUNK_ENV, SC_DB_BYTES) / per;
    if (chunk < 1) chunk = 1;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int nb = (int)(n - i0 < chunk ? n - i0 : chunk);
        float *d_in = (float *)roam_scratch(ctx, S_IN0, sizeof(float) * (size_t)rows * width * nb);
        if (!d_in) return ROAM_E_HIP;
        HIP_TRY(ctx, roam_upload_packed_f32(st, d_in, polar + i0 * image_stride, nb, width, rows, row_stride, image_stride));
        const ScSrc src = {d_in, (int64_t)rows * width, width, 0, nullptr};
        HIP_TRY(ctx, sc_launch_describe(st, false, src, nb, rows, clip, S, R, floor_v, 0, desc, nrm, valid, first + i0));
        if (offs) LOOP_TRY(sc_launch_offsets(ctx, false, src, nb, rows, clip, S, R, floor_v, 0, *offs, first + i0));
        if (cloud_db) {
            const PeakSrc ps = {d_in, (int64_t)rows * width, width, 0, 0, nullptr};
            LOOP_TRY(sc_build_clouds(ctx, cloud_db, ps, nb, cols, first + i0, h_motion ? h_motion + 4 * i0 * rows : nullptr));
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));           // the next chunk reuses the upload buffer
    }
    return ROAM_OK;
}

int32_t sc_check_f32_args(roam_ctx *ctx, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride, int64_t image_stride,
                          int32_t clip_px, int32_t sectors, int32_t rings, double floor, int *clip)
{
    if (!polar) { ROAM_SET_ERR(ctx, "scan context: polar is null"); return ROAM_E_ARG; }
    if (n < 1) { ROAM_SET_ERR(ctx, "scan context: n >= 1 images, not %d", n); return ROAM_E_ARG; }
    LOOP_TRY(sc_check_geometry(ctx->err, sizeof(ctx->err), rows, cols, clip_px, sectors, rings, clip));
    if (row_stride < cols) { ROAM_SET_ERR(ctx, "scan context: row_stride %lld below cols %d", (long long)row_stride, cols); return ROAM_E_ARG; }
    if (n > 1 && image_stride < (int64_t)(rows - 1) * row_stride + cols) {
        ROAM_SET_ERR(ctx, "scan context: image_stride %lld below the extent of an image", (long long)image_stride);
        return ROAM_E_ARG;
    }
    if (!(std::isfinite(floor) && floor >= 0.0)) { ROAM_SET_ERR(ctx, "scan context: floor finite and >= 0, not %g", floor); return ROAM_E_ARG; }
    return ROAM_OK;
}

extern "C" int32_t roam_scan_context_f32(roam_ctx *ctx, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride,
                                         int64_t image_stride, int32_t clip_px, int32_t sectors, int32_t rings, double floor, float *desc_out)
{
    if (!ctx) return ROAM_E_ARG;
    int clip;
    LOOP_TRY(sc_check_f32_args(ctx, polar, n, rows, cols, row_stride, image_stride, clip_px, sectors, rings, floor, &clip));
    if (!desc_out) { ROAM_SET_ERR(ctx, "scan context: desc_out is null"); return ROAM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float) * (size_t)n * sectors * rings;
    float *d_desc = (float *)roam_scratch(ctx, S_OUT0, bytes);
    if (!d_desc) return ROAM_E_HIP;
    LOOP_TRY(sc_describe_host_f32(ctx, polar, n, rows, row_stride, image_stride, clip, sectors, rings, floor, d_desc, nullptr, nullptr, 0));
    HIP_TRY(ctx, hipMemcpyAsync(desc_out, d_desc, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}
