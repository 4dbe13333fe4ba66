// The loop database's resident peak clouds: the store.  Map of the family: loop.h.
//
// Peak clouds (roam_loop_db_keep_clouds).  A database that keeps clouds stores, beside each descriptor, the scan's polar peaks in metres:
// the peaks of roam_peaks_record_u8 / roam_peaks_polar_f32 in their azimuth-major order, N of them, of which the entry keeps
// q = 0, step, 2 step, ... with step = max(point_stride, ceil(N / max_points)), as x = fl64(fl64(r res) cos_t[theta]) and y likewise
// with sin_t; the tables come from the host's libm (roam_polar_cloud_table), the device only multiplies.  The peak row kernels of
// peaks.hip leave row_stage / row_count; cloud_gather_kernel, one workgroup per scan, scans the row counts, derives step from the total
// and writes the selected peaks straight to the entry's slot - the int32 peak list is never made.  A lane owns a run of consecutive
// rows and knows the global index of their first peak from the scan, so what is stored depends on the scan alone, not on the batch or
// the chunk.
//
// Motion compensation (roam_cloud_motion_table).  A scan sweeps its azimuths over `period` seconds; with the scan's velocity
// v = (vx, vy, vtheta) in the sensor frame the peak of row t is moved to where mid-scan would have seen it: tau_t =
// period ((2 t - rows) / (2 rows)), a = vtheta tau_t, (x, y) = R(a) (x0, y0) + (vx, vy) tau_t - MotionDistortionSolver.undistort with
// the time taken from the peak's row.  The host makes the per-row table C S DX DY with its libm, cloud_gather_motion_kernel reads a
// row of it for every azimuth row a lane owns and applies it in registers before the two stores: six float64 operations per point,
// each rounded once.  A scan without a velocity has a table of NaN and takes the plain path inside the same launch; a launch without
// any table runs cloud_gather_kernel, whose code the motion form does not touch.
#include "loop.h"
#include "cloud_motion.h"
#include "peaks_common.h"
#include <math.h>

#define CG_THREADS 512                           // cloud_gather_kernel: eight waves, a row per lane up to 512 azimuths

// ---------------------------------------------------------------------------------------------------------------- device
// the stored cloud of scan b of the launch (entry first + b, the pointers already moved there) from the row kernel's staging: see the
// head of the file.  A lane takes the rows [lo, hi) and walks their peaks with the global index q = off + j.  MOTION: `motion` is the
// launch's table, rows x 4 per scan; a scan whose first value is NaN has no velocity (uniform over the workgroup)
template <bool MOTION>
__device__ __forceinline__ void cloud_gather_body(const uint16_t *__restrict__ row_stage, int stage_cap, const int32_t *__restrict__ row_count,
                                                  int rows, const double *__restrict__ trig, double res, int max_points, int point_stride,
                                                  double *__restrict__ cloud, int32_t *__restrict__ cloud_n, int32_t *__restrict__ cloud_peaks,
                                                  const double *__restrict__ motion)
{
    __shared__ int scan_sh[8];
    const int64_t b = blockIdx.x;
    const int t = threadIdx.x;
    const int ritems = (rows + CG_THREADS - 1) / CG_THREADS;
    const int lo = min(t * ritems, rows), hi = min(lo + ritems, rows);
    const int32_t *rc = row_count + b * rows;
    int c = 0;
    for (int r = lo; r < hi; ++r) c += min(rc[r], stage_cap);
    int total;
    int off = block_excl_scan(c, scan_sh, &total);
    const int fit = (total + max_points - 1) / max_points;
    const int step = fit > point_stride ? fit : point_stride;
    double *out = cloud + 2 * b * max_points;
    const double2 *mt = nullptr;
    bool moving = false;
    if constexpr (MOTION) {
        mt = (const double2 *)(motion + 4 * b * rows);
        moving = mt[0].x == mt[0].x;
    }
    for (int r = lo; r < hi; ++r) {
        const int n = min(rc[r], stage_cap);
        const uint16_t *sr = row_stage + (b * rows + r) * stage_cap;
        const double ct = trig[r], st = trig[rows + r];
        double2 cs = make_double2(1.0, 0.0), d = make_double2(0.0, 0.0);
        if constexpr (MOTION)
            if (moving && n > 0) { cs = mt[2 * r]; d = mt[2 * r + 1]; }
        const int rem = off % step;
        for (int j = rem ? step - rem : 0; j < n; j += step) {
            const int slot = (off + j) / step;             // < ceil(total / step) <= max_points
            const double rho = (double)sr[j] * res;
            double x = rho * ct, y = rho * st;
            if constexpr (MOTION)
                if (moving) {
                    const double x0 = x, y0 = y;
                    x = __dadd_rn(__dadd_rn(__dmul_rn(cs.x, x0), -__dmul_rn(cs.y, y0)), d.x);
                    y = __dadd_rn(__dadd_rn(__dmul_rn(cs.y, x0), __dmul_rn(cs.x, y0)), d.y);
                }
            out[2 * slot] = x;
            out[2 * slot + 1] = y;
        }
        off += n;
    }
    if (t == 0) {
        cloud_n[b] = (total + step - 1) / step;
        cloud_peaks[b] = total;
    }
}

__global__ __launch_bounds__(CG_THREADS) void cloud_gather_kernel(const uint16_t *__restrict__ row_stage, int stage_cap,
                                                                  const int32_t *__restrict__ row_count, int rows, const double *__restrict__ trig,
                                                                  double res, int max_points, int point_stride, double *__restrict__ cloud,
                                                                  int32_t *__restrict__ cloud_n, int32_t *__restrict__ cloud_peaks)
{
    cloud_gather_body<false>(row_stage, stage_cap, row_count, rows, trig, res, max_points, point_stride, cloud, cloud_n, cloud_peaks, nullptr);
}

__global__ __launch_bounds__(CG_THREADS) void cloud_gather_motion_kernel(const uint16_t *__restrict__ row_stage, int stage_cap,
                                                                         const int32_t *__restrict__ row_count, int rows,
                                                                         const double *__restrict__ trig, double res, int max_points,
                                                                         int point_stride, double *__restrict__ cloud,
                                                                         int32_t *__restrict__ cloud_n, int32_t *__restrict__ cloud_peaks,
                                                                         const double *__restrict__ motion)
{
    cloud_gather_body<true>(row_stage, stage_cap, row_count, rows, trig, res, max_points, point_stride, cloud, cloud_n, cloud_peaks, motion);
}

// ---------------------------------------------------------------------------------------------------------------- host
// the staging and the build: what they do is said where loop.h declares them
hipError_t sc_launch_cloud_gather(hipStream_t st, const roam_loop_db *db, int nb, const uint16_t *stage, int stage_cap, const int32_t *rcount,
                                  int64_t first, const double *motion)
{
    if (motion)
        hipLaunchKernelGGL(cloud_gather_motion_kernel, dim3(nb), dim3(CG_THREADS), 0, st, stage, stage_cap, rcount, db->cloud_rows, db->trig,
                           db->res, db->max_points, db->point_stride, db->cloud + 2 * first * db->max_points, db->cloud_n + first,
                           db->cloud_peaks + first, motion);
    else
        hipLaunchKernelGGL(cloud_gather_kernel, dim3(nb), dim3(CG_THREADS), 0, st, stage, stage_cap, rcount, db->cloud_rows, db->trig, db->res,
                           db->max_points, db->point_stride, db->cloud + 2 * first * db->max_points, db->cloud_n + first, db->cloud_peaks + first);
    return hipGetLastError();
}

int32_t sc_cloud_stage(roam_ctx *ctx, int rows, int cols, int nb, uint16_t **stage, int32_t **rcount)
{
    const int stage_cap = (cols + 1) / 2;
    *stage = (uint16_t *)roam_scratch(ctx, S_TMP0, sizeof(uint16_t) * (size_t)nb * rows * stage_cap);
    *rcount = (int32_t *)roam_scratch(ctx, S_TMP1, sizeof(int32_t) * (size_t)nb * rows);
    return *stage && *rcount ? ROAM_OK : ROAM_E_HIP;
}

int32_t sc_motion_upload(roam_ctx *ctx, int rows, int nb, const double *h_motion, const double **d_motion)
{
    *d_motion = nullptr;
    if (!h_motion) return ROAM_OK;
    const size_t bytes = sizeof(double) * 4 * (size_t)nb * rows;
    double *d = (double *)roam_scratch(ctx, S_IN2, bytes);
    if (!d) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(d, h_motion, bytes, hipMemcpyHostToDevice, ctx->stream));
    *d_motion = d;
    return ROAM_OK;
}

int32_t sc_build_clouds(roam_ctx *ctx, const roam_loop_db *db, const PeakSrc &ps, int nb, int cols, int64_t first, const double *h_motion)
{
    uint16_t *stage;
    int32_t *rcount;
    const double *d_motion;
    LOOP_TRY(sc_cloud_stage(ctx, db->cloud_rows, cols, nb, &stage, &rcount));
    LOOP_TRY(sc_motion_upload(ctx, db->cloud_rows, nb, h_motion, &d_motion));
    HIP_TRY(ctx, launch_peaks_rows(ctx->stream, ps, nb, db->cloud_rows, cols, stage, (cols + 1) / 2, rcount));
    HIP_TRY(ctx, sc_launch_cloud_gather(ctx->stream, db, nb, stage, (cols + 1) / 2, rcount, first, d_motion));
    return ROAM_OK;
}

int32_t sc_motion_table(roam_ctx *ctx, const roam_loop_db *db, int n, const double *velocities, double period, int cols, std::vector<double> *table)
{
    table->clear();
    if (!velocities) return ROAM_OK;
    if (!db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db: velocities for a db that keeps no clouds (roam_loop_db_keep_clouds)"); return ROAM_E_ARG; }
    if (!cloud_motion_check(ctx->err, sizeof(ctx->err), n, velocities, period, cols, db->res, ROAM_ICP_MAX_COORD)) return ROAM_E_ARG;
    table->resize(4 * (size_t)n * db->cloud_rows);
    cloud_motion_fill(db->cloud_rows, period, n, velocities, table->data());
    return ROAM_OK;
}

int32_t sc_check_cloud_add(roam_ctx *ctx, const roam_loop_db *db, int rows, int cols)
{
    if (rows != db->cloud_rows) {
        ROAM_SET_ERR(ctx, "loop db: rows = %d, but the database keeps clouds of %d azimuths", rows, db->cloud_rows);
        return ROAM_E_ARG;
    }
    if (cols > ROAM_MAX_COLS) { ROAM_SET_ERR(ctx, "loop db: cols <= %d for a database that keeps clouds, not %d", ROAM_MAX_COLS, cols); return ROAM_E_ARG; }
    return ROAM_OK;
}

int32_t sc_mirror_counts(roam_ctx *ctx, roam_loop_db *db, int64_t first, int n)
{
    HIP_TRY(ctx, hipMemcpyAsync(db->h_n.data() + first, db->cloud_n + first, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(db->h_peaks.data() + first, db->cloud_peaks + first, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

extern "C" int32_t roam_polar_cloud_table(int32_t rows, double *cos_out, double *sin_out)
{
    if (rows < 1 || rows > SC_MAX_ROWS || !cos_out || !sin_out) return ROAM_E_ARG;
    for (int t = 0; t < rows; ++t) {
        const double phi = (2.0 * M_PI * (double)t) / (double)rows;
        cos_out[t] = cos(phi);
        sin_out[t] = sin(phi);
    }
    return ROAM_OK;
}

extern "C" int32_t roam_cloud_motion_table(int32_t rows, double period, int32_t n, const double *velocities, double *out)
{
    if (rows < 1 || rows > SC_MAX_ROWS || n < 1 || !velocities || !out) return ROAM_E_ARG;
    if (!cloud_motion_check(nullptr, 0, n, velocities, period, 0, 0.0, INFINITY)) return ROAM_E_ARG;
    cloud_motion_fill(rows, period, n, velocities, out);
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_keep_clouds(roam_ctx *ctx, roam_loop_db *db, int32_t rows, int32_t max_points, int32_t point_stride,
                                            double range_resolution_m)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    if (db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db: db keeps clouds already"); return ROAM_E_ARG; }
    if (db->count) { ROAM_SET_ERR(ctx, "loop db: keep_clouds wants an empty db, this one holds %d entries", db->count); return ROAM_E_ARG; }
    if (max_points < 1 || max_points > ROAM_ICP_MAX_POINTS) {
        ROAM_SET_ERR(ctx, "loop db: max_points in [1, %d], not %d", ROAM_ICP_MAX_POINTS, max_points);
        return ROAM_E_ARG;
    }
    if (point_stride < 1) { ROAM_SET_ERR(ctx, "loop db: point_stride >= 1, not %d", point_stride); return ROAM_E_ARG; }
    if (!(std::isfinite(range_resolution_m) && range_resolution_m > 0.0)) {
        ROAM_SET_ERR(ctx, "loop db: range_resolution_m finite and > 0, not %g", range_resolution_m);
        return ROAM_E_ARG;
    }
    if (rows < 1 || rows > SC_MAX_ROWS) { ROAM_SET_ERR(ctx, "loop db: rows in [1, %d], not %d", SC_MAX_ROWS, rows); return ROAM_E_ARG; }
    const int64_t per = (int64_t)max_points * 2 * sizeof(double);
    if (db->capacity > SC_DB_BYTES / per) {
        ROAM_SET_ERR(ctx, "loop db: capacity %d x max_points %d x 16 bytes is beyond the %lld bytes of a database", db->capacity, max_points,
                     (long long)SC_DB_BYTES);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<double> table(2 * (size_t)rows);
    (void)roam_polar_cloud_table(rows, table.data(), table.data() + rows);
    const size_t cap = (size_t)db->capacity;
    if (hipMalloc(&db->cloud, (size_t)per * cap) != hipSuccess || hipMalloc(&db->cloud_n, sizeof(int32_t) * cap) != hipSuccess ||
        hipMalloc(&db->cloud_peaks, sizeof(int32_t) * cap) != hipSuccess || hipMalloc(&db->trig, sizeof(double) * table.size()) != hipSuccess) {
        ROAM_SET_ERR(ctx, "loop db: hipMalloc of %lld bytes of clouds failed", (long long)(per * db->capacity));
        for (void **q : {(void **)&db->cloud, (void **)&db->cloud_n, (void **)&db->cloud_peaks, (void **)&db->trig}) {
            if (*q) (void)hipFree(*q);
            *q = nullptr;
        }
        return ROAM_E_HIP;
    }
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemsetAsync(db->cloud_n, 0, sizeof(int32_t) * cap, st));
    HIP_TRY(ctx, hipMemsetAsync(db->cloud_peaks, 0, sizeof(int32_t) * cap, st));
    HIP_TRY(ctx, hipMemcpyAsync(db->trig, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));               // the table is a local
    db->h_n.assign(cap, 0);
    db->h_peaks.assign(cap, 0);
    db->max_points = max_points; db->point_stride = point_stride; db->res = range_resolution_m;
    db->cloud_rows = rows;                                // last: the database keeps clouds from here on
    return ROAM_OK;
}

// db keeps clouds and `index` is a stored entry
static int32_t sc_check_cloud_entry(roam_ctx *ctx, const roam_loop_db *db, int32_t index)
{
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    if (!db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db: db keeps no clouds (roam_loop_db_keep_clouds)"); return ROAM_E_STATE; }
    if (index < 0 || index >= db->count) { ROAM_SET_ERR(ctx, "loop db: index %d outside the %d entries stored", index, db->count); return ROAM_E_ARG; }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_set_cloud(roam_ctx *ctx, roam_loop_db *db, int32_t index, const double *xy, int32_t n)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_cloud_entry(ctx, db, index));
    if (n < 0 || n > db->max_points) { ROAM_SET_ERR(ctx, "loop db: n in [0, max_points = %d], not %d", db->max_points, n); return ROAM_E_ARG; }
    if (n > 0 && !xy) { ROAM_SET_ERR(ctx, "loop db: xy is null"); return ROAM_E_ARG; }
    for (int64_t q = 0; q < 2 * (int64_t)n; ++q)
        if (!(fabs(xy[q]) <= ROAM_ICP_MAX_COORD)) {       // NaN and the infinities fail too
            ROAM_SET_ERR(ctx, "loop db: xy point %lld: a coordinate that is not finite or beyond %g m", (long long)(q / 2), ROAM_ICP_MAX_COORD);
            return ROAM_E_ARG;
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int32_t two[2] = {n, n};
    if (n > 0) HIP_TRY(ctx, hipMemcpyAsync(db->cloud + 2 * (int64_t)index * db->max_points, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(db->cloud_n + index, two, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(db->cloud_peaks + index, two + 1, sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    db->h_n[index] = db->h_peaks[index] = n;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_get_cloud(roam_ctx *ctx, roam_loop_db *db, int32_t index, double *xy_out, int32_t cap, int32_t *n_out,
                                          int32_t *n_peaks_out)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(sc_check_cloud_entry(ctx, db, index));
    if (cap < 0 || (cap > 0 && !xy_out)) { ROAM_SET_ERR(ctx, "loop db: xy_out of cap >= 0 points, not %d%s", cap, cap > 0 ? " and null" : ""); return ROAM_E_ARG; }
    const int n = db->h_n[index];
    if (n_out) *n_out = n;
    if (n_peaks_out) *n_peaks_out = db->h_peaks[index];
    const int m = n < cap ? n : cap;
    if (m > 0) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipMemcpyAsync(xy_out, db->cloud + 2 * (int64_t)index * db->max_points, sizeof(double) * 2 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (n > cap) { ROAM_SET_ERR(ctx, "loop db: entry %d holds %d points, capacity %d", index, n, cap); return ROAM_E_CAPACITY; }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_cloud_counts(const roam_loop_db *db, int32_t first, int32_t n, int32_t *n_out, int32_t *n_peaks_out)
{
    if (!db || !db->cloud_rows || first < 0 || n < 0 || n > db->count - first) return ROAM_E_ARG;
    for (int i = 0; i < n; ++i) {
        if (n_out) n_out[i] = db->h_n[first + i];
        if (n_peaks_out) n_peaks_out[i] = db->h_peaks[first + i];
    }
    return ROAM_OK;
}
