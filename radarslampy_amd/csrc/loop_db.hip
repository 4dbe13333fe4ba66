// The loop database: its lifetime and its three ways of adding entries - host float32 images, ready-made descriptors, and the u8
// records resident in an engine's pool.  No kernel lives here: the descriptors are loop_describe.hip's, the clouds loop_cloud.hip's.
// Map of the family: loop.h.
#include "loop.h"
#include <cmath>

static void sc_db_free(roam_loop_db *db)
{
    if (db->desc) (void)hipFree(db->desc);
    if (db->nrm) (void)hipFree(db->nrm);
    if (db->valid) (void)hipFree(db->valid);
    if (db->cloud) (void)hipFree(db->cloud);
    if (db->cloud_n) (void)hipFree(db->cloud_n);
    if (db->cloud_peaks) (void)hipFree(db->cloud_peaks);
    if (db->trig) (void)hipFree(db->trig);
    sc_offsets_free(db);
    delete db;
}

extern "C" int32_t roam_loop_db_create(roam_ctx *ctx, int32_t capacity, int32_t sectors, int32_t rings, roam_loop_db **out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!out) { ROAM_SET_ERR(ctx, "loop db: out is null"); return ROAM_E_ARG; }
    if (sectors < 2 || sectors > ROAM_SCAN_CONTEXT_MAX_SECTORS || rings < 1 || rings > ROAM_SCAN_CONTEXT_MAX_RINGS) {
        ROAM_SET_ERR(ctx, "loop db: sectors in [2, %d] and rings in [1, %d], not %d and %d", ROAM_SCAN_CONTEXT_MAX_SECTORS,
                     ROAM_SCAN_CONTEXT_MAX_RINGS, sectors, rings);
        return ROAM_E_ARG;
    }
    const int Rp = (rings + 3) & ~3;
    const int64_t per = (int64_t)sectors * (sizeof(float) * rings + sizeof(double) * Rp + sizeof(int32_t));
    if (capacity < 1 || capacity > SC_DB_BYTES / per) {
        ROAM_SET_ERR(ctx, "loop db: capacity in [1, %lld] (%lld bytes per entry, %lld in all), not %d", (long long)(SC_DB_BYTES / per),
                     (long long)per, (long long)SC_DB_BYTES, capacity);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    roam_loop_db *db = new roam_loop_db;
    db->owner = ctx;
    db->S = sectors; db->R = rings; db->Rp = Rp; db->capacity = capacity;
    const size_t rows = (size_t)capacity * sectors;
    if (hipMalloc(&db->desc, sizeof(float) * rows * rings) != hipSuccess || hipMalloc(&db->nrm, sizeof(double) * rows * Rp) != hipSuccess ||
        hipMalloc(&db->valid, sizeof(int32_t) * rows) != hipSuccess) {
        ROAM_SET_ERR(ctx, "loop db: hipMalloc of %lld bytes failed", (long long)(per * capacity));
        sc_db_free(db);
        return ROAM_E_HIP;
    }
    *out = db;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_destroy(roam_ctx *ctx, roam_loop_db *db)
{
    if (!ctx || !db) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // nothing enqueued reads it any more
    sc_db_free(db);
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_count(const roam_loop_db *db, int32_t *count)
{
    if (!db || !count) return ROAM_E_ARG;
    *count = db->count;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_get(roam_ctx *ctx, roam_loop_db *db, int32_t first, int32_t n, float *desc_out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db || !desc_out) { ROAM_SET_ERR(ctx, "loop db: %s is null", db ? "desc_out" : "db"); return ROAM_E_ARG; }
    if (first < 0 || n < 1 || n > db->count - first) {
        ROAM_SET_ERR(ctx, "loop db: entries [%d, %d + %d) outside the %d stored", first, first, n, db->count);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t per = (int64_t)db->S * db->R;
    HIP_TRY(ctx, hipMemcpyAsync(desc_out, db->desc + first * per, sizeof(float) * per * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the adds
static int32_t sc_check_room(roam_ctx *ctx, const roam_loop_db *db, int32_t n)
{
    if (n < 1) { ROAM_SET_ERR(ctx, "loop db: n >= 1 entries, not %d", n); return ROAM_E_ARG; }
    if (n > db->capacity - db->count) {
        ROAM_SET_ERR(ctx, "loop db: %d entries do not fit (%d of %d used)", n, db->count, db->capacity);
        return ROAM_E_CAPACITY;
    }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_add_f32(roam_ctx *ctx, roam_loop_db *db, const float *polar, int32_t n, int32_t rows, int32_t cols,
                                        int64_t row_stride, int64_t image_stride, int32_t clip_px, double floor, int32_t *first_index_out)
{
    return roam_loop_db_add_f32_motion(ctx, db, polar, n, rows, cols, row_stride, image_stride, clip_px, floor, nullptr, 0.25, first_index_out);
}

extern "C" int32_t roam_loop_db_add_f32_motion(roam_ctx *ctx, roam_loop_db *db, const float *polar, int32_t n, int32_t rows, int32_t cols,
                                               int64_t row_stride, int64_t image_stride, int32_t clip_px, double floor, const double *velocities,
                                               double period, int32_t *first_index_out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    int clip;
    LOOP_TRY(sc_check_f32_args(ctx, polar, n, rows, cols, row_stride, image_stride, clip_px, db->S, db->R, floor, &clip));
    if (db->cloud_rows) LOOP_TRY(sc_check_cloud_add(ctx, db, rows, cols));
    std::vector<double> motion;
    LOOP_TRY(sc_motion_table(ctx, db, n, velocities, period, cols, &motion));
    LOOP_TRY(sc_check_room(ctx, db, n));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ScOffsets offs;
    if (db->n_off) LOOP_TRY(sc_offsets_of_db(ctx, db, rows, &offs));
    LOOP_TRY(sc_describe_host_f32(ctx, polar, n, rows, row_stride, image_stride, clip, db->S, db->R, floor, db->desc, db->nrm, db->valid, db->count,
                                  db->cloud_rows ? db : nullptr, cols, db->n_off ? &offs : nullptr, velocities ? motion.data() : nullptr));
    if (db->cloud_rows) LOOP_TRY(sc_mirror_counts(ctx, db, db->count, n));
    if (first_index_out) *first_index_out = db->count;
    db->count += n;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_add_desc(roam_ctx *ctx, roam_loop_db *db, const float *desc, int32_t n, int32_t *first_index_out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db || !desc) { ROAM_SET_ERR(ctx, "loop db: %s is null", db ? "desc" : "db"); return ROAM_E_ARG; }
    LOOP_TRY(sc_check_room(ctx, db, n));
    const int64_t per = (int64_t)db->S * db->R;
    for (int64_t q = 0; q < per * n; ++q)
        if (!std::isfinite(desc[q])) {
            ROAM_SET_ERR(ctx, "loop db: desc entry %lld, element %lld is not finite", (long long)(q / per), (long long)(q % per));
            return ROAM_E_ARG;
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(db->desc + db->count * per, desc, sizeof(float) * per * n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, sc_launch_norm(st, db, db->count, n));
    if (db->n_off) LOOP_TRY(sc_offsets_clear(ctx, db, db->count, n));      // no scan, no variants: all invalid (roam_loop_db_set_variants fills them)
    if (db->cloud_rows) {                                 // ready-made descriptors bring no scan: empty clouds (roam_loop_db_set_cloud fills them)
        HIP_TRY(ctx, hipMemsetAsync(db->cloud_n + db->count, 0, sizeof(int32_t) * (size_t)n, st));
        HIP_TRY(ctx, hipMemsetAsync(db->cloud_peaks + db->count, 0, sizeof(int32_t) * (size_t)n, st));
        for (int i = 0; i < n; ++i) db->h_n[db->count + i] = db->h_peaks[db->count + i] = 0;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (first_index_out) *first_index_out = db->count;
    db->count += n;
    return ROAM_OK;
}

// ---------------------------------------------------------------------------------------------------------------- resident records
// what every record entry refuses, in this order: no db, a bad geometry (-> the clip), a bad floor_code, a cloud timing on a database
// that keeps none, records that are not the kept clouds' shape, no room for n entries.  Nothing is enqueued
static int32_t sc_check_records(roam_ctx *ctx, const roam_loop_db *db, const LoopPool &pool, int32_t n, int32_t clip_px, int32_t floor_code,
                                bool cloud_timing, int *clip)
{
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    LOOP_TRY(sc_check_geometry(ctx->err, sizeof(ctx->err), pool.rows, pool.clip, clip_px, db->S, db->R, clip));
    if (floor_code < 0 || floor_code > 254) { ROAM_SET_ERR(ctx, "loop db: floor_code in [0, 254], not %d", floor_code); return ROAM_E_ARG; }
    if (cloud_timing && !db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db timing: db keeps no clouds"); return ROAM_E_ARG; }
    if (db->cloud_rows) LOOP_TRY(sc_check_cloud_add(ctx, db, pool.rows, pool.clip));
    return sc_check_room(ctx, db, n);
}

static int32_t sc_check_reps(roam_ctx *ctx, int32_t reps)
{
    if (reps < 1) { ROAM_SET_ERR(ctx, "loop db timing: reps >= 1, not %d", reps); return ROAM_E_ARG; }
    return ROAM_OK;
}

// on ctx->stream: the wait for the pool's pending uploads, then the upload of the n pool indices (host) -> the records as the
// describing kernel and the peak row kernel read them
static int32_t sc_stage_records(roam_ctx *ctx, const LoopPool &pool, int32_t n, const int32_t *pool_idx, ScSrc *src, PeakSrc *peaks)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    if (pool.pending) HIP_TRY(ctx, hipStreamWaitEvent(st, pool.pending, 0));
    int32_t *d_idx = (int32_t *)roam_scratch(ctx, S_IN1, sizeof(int32_t) * (size_t)n);
    if (!d_idx) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(d_idx, pool_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    *src = ScSrc{pool.pool, pool.rec_bytes, pool.row_stride, pool.payload_off, d_idx};
    *peaks = PeakSrc{pool.pool, pool.rec_bytes, pool.row_stride, pool.payload_off, 1, d_idx};
    return ROAM_OK;
}

// the variants of the n staged records -> the entries from db->count on, in chunks that bound the slabs; enqueued
static int32_t sc_records_offsets(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, const ScSrc &src, int32_t n, int clip, int32_t floor_code,
                                  const ScOffsets &offs)
{
    int64_t chunk = roam_chunk_limit(SC_CHUNK_ENV, SC_DB_BYTES) / sc_offset_part_bytes(true, pool.rows, db->S, db->R, db->n_off);
    if (chunk < 1) chunk = 1;
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int nb = (int)(n - i0 < chunk ? n - i0 : chunk);
        ScSrc part = src;
        part.index += i0;
        LOOP_TRY(sc_launch_offsets(ctx, true, part, nb, pool.rows, clip, db->S, db->R, 0.0, floor_code, offs, db->count + i0));
        if (i0 + nb < n) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // the next chunk reuses the slabs
    }
    return ROAM_OK;
}

int32_t loop_records_append(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, int32_t n, const int32_t *pool_idx, int32_t clip_px,
                            int32_t floor_code, int32_t *first_index_out, const double *velocities, double period)
{
    int clip;
    LOOP_TRY(sc_check_records(ctx, db, pool, n, clip_px, floor_code, false, &clip));
    std::vector<double> motion;                           // lives until the stream has been waited for
    LOOP_TRY(sc_motion_table(ctx, db, n, velocities, period, pool.clip, &motion));
    ScSrc src;
    PeakSrc ps;
    LOOP_TRY(sc_stage_records(ctx, pool, n, pool_idx, &src, &ps));
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, sc_launch_describe(st, true, src, n, pool.rows, clip, db->S, db->R, 0.0, floor_code, db->desc, db->nrm, db->valid, db->count));
    if (db->n_off) {
        ScOffsets offs;
        LOOP_TRY(sc_offsets_of_db(ctx, db, pool.rows, &offs));
        LOOP_TRY(sc_records_offsets(ctx, db, pool, src, n, clip, floor_code, offs));
    }
    if (db->cloud_rows) {                                 // in chunks that bound the staging; what is stored does not depend on the cut
        int64_t chunk = roam_chunk_limit(SC_CHUNK_ENV, SC_DB_BYTES) / (sc_stage_bytes(pool.rows, pool.clip) + (velocities ? sc_motion_bytes(pool.rows) : 0));
        if (chunk < 1) chunk = 1;
        for (int64_t i0 = 0; i0 < n; i0 += chunk) {
            const int nb = (int)(n - i0 < chunk ? n - i0 : chunk);
            PeakSrc part = ps;
            part.lane_index += i0;
            LOOP_TRY(sc_build_clouds(ctx, db, part, nb, pool.clip, db->count + i0, velocities ? motion.data() + 4 * i0 * pool.rows : nullptr));
        }
        LOOP_TRY(sc_mirror_counts(ctx, db, db->count, n));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));               // the index list is the caller's
    if (first_index_out) *first_index_out = db->count;
    db->count += n;
    return ROAM_OK;
}

int32_t loop_records_time_describe(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, int32_t n, const int32_t *pool_idx, int32_t clip_px,
                                   int32_t floor_code, int32_t reps, float *ms_per_rep)
{
    int clip;
    LOOP_TRY(sc_check_records(ctx, db, pool, n, clip_px, floor_code, false, &clip));
    LOOP_TRY(sc_check_reps(ctx, reps));
    ScSrc src;
    PeakSrc ps;
    LOOP_TRY(sc_stage_records(ctx, pool, n, pool_idx, &src, &ps));
    const hipStream_t st = ctx->stream;
    return roam_time_launches(ctx, st, reps, ms_per_rep, [&] {
        return sc_launch_describe(st, true, src, n, pool.rows, clip, db->S, db->R, 0.0, floor_code, db->desc, db->nrm, db->valid, db->count);
    });
}

int32_t loop_records_time_offsets(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, int32_t n, const int32_t *pool_idx, int32_t clip_px,
                                  int32_t floor_code, int32_t reps, float *ms_per_rep)
{
    int clip;
    LOOP_TRY(sc_check_records(ctx, db, pool, n, clip_px, floor_code, false, &clip));
    LOOP_TRY(sc_check_reps(ctx, reps));
    if (!db->n_off) { ROAM_SET_ERR(ctx, "loop db timing: db keeps no offsets"); return ROAM_E_ARG; }
    if (n * sc_offset_part_bytes(true, pool.rows, db->S, db->R, db->n_off) > SC_DB_BYTES) {
        ROAM_SET_ERR(ctx, "loop db timing: %d records do not fit one launch", n);
        return ROAM_E_ARG;
    }
    ScSrc src;
    PeakSrc ps;
    LOOP_TRY(sc_stage_records(ctx, pool, n, pool_idx, &src, &ps));
    ScOffsets offs;
    LOOP_TRY(sc_offsets_of_db(ctx, db, pool.rows, &offs));
    int32_t rc = ROAM_OK;
    const int32_t rt = roam_time_launches(ctx, ctx->stream, reps, ms_per_rep, [&] {
        rc = sc_launch_offsets(ctx, true, src, n, pool.rows, clip, db->S, db->R, 0.0, floor_code, offs, db->count);
        return rc == ROAM_OK ? hipSuccess : hipErrorUnknown;
    });
    return rc != ROAM_OK ? rc : rt;
}

int32_t loop_records_time_cloud(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, int32_t n, const int32_t *pool_idx, int32_t reps, float *ms,
                                const double *velocities, double period)
{
    const int rows = pool.rows, cols = pool.clip;
    int clip;
    LOOP_TRY(sc_check_records(ctx, db, pool, n, 0, 0, true, &clip));
    LOOP_TRY(sc_check_reps(ctx, reps));
    std::vector<double> motion;
    LOOP_TRY(sc_motion_table(ctx, db, n, velocities, period, cols, &motion));
    if (n * (sc_stage_bytes(rows, cols) + (velocities ? sc_motion_bytes(rows) : 0)) > SC_DB_BYTES) { ROAM_SET_ERR(ctx, "loop db timing: %d records do not fit one launch", n); return ROAM_E_ARG; }
    ScSrc src;
    PeakSrc ps;
    LOOP_TRY(sc_stage_records(ctx, pool, n, pool_idx, &src, &ps));
    const hipStream_t st = ctx->stream;
    uint16_t *stage;
    int32_t *rcount;
    const double *d_motion;
    LOOP_TRY(sc_cloud_stage(ctx, rows, cols, n, &stage, &rcount));
    LOOP_TRY(sc_motion_upload(ctx, rows, n, velocities ? motion.data() : nullptr, &d_motion));
    LOOP_TRY(roam_time_launches(ctx, st, reps, ms, [&] { return launch_peaks_rows(st, ps, n, rows, cols, stage, (cols + 1) / 2, rcount); }));
    return roam_time_launches(ctx, st, reps, ms + 1, [&] { return sc_launch_cloud_gather(st, db, n, stage, (cols + 1) / 2, rcount, db->count, d_motion); });
}
