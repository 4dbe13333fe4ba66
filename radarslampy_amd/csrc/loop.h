// loop.h - what the units of the place-recognition family share: the loop database, its scan-context descriptors, its resident peak
// clouds and the verification that runs from them; internal.  Which unit owns what:
//   loop_describe.hip  scan_context_kernel, scan_context_norm_kernel; the geometry and float32 argument checks;
//                      roam_scan_context_plan, roam_scan_context_f32; host float32 images in chunks (sc_describe_host_f32)
//   loop_db.hip        the database's lifetime (create, destroy, count, get) and its three adds: add_f32, add_desc and the engine's
//                      resident records (loop_records_prepare / _append / _time_describe / _time_offsets / _time_cloud)
//   loop_query.hip     loop_distance_kernel, loop_variant_fold_kernel, loop_select_kernel, loop_variant_gather_kernel; the query pass
//                      (LoopQueryBufs and the loop_query_* steps); roam_loop_db_query, roam_loop_db_query_offsets and their timing entries
//   loop_cloud.hip     cloud_gather_kernel and its motion form, the row staging and the cloud build; roam_polar_cloud_table,
//                      roam_cloud_motion_table (cloud_motion.h: the velocity checks and the table, host only), roam_loop_db_keep_clouds,
//                      set_cloud, get_cloud, cloud_counts
//   loop_verify.hip    loop_pairs_kernel, the pair scratch and staging; roam_loop_db_verify, roam_time_loop_db_verify,
//                      roam_loop_db_query_verify
//   loop_offset.hip    the origin-shifted variants of an entry (Scan Context++): scan_context_offset_kernel and its finishing kernel,
//                      the variant store (roam_loop_db_keep_offsets, set_variants, get_variants), roam_scan_context_offset_table,
//                      roam_scan_context_offsets_f32; loop_query.hip reads the store as its queries, loop_verify.hip seeds from it
//   loop_map.hip       the global map from the resident clouds at given poses: map_bounds_kernel, map_splat_kernel, the compaction
//                      (map_count_kernel, map_scan_kernel, map_write_kernel); roam_map_pose_table, roam_map_plan,
//                      roam_loop_db_map_bounds, roam_loop_db_map_render, roam_time_loop_db_map.  It reads the database and writes
//                      scratch of the context only; no other unit calls into it
//   map_match.hip      a scan localised in a rendered map (correlative matching): the resident match field (roam_map_field),
//                      mm_field_kernel, mm_match_kernel, mm_finish_kernel; roam_map_field_*, roam_map_match_angles, roam_map_match_plan,
//                      roam_map_match_clouds, roam_loop_db_map_match, roam_time_map_match (map_match.h: the tables and the argument
//                      checks, host only).  It reads the database's clouds and the grids a render returned; it calls no other unit
//   icp.hip            the ICP of a pair of stored clouds (icp2d_store_kernel), which loop_verify.hip launches
// engine_lanes.hip describes the engine's pool (LoopPool) and calls the record entries.  The reference has no place recognition (a
// commented-out "import m2dp" at Mapping.py:7 and an unused Keyframe.pointCloud at :61-62), so parity is unpinned: the contracts are
// tests/scan_context_model.py, tests/loop_cloud_model.py, tests/loop_cloud_motion_model.py, tests/scan_context_offset_model.py,
// tests/global_map_model.py and tests/map_match_model.py.
#pragma once
#include "roam_internal.h"
#include <vector>

#define LOOP_UNIT __attribute__((visibility("hidden")))      // host functions that cross a unit, kept out of the library's symbol table
#define LOOP_TRY(call) do { const int32_t rc_ = (call); if (rc_ != ROAM_OK) return rc_; } while (0)

#define SC_THREADS 256
#define SC_QW 4                                  // queries per wave
#define SC_QB (SC_QW * (SC_THREADS / 64))        // queries per workgroup
#define SC_LDS_BYTES 32768                       // the doubled candidate of one phase
#define SC_DB_BYTES ((int64_t)2000 << 20)        // a database, and the scratch of one launch, as in the other batched stages
#define SC_CHUNK_ENV "ROAM_LOOP_CHUNK_BYTES"     // the tests' smaller launch scratch (roam_chunk_limit): where a batch is cut, nothing else
#define SC_MAX_ROWS 65536

struct roam_loop_db {
    roam_ctx *owner = nullptr;   // the context it was created on: its allocations live on that context's device (map_match.hip asks)
    int S = 0, R = 0, Rp = 0, capacity = 0, count = 0;
    float *desc = nullptr;       // capacity x S x R
    double *nrm = nullptr;       // capacity x S x Rp: normalised columns, zero for an invalid sector and in the padding
    int32_t *valid = nullptr;    // capacity x S
    // the peak clouds (roam_loop_db_keep_clouds): cloud_rows = 0 when the database keeps none
    int cloud_rows = 0, max_points = 0, point_stride = 0;
    double res = 0.0;            // metres per range bin
    double *cloud = nullptr;     // capacity x max_points x 2, metres
    int32_t *cloud_n = nullptr, *cloud_peaks = nullptr;      // capacity each: the points stored, the scan's full peak count
    double *trig = nullptr;      // cos(phi_t), t < cloud_rows, then sin(phi_t)
    std::vector<int32_t> h_n, h_peaks;                       // host mirror of the two counts, kept by the blocking entries
    // the origin-shifted variants (roam_loop_db_keep_offsets): n_off = 0 when the database keeps none.  Variant a >= 1 of entry e is
    // row e n_off + a - 1 of the store; variant 0 is the entry itself
    int n_off = 0, off_rows = 0; // off_rows: the azimuths off_trig was made for (0: not yet)
    float *vdesc = nullptr;      // capacity x n_off x S x R
    double *vnrm = nullptr;      // capacity x n_off x S x Rp
    int32_t *vvalid = nullptr;   // capacity x n_off x S
    double *off_bins = nullptr, *off_m = nullptr;            // n_off x 2 each: the offsets in range bins and in metres
    double *off_trig = nullptr;  // sc_offset_table's four tables for off_rows azimuths (room for SC_MAX_ROWS)
};

// the float64 norm of one sector column of a descriptor, rings ascending - the one function behind every stored nrm / valid, so that
// an entry's (and a variant's) stored bits depend on its descriptor alone
__device__ static inline double sc_sector_norm(const float *d, int R)
{
    double n2 = 0.0;
    for (int r = 0; r < R; ++r) n2 += (double)d[r] * (double)d[r];
    return sqrt(n2);
}

__device__ static inline double sc_normalised(float d, double norm) { return norm > 0.0 ? (double)d / norm : 0.0; }

// image z of a launch: base + (index ? index[z] : z) * image_stride (+ payload_off for u8 records); strides in elements
struct ScSrc {
    const void *base;
    int64_t image_stride, row_stride;
    int32_t payload_off;
    const int32_t *index;
};

#define SC_FAIL(err, cap, ...)                              \
    do {                                                    \
        if (err) snprintf(err, cap, __VA_ARGS__);           \
        return ROAM_E_ARG;                                  \
    } while (0)

struct ScOffsets;                                // loop_offset.hip, below

// ---- loop_describe.hip
// the checks of the geometry, shared by every describing entry -> the clip
LOOP_UNIT int32_t sc_check_geometry(char *err, size_t cap, int32_t rows, int32_t cols, int32_t clip_px, int32_t sectors, int32_t rings, int *clip_out);
LOOP_UNIT int32_t sc_check_f32_args(roam_ctx *ctx, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride,
                                    int64_t image_stride, int32_t clip_px, int32_t sectors, int32_t rings, double floor, int *clip);
// n images -> rows of desc / nrm / valid starting at entry `first` (nrm / valid may be null)
LOOP_UNIT hipError_t sc_launch_describe(hipStream_t st, bool u8, const ScSrc &src, int n, int rows, int clip, int S, int R, double floor_v,
                                        int floor_code, float *desc, double *nrm, int32_t *valid, int64_t first);
// the n descriptors already in db->desc from entry `first` on -> their nrm / valid
LOOP_UNIT hipError_t sc_launch_norm(hipStream_t st, const roam_loop_db *db, int64_t first, int n);
// the same kernel on any n_rows sector columns of ready-made descriptors (the variant store's)
LOOP_UNIT hipError_t sc_launch_norm_rows(hipStream_t st, const float *desc, int64_t n_rows, int R, int Rp, double *nrm, int32_t *valid);
// host float32 images in chunks under the scratch limit: upload the clipped columns tightly, describe into desc (+ nrm, valid) from
// entry `first` on.  cloud_db (optional, a database that keeps clouds; cols = the images' full width): all the columns are uploaded,
// and the images' peak clouds go to the entries from `first` on as well - with h_motion (sc_motion_table's table of the n images on the
// host, null: none) motion-compensated; its rows follow the chunks
LOOP_UNIT int32_t sc_describe_host_f32(roam_ctx *ctx, const float *polar, int n, int rows, int64_t row_stride, int64_t image_stride, int clip,
                                       int S, int R, double floor_v, float *desc, double *nrm, int32_t *valid, int64_t first,
                                       const roam_loop_db *cloud_db = nullptr, int cols = 0, const ScOffsets *offs = nullptr,
                                       const double *h_motion = nullptr);

// ---- loop_offset.hip
// where the variants of a describing call come from and go to: device pointers, the store's at its entry 0 (vnrm / vvalid may be null)
struct ScOffsets {
    int n_off;
    const double *trig, *off_bins;
    float *vdesc;
    double *vnrm;
    int32_t *vvalid;
};
// tables of the host's libm for `rows` azimuths and the S sector boundaries: out = cos(phi_a) (rows), sin(phi_a) (rows), cos(beta_s) (S),
// sin(beta_s) (S), phi_a = (2.0 * M_PI * (a + 0.5)) / rows, beta_s = (2.0 * M_PI * floor(s rows / S)) / rows
LOOP_UNIT void sc_offset_table(int rows, int S, double *out);
// device bytes of partial sums one image of a launch takes (the float32 form: one slab per block of rows; u8: one slab)
LOOP_UNIT int64_t sc_offset_part_bytes(bool u8, int rows, int S, int R, int n_off);
// the n_off variants of n images -> the store's entries from `first` on; enqueued, not awaited (scratch S_TMP5 / S_TMP6)
LOOP_UNIT int32_t sc_launch_offsets(roam_ctx *ctx, bool u8, const ScSrc &src, int n, int rows, int clip, int S, int R, double floor_v,
                                    int floor_code, const ScOffsets &offs, int64_t first);
// a database that keeps offsets: its tables for scans of `rows` azimuths (uploaded when rows changes) -> what sc_launch_offsets takes
LOOP_UNIT int32_t sc_offsets_of_db(roam_ctx *ctx, roam_loop_db *db, int rows, ScOffsets *out);
// the n ready-made entries from `first` on: all their variants zero (invalid: distance 1)
LOOP_UNIT int32_t sc_offsets_clear(roam_ctx *ctx, const roam_loop_db *db, int64_t first, int n);
LOOP_UNIT void sc_offsets_free(roam_loop_db *db);

// ---- loop_cloud.hip
// bytes of row staging one scan of `cols` range bins takes (row_stage + row_count)
static inline int64_t sc_stage_bytes(int rows, int cols) { return (int64_t)rows * ((cols + 1) / 2) * sizeof(uint16_t) + (int64_t)rows * sizeof(int32_t); }
// the staging of nb scans (taken from the scratch slots S_TMP0 / S_TMP1, which no enqueued engine step reads: a step owns its buffers)
LOOP_UNIT int32_t sc_cloud_stage(roam_ctx *ctx, int rows, int cols, int nb, uint16_t **stage, int32_t **rcount);
// motion: the launch's motion table on the device, nb x rows x 4 (null: no scan has a velocity, the plain kernel)
LOOP_UNIT hipError_t sc_launch_cloud_gather(hipStream_t st, const roam_loop_db *db, int nb, const uint16_t *stage, int stage_cap, const int32_t *rcount,
                                            int64_t first, const double *motion = nullptr);
// the clouds of the nb scans of `ps` (cols range bins each) -> the entries from `first` on; enqueued, not awaited.  h_motion: these
// scans' rows of sc_motion_table's table on the host (null: none), which the caller keeps until the stream has been waited for
LOOP_UNIT int32_t sc_build_clouds(roam_ctx *ctx, const roam_loop_db *db, const PeakSrc &ps, int nb, int cols, int64_t first,
                                  const double *h_motion = nullptr);
// the checks of an add's velocities (n x 3, null: none -> an empty table) against scans of `cols` range bins, then the motion table of
// the n scans, n x cloud_rows x 4 (cloud_motion.h).  No device call
LOOP_UNIT int32_t sc_motion_table(roam_ctx *ctx, const roam_loop_db *db, int n, const double *velocities, double period, int cols,
                                  std::vector<double> *table);
// nb scans' rows of that table -> the device (scratch S_IN2), enqueued; h_motion null -> *d_motion null
LOOP_UNIT int32_t sc_motion_upload(roam_ctx *ctx, int rows, int nb, const double *h_motion, const double **d_motion);
// bytes of motion table one scan takes
static inline int64_t sc_motion_bytes(int rows) { return (int64_t)rows * 4 * sizeof(double); }
// what an add to a cloud-keeping database refuses beyond the descriptor's checks
LOOP_UNIT int32_t sc_check_cloud_add(roam_ctx *ctx, const roam_loop_db *db, int rows, int cols);
// the end of a blocking add of n entries from `first` on: their counts to the host mirror; waits for the stream
LOOP_UNIT int32_t sc_mirror_counts(roam_ctx *ctx, roam_loop_db *db, int64_t first, int n);

// ---- loop_db.hip: resident u8 records, for engine_lanes.hip after its own checks (the engine, the pool indices)
struct LoopPool {
    const uint8_t *pool;         // pool_scans records of rec_bytes
    int64_t rec_bytes, row_stride;
    int32_t payload_off, rows, clip;         // clip: the range bins a record holds
    hipEvent_t pending;          // the pool's pending uploads (null: none): the stream waits for it once the arguments have passed
};
// Each entry first checks (db, the geometry, floor_code, the clouds, the room for n entries; a timing entry then its reps) and only
// then enqueues: the wait for the pool's uploads and the upload of pool_idx (host, n indices the caller has checked).
// describe the records and append them to db, blocking; a database that keeps clouds gets the records' peak clouds too, with
// velocities (n x 3, null: none; refused before anything is enqueued - sc_motion_table) motion-compensated over `period`
LOOP_UNIT int32_t loop_records_append(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, int32_t n, const int32_t *pool_idx, int32_t clip_px,
                                      int32_t floor_code, int32_t *first_index_out, const double *velocities = nullptr, double period = 0.25);
// nothing is appended: `reps` launches of the describing kernel into the free entries, timed (roam_time_launches)
LOOP_UNIT int32_t loop_records_time_describe(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, int32_t n, const int32_t *pool_idx, int32_t clip_px,
                                             int32_t floor_code, int32_t reps, float *ms_per_rep);
// likewise the variants of the records (the clear, the binning kernel and the finishing kernel as one launch) into the free entries
LOOP_UNIT int32_t loop_records_time_offsets(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, int32_t n, const int32_t *pool_idx, int32_t clip_px,
                                            int32_t floor_code, int32_t reps, float *ms_per_rep);
// likewise the two kernels of the cloud build, each alone: ms[0] the peak row kernel, ms[1] the cloud gather - with velocities its
// motion form, the table uploaded once before the launches
LOOP_UNIT int32_t loop_records_time_cloud(roam_ctx *ctx, roam_loop_db *db, const LoopPool &pool, int32_t n, const int32_t *pool_idx, int32_t reps,
                                          float *ms, const double *velocities = nullptr, double period = 0.25);

// ---- loop_query.hip: the query pass of one chunk of nq queries at k candidates each, shared with roam_loop_db_query_verify
LOOP_UNIT int32_t sc_check_query(roam_ctx *ctx, const roam_loop_db *db, int32_t n_query, const int32_t *query_index, const int32_t *max_index,
                                 int32_t k, double max_distance);
struct LoopQueryBufs {
    double *d_dist;              // nq x count  (S_TMP0)
    int32_t *d_shift;            // nq x count  (S_TMP1)
    int32_t *d_q, *d_qmax;       // nq each, one take of 2 nq: the queries' indices, their clamped max_index  (S_IN1)
    int32_t *d_ci;               // nq x k: the candidates' indices, distances and shifts  (S_OUT0, S_OUT1, S_OUT2)
    double *d_cd;
    int32_t *d_cs;
    // a query over the variants (n_off > 0; all null otherwise)
    int n_off;
    double *d_vdist;             // nq n_off x count: row q n_off + o = variant o + 1 of query q  (S_TMP2)
    int32_t *d_vshift;           // likewise  (S_TMP5)
    int32_t *d_var;              // nq x count: the winning variant of every pair  (S_TMP6)
    int32_t *d_vq, *d_vqmax;     // nq n_off each: the variants' rows in the store, their queries' maxima  (S_TMP7)
    int32_t *d_cv;               // nq x k: the candidates' winning variants  (S_IN0)
    std::vector<int32_t> h_rows; // the host side of d_vq / d_vqmax while their upload is in flight
};
// max_index clamped to [0, count]
LOOP_UNIT std::vector<int32_t> loop_query_clamp(const roam_loop_db *db, int32_t n_query, const int32_t *max_index);
// take the scratch of the chunk and upload its nq indices and clamped maxima (host pointers at the chunk's first query)
// with_variants: also the scratch and the row lists of a query over the variants of a database that keeps offsets
LOOP_UNIT int32_t loop_query_stage(roam_ctx *ctx, const roam_loop_db *db, int nq, int k, const int32_t *query_index, const int32_t *qmax, LoopQueryBufs *b,
                                   bool with_variants = false);
// device bytes of distance scratch one query takes
LOOP_UNIT int64_t loop_query_bytes(const roam_loop_db *db, bool with_variants);
// distance, then selection.  every_pair: the distance of every (query, entry), not only of the entries below the query's maximum - what
// the dist_full / shift_full outputs want
LOOP_UNIT int32_t loop_query_enqueue(roam_ctx *ctx, const roam_loop_db *db, const LoopQueryBufs &b, int nq, int k, double max_distance, bool every_pair);
// the three candidate downloads
LOOP_UNIT int32_t loop_query_download(roam_ctx *ctx, const LoopQueryBufs &b, int nq, int k, int32_t *cand_index, double *cand_dist, int32_t *cand_shift);

// ---- icp.hip, for the verification (loop_verify.hip).  Pair p aligns the stored cloud of entry src_index[p] to that of entry
// dst_index[p]: slot e = cloud + 2 e max_points, cloud_n[e] points; an index of -1 is an empty cloud.  partner: np x max_points
struct IcpStoreArgs {
    const double *cloud;
    const int32_t *cloud_n;
    int32_t max_points;
    const int32_t *src_index, *dst_index;         // np each
    const double *init;                           // np x 3
    int32_t *partner;
    double *pose;                                 // np x 3
    roam_icp_stats *stats;
    roam_icp_opts o;
};
LOOP_UNIT hipError_t launch_icp2d_store(hipStream_t st, const IcpStoreArgs &A, int np);
// opts (NULL: the defaults) -> *o, checked as roam_icp2d_batch checks them
LOOP_UNIT int32_t roam_icp_resolve_opts(roam_ctx *ctx, const roam_icp_opts *opts, roam_icp_opts *o);
