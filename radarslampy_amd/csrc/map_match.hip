// Map matching: a scan localised in a rendered global map by correlative scan-to-map matching (Olson 2009).  Map of the family: loop.h;
// the definition: include/roam_abi.h ("map matching"), the contract tests/map_match_model.py; the tables and the argument checks are
// map_match.h (host only).
//
// The field.  mm_field_kernel smears the occupied cells of a render with the caller's table (a maximum, not a sum) into one byte per
// cell.  The handle keeps it with a border of one zero cell on every side (Wp = W + 2), so that a position outside the grid is read
// as the zero it counts for: an index clamped to [-1, W] lands on the border, and no load needs a branch.
// The match.  mm_match_kernel, one workgroup per (query, angle, block of translation rows): the cloud goes through LDS in chunks of
// MM_CHUNK points.  A point becomes its cell (u, v) once per workgroup - three multiplies, three additions and a division per axis in
// float64, nothing after that is floating point.  A point whose whole window of shifts lies inside the bordered field is stored as its
// byte offset and costs an addition per load; one whose window is cut by the border keeps (u, v) and is clamped per load; one whose
// window misses the grid, or that is far, is dropped.  Which list a point is on is the same for every lane, so neither loop diverges.
// The candidates of the row block are numbered row-major, candidate c = t + j MM_THREADS is accumulator j of thread t: the 64 loads of
// a wavefront for one point are consecutive bytes of one field row (or of a few rows where the window is narrow), and the LDS read of
// the point is one address on every lane, a broadcast.  A score is a sum of bytes in a uint32.
// The best candidate of a query is the maximum of (score << 32 | ~flat index) over everything: per thread, then an LDS atomic, then one
// global atomic per workgroup - integers, so no order shows.  mm_finish_kernel, one workgroup per query, unpacks it and counts the
// points inside the grid at the best candidate.
#include "loop.h"
#include "map_match.h"

#define MM_CHUNK 2048                            // points in LDS at a time
#define MM_FAR 1073741824.0                      // 2^30
#define MM_MAX_QUERIES 65535                     // grid.y

struct roam_map_field {
    roam_ctx *ctx = nullptr;
    double ox = 0.0, oy = 0.0, res = 0.0;
    int W = 0, H = 0;
    uint8_t *pad = nullptr;      // (H + 2) x (W + 2): the field with its zero border
};

struct MmTable {
    uint8_t t[(2 * ROAM_MATCH_MAX_RADIUS + 1) * (2 * ROAM_MATCH_MAX_RADIUS + 1)];
};

struct MmField {
    const uint8_t *pad;
    double ox, oy, res;
    int W, H, Wp;
};

// the clouds, the priors and the window of a call, device pointers
struct MmQuery {
    const double *pts;           // the points of every cloud
    const int64_t *start;        // n_query: the first point of cloud q, in points
    const int32_t *count;        // n_query
    const double *priors;        // n_query x 3
    const double *cs;            // n_query x n_theta x 2
    int n_theta, kx, ky;
};

// ---------------------------------------------------------------------------------------------------------------- device
// pad (Hp x Wp) from the grids: the border zero, inside the maximum of the table over the occupied cells within the radius
__global__ __launch_bounds__(MM_THREADS) void mm_field_kernel(const uint32_t *__restrict__ hits, const uint32_t *__restrict__ views, int W, int H,
                                                              uint32_t min_hits, uint32_t min_views, int radius, MmTable tab, uint8_t *__restrict__ pad)
{
    const int Wp = W + 2;
    const int64_t cell = (int64_t)blockIdx.x * MM_THREADS + threadIdx.x;
    if (cell >= (int64_t)Wp * (H + 2)) return;
    const int u = (int)(cell % Wp) - 1, v = (int)(cell / Wp) - 1;
    uint32_t best = 0;
    if (u >= 0 && u < W && v >= 0 && v < H) {
        const int side = 2 * radius + 1;
        const int v0 = max(v - radius, 0), v1 = min(v + radius, H - 1), u0 = max(u - radius, 0), u1 = min(u + radius, W - 1);
        for (int y = v0; y <= v1; ++y)
            for (int x = u0; x <= u1; ++x) {
                const int64_t c = (int64_t)y * W + x;
                if (hits[c] >= min_hits && views[c] >= min_views) best = max(best, (uint32_t)tab.t[(y - v + radius) * side + (x - u + radius)]);
            }
    }
    pad[cell] = (uint8_t)best;
}

// the cell of point p of a cloud at the pose (c, s, x0, y0); false: the point is far
__device__ static inline bool mm_cell(const MmField &f, const double *__restrict__ pts, int64_t p, double c, double s, double x0, double y0, int *u, int *v)
{
    const double px = pts[2 * p], py = pts[2 * p + 1];
    const double wx = ((c * px) - (s * py)) + x0, wy = ((s * px) + (c * py)) + y0;
    const double dx = (wx - f.ox) / f.res, dy = (wy - f.oy) / f.res;
    if (!(dx >= -MM_FAR && dx < MM_FAR && dy >= -MM_FAR && dy < MM_FAR)) return false;
    *u = (int)floor(dx);
    *v = (int)floor(dy);
    return true;
}

// the n_whole points whose windows lie inside the bordered field (cell[p].x: the byte offset of the unshifted cell) and the n_cut points
// cut by the border (from the end of the list backwards: (u, v)) into the NACC accumulators of this thread
template <int NACC>
__device__ static inline void mm_accumulate(const MmField &f, const int2 *cell, int n_whole, int n_cut, const int *off, const int *da, const int *db,
                                            uint32_t *acc)
{
    const uint8_t *__restrict__ pad = f.pad;
#pragma unroll 4
    for (int p = 0; p < n_whole; ++p) {
        const int base = cell[p].x;
#pragma unroll
        for (int j = 0; j < NACC; ++j) acc[j] += pad[base + off[j]];
    }
    for (int p = 0; p < n_cut; ++p) {
        const int2 uv = cell[MM_CHUNK - 1 - p];
#pragma unroll
        for (int j = 0; j < NACC; ++j) {
            const int x = min(max(uv.x + da[j], -1), f.W), y = min(max(uv.y + db[j], -1), f.H);
            acc[j] += pad[(y + 1) * f.Wp + (x + 1)];
        }
    }
}

// see the head of the file.  blockIdx.x = blk n_theta + i, blockIdx.y = q; keys (n_query) zero before the launch; scores may be null
__global__ __launch_bounds__(MM_THREADS) void mm_match_kernel(MmField f, MmQuery m, int rows_per_wg, unsigned long long *__restrict__ keys,
                                                              uint32_t *__restrict__ scores)
{
    __shared__ int2 cell[MM_CHUNK];
    __shared__ int n_list[2];                    // the points on the two lists of the chunk
    __shared__ unsigned long long best_key;
    const int t = threadIdx.x, q = blockIdx.y, i = blockIdx.x % m.n_theta, blk = blockIdx.x / m.n_theta;
    const int rowlen = 2 * m.kx + 1, nb = 2 * m.ky + 1, b0 = blk * rows_per_wg;
    const int ncand = min(rows_per_wg, nb - b0) * rowlen, nacc = (ncand + MM_THREADS - 1) / MM_THREADS;
    const int n = m.count[q];
    const double *pts = m.pts + 2 * m.start[q];
    const double c = m.cs[2 * ((int64_t)q * m.n_theta + i)], s = m.cs[2 * ((int64_t)q * m.n_theta + i) + 1];
    const double x0 = m.priors[3 * q], y0 = m.priors[3 * q + 1];
    int off[MM_ACC], da[MM_ACC], db[MM_ACC];
    uint32_t acc[MM_ACC];
#pragma unroll
    for (int j = 0; j < MM_ACC; ++j) {
        const int cand = t + j * MM_THREADS;
        const bool live = cand < ncand;          // a dead accumulator reads the unshifted cell and is never written
        da[j] = live ? cand % rowlen - m.kx : 0;
        db[j] = live ? b0 + cand / rowlen - m.ky : 0;
        off[j] = db[j] * f.Wp + da[j];
        acc[j] = 0;
    }
    if (t == 0) best_key = 0;
    for (int first = 0; first < n; first += MM_CHUNK) {
        __syncthreads();                         // the previous chunk has been read
        if (t < 2) n_list[t] = 0;
        __syncthreads();
        for (int p = first + t; p < min(first + MM_CHUNK, n); p += MM_THREADS) {
            int u, v;
            if (!mm_cell(f, pts, p, c, s, x0, y0, &u, &v)) continue;
            if (u + m.kx < 0 || u - m.kx >= f.W || v + m.ky < 0 || v - m.ky >= f.H) continue;     // no shift of the window takes it into the grid
            if (u - m.kx >= -1 && u + m.kx <= f.W && v - m.ky >= -1 && v + m.ky <= f.H)
                cell[atomicAdd(&n_list[0], 1)] = make_int2((v + 1) * f.Wp + (u + 1), 0);
            else
                cell[MM_CHUNK - 1 - atomicAdd(&n_list[1], 1)] = make_int2(u, v);
        }
        __syncthreads();
        const int n_whole = n_list[0], n_cut = n_list[1];
        switch (nacc) {
        case 1: mm_accumulate<1>(f, cell, n_whole, n_cut, off, da, db, acc); break;
        case 2: mm_accumulate<2>(f, cell, n_whole, n_cut, off, da, db, acc); break;
        case 3: mm_accumulate<3>(f, cell, n_whole, n_cut, off, da, db, acc); break;
        case 4: mm_accumulate<4>(f, cell, n_whole, n_cut, off, da, db, acc); break;
        case 5: mm_accumulate<5>(f, cell, n_whole, n_cut, off, da, db, acc); break;
        case 6: mm_accumulate<6>(f, cell, n_whole, n_cut, off, da, db, acc); break;
        case 7: mm_accumulate<7>(f, cell, n_whole, n_cut, off, da, db, acc); break;
        default: mm_accumulate<8>(f, cell, n_whole, n_cut, off, da, db, acc); break;
        }
    }
    // the scores, and the best candidate of the workgroup
    const int64_t slab = ((int64_t)q * m.n_theta + i) * nb * rowlen + (int64_t)b0 * rowlen;       // the flat index of candidate 0, query included
    const uint32_t flat0 = (uint32_t)((i * nb + b0) * rowlen);
    unsigned long long key = 0;
#pragma unroll
    for (int j = 0; j < MM_ACC; ++j) {
        const int cand = t + j * MM_THREADS;
        if (cand >= ncand) continue;
        if (scores) scores[slab + cand] = acc[j];
        const unsigned long long k = (unsigned long long)acc[j] << 32 | (uint32_t)~(flat0 + (uint32_t)cand);
        key = k > key ? k : key;
    }
    __syncthreads();                             // best_key = 0 is visible (a cloud without points has passed no barrier yet)
    if (key) atomicMax(&best_key, key);
    __syncthreads();
    if (t == 0) atomicMax(keys + q, best_key);
}

// info (n_query, 6): score, i, b, a, n_points, n_inside from the key of every query
__global__ __launch_bounds__(MM_THREADS) void mm_finish_kernel(MmField f, MmQuery m, const unsigned long long *__restrict__ keys, int32_t *__restrict__ info)
{
    __shared__ int inside;
    const int t = threadIdx.x, q = blockIdx.x;
    const int rowlen = 2 * m.kx + 1, nb = 2 * m.ky + 1;
    const unsigned long long key = keys[q];
    const uint32_t flat = ~(uint32_t)key;
    const int i = (int)(flat / (uint32_t)(nb * rowlen)), b = (int)(flat / (uint32_t)rowlen) % nb, a = (int)(flat % (uint32_t)rowlen);
    const int n = m.count[q];
    const double *pts = m.pts + 2 * m.start[q];
    const double c = m.cs[2 * ((int64_t)q * m.n_theta + i)], s = m.cs[2 * ((int64_t)q * m.n_theta + i) + 1];
    if (t == 0) inside = 0;
    __syncthreads();
    int mine = 0;
    for (int p = t; p < n; p += MM_THREADS) {
        int u, v;
        if (!mm_cell(f, pts, p, c, s, m.priors[3 * q], m.priors[3 * q + 1], &u, &v)) continue;
        const int x = u + (a - m.kx), y = v + (b - m.ky);
        mine += x >= 0 && x < f.W && y >= 0 && y < f.H;
    }
    if (mine) atomicAdd(&inside, mine);
    __syncthreads();
    if (t == 0) {
        int32_t *o = info + 6 * q;
        o[0] = (int32_t)(key >> 32); o[1] = i; o[2] = b; o[3] = a; o[4] = n; o[5] = inside;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
// The uploads of an entry come from host memory that the entry owns (h_lists, the counts) or that the caller gets back when it returns:
// declared after them, this waits for the stream on every path that has not done so itself
struct MmDrain {
    hipStream_t st;
    bool armed = true;
    ~MmDrain() { if (armed) (void)hipStreamSynchronize(st); }
};

extern "C" int32_t roam_map_field_table(double sigma_cells, int32_t radius, uint8_t *table_out)
{
    return map_field_table(sigma_cells, radius, table_out) ? ROAM_OK : ROAM_E_ARG;
}

extern "C" int32_t roam_map_match_angles(int32_t n_query, const double *priors, int32_t n_theta, double step_rad, double *cs_out)
{
    if (!cs_out || !map_match_check_window(nullptr, 0, n_query, priors, n_theta, step_rad, 0, 0, false)) return ROAM_E_ARG;
    map_match_angle_table(n_query, priors, n_theta, step_rad, cs_out);
    return ROAM_OK;
}

extern "C" int32_t roam_map_match_plan(int32_t cu_count, int32_t n_query, int32_t n_theta, int32_t kx, int32_t ky, int32_t *rows_out, int32_t *n_blk_out)
{
    const double none[3] = {0.0, 0.0, 0.0};
    if (!rows_out || !n_blk_out || cu_count < 1 || n_query < 1 || n_query > MM_MAX_QUERIES) return ROAM_E_ARG;
    if (!map_match_check_window(nullptr, 0, 1, none, n_theta, 0.0, kx, ky, false)) return ROAM_E_ARG;
    map_match_plan(cu_count, n_query, n_theta, kx, ky, map_match_rows_env(), rows_out, n_blk_out);
    return ROAM_OK;
}

static MmTable mm_table(int radius, const uint8_t *table)
{
    MmTable t;
    memset(&t, 0, sizeof(t));
    memcpy(t.t, table, (size_t)(2 * radius + 1) * (2 * radius + 1));
    return t;
}

// the grids (S_TMP0: hits, then views) -> pad
static hipError_t mm_launch_field(hipStream_t st, const uint32_t *d_grids, int W, int H, int min_hits, int min_views, int radius, const MmTable &tab,
                                  uint8_t *pad)
{
    const int64_t cells = (int64_t)(W + 2) * (H + 2);
    hipLaunchKernelGGL(mm_field_kernel, dim3((unsigned)((cells + MM_THREADS - 1) / MM_THREADS)), dim3(MM_THREADS), 0, st, d_grids, d_grids + (size_t)W * H,
                       W, H, (uint32_t)min_hits, (uint32_t)min_views, radius, tab, pad);
    return hipGetLastError();
}

static int32_t mm_upload_grids(roam_ctx *ctx, const uint32_t *hits, const uint32_t *views, int W, int H, uint32_t **d_grids)
{
    const size_t cells = (size_t)W * H;
    uint32_t *g = (uint32_t *)roam_scratch(ctx, S_TMP0, sizeof(uint32_t) * 2 * cells);
    if (!g) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(g, hits, sizeof(uint32_t) * cells, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(g + cells, views, sizeof(uint32_t) * cells, hipMemcpyHostToDevice, ctx->stream));
    *d_grids = g;
    return ROAM_OK;
}

extern "C" int32_t roam_map_field_create(roam_ctx *ctx, double ox, double oy, double res, int32_t W, int32_t H, const uint32_t *hits,
                                         const uint32_t *views, int32_t min_hits, int32_t min_views, int32_t radius, const uint8_t *table,
                                         roam_map_field **field_out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!hits || !views || !table || !field_out) {
        ROAM_SET_ERR(ctx, "map field: %s is null", !hits ? "hits" : !views ? "views" : !table ? "table" : "field_out");
        return ROAM_E_ARG;
    }
    if (!map_field_check(ctx->err, sizeof(ctx->err), ox, oy, res, W, H, min_hits, min_views, radius)) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t *d_grids = nullptr;
    {
        MmDrain drain{ctx->stream};              // a second copy that fails must not leave the first reading the caller's grid
        LOOP_TRY(mm_upload_grids(ctx, hits, views, W, H, &d_grids));
        drain.armed = false;
    }
    roam_map_field *f = new roam_map_field;
    f->ctx = ctx; f->ox = ox; f->oy = oy; f->res = res; f->W = W; f->H = H;
    hipError_t e = hipMalloc(&f->pad, (size_t)(W + 2) * (H + 2));
    if (e == hipSuccess) e = mm_launch_field(ctx->stream, d_grids, W, H, min_hits, min_views, radius, mm_table(radius, table), f->pad);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // hits and views are the caller's again
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream); // hits and views are the caller's again on this path too
        ROAM_SET_ERR(ctx, "map field: building %d x %d cells failed: %s", W, H, hipGetErrorString(e));
        if (f->pad) (void)hipFree(f->pad);
        delete f;
        return ROAM_E_HIP;
    }
    *field_out = f;
    return ROAM_OK;
}

// what every entry that takes a field refuses first
static int32_t mm_check_field(roam_ctx *ctx, const roam_map_field *field)
{
    if (!field) { ROAM_SET_ERR(ctx, "map match: field is null"); return ROAM_E_ARG; }
    if (field->ctx != ctx) { ROAM_SET_ERR(ctx, "map match: field was made on another context"); return ROAM_E_ARG; }
    return ROAM_OK;
}

extern "C" int32_t roam_map_field_read(roam_ctx *ctx, roam_map_field *field, uint8_t *out)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(mm_check_field(ctx, field));
    if (!out) { ROAM_SET_ERR(ctx, "map field: out is null"); return ROAM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t Wp = (size_t)field->W + 2;
    HIP_TRY(ctx, hipMemcpy2DAsync(out, (size_t)field->W, field->pad + Wp + 1, Wp, (size_t)field->W, (size_t)field->H, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

extern "C" int32_t roam_map_field_destroy(roam_ctx *ctx, roam_map_field *field)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(mm_check_field(ctx, field));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // nothing enqueued reads it any more
    HIP_TRY(ctx, hipFree(field->pad));
    delete field;
    return ROAM_OK;
}

// the device side of one match: the query lists and the table (S_IN0), the keys and the records (S_OUT0), the volume (S_OUT1)
struct MmBufs {
    MmField f;
    MmQuery m;
    int n_query, rows_per_wg, n_blk;
    unsigned long long *keys;
    int32_t *info;
    uint32_t *scores;            // null: no volume
    int64_t volume;              // entries of the volume
    std::vector<char> h_lists;   // the host side of S_IN0 while its upload is in flight
};

// the checks have passed.  start / count (host, n_query each): the clouds inside d_pts
static int32_t mm_stage(roam_ctx *ctx, const roam_map_field *field, const double *d_pts, int n_query, const int64_t *start, const int32_t *count,
                        const double *priors, int n_theta, double step_rad, int kx, int ky, bool with_volume, MmBufs *b)
{
    const size_t nq = (size_t)n_query, n_cs = 2 * nq * n_theta;
    // start (8 nq), priors (24 nq), cs (8 n_cs), count (4 nq)
    b->h_lists.resize(8 * nq + 24 * nq + 8 * n_cs + 4 * nq);
    char *h = b->h_lists.data();
    memcpy(h, start, 8 * nq);
    memcpy(h + 8 * nq, priors, 24 * nq);
    map_match_angle_table(n_query, priors, n_theta, step_rad, (double *)(h + 32 * nq));
    memcpy(h + 32 * nq + 8 * n_cs, count, 4 * nq);
    const int rowlen = 2 * kx + 1, nb = 2 * ky + 1;
    b->volume = (int64_t)n_query * n_theta * nb * rowlen;
    char *d = (char *)roam_scratch(ctx, S_IN0, b->h_lists.size());
    char *out = (char *)roam_scratch(ctx, S_OUT0, (8 + 24) * nq);
    b->scores = with_volume ? (uint32_t *)roam_scratch(ctx, S_OUT1, sizeof(uint32_t) * (size_t)b->volume) : nullptr;
    if (!d || !out || (with_volume && !b->scores)) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(d, h, b->h_lists.size(), hipMemcpyHostToDevice, ctx->stream));
    b->f = MmField{field->pad, field->ox, field->oy, field->res, field->W, field->H, field->W + 2};
    b->m = MmQuery{d_pts, (const int64_t *)d, (const int32_t *)(d + 32 * nq + 8 * n_cs), (const double *)(d + 8 * nq), (const double *)(d + 32 * nq), n_theta, kx, ky};
    b->n_query = n_query;
    b->keys = (unsigned long long *)out;
    b->info = (int32_t *)(out + 8 * nq);
    map_match_plan(ctx->cu_count, n_query, n_theta, kx, ky, map_match_rows_env(), &b->rows_per_wg, &b->n_blk);
    return ROAM_OK;
}

static hipError_t mm_launch_match(hipStream_t st, const MmBufs &b)
{
    const hipError_t e = hipMemsetAsync(b.keys, 0, sizeof(unsigned long long) * (size_t)b.n_query, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mm_match_kernel, dim3((unsigned)(b.n_blk * b.m.n_theta), (unsigned)b.n_query), dim3(MM_THREADS), 0, st, b.f, b.m, b.rows_per_wg, b.keys,
                       b.scores);
    hipLaunchKernelGGL(mm_finish_kernel, dim3((unsigned)b.n_query), dim3(MM_THREADS), 0, st, b.f, b.m, b.keys, b.info);
    return hipGetLastError();
}

// the read-back, and the poses of the best candidates
static int32_t mm_download(roam_ctx *ctx, const MmBufs &b, const double *priors, double step_rad, double *pose_out, int32_t *info_out, uint32_t *scores_out)
{
    HIP_TRY(ctx, hipMemcpyAsync(info_out, b.info, sizeof(int32_t) * 6 * (size_t)b.n_query, hipMemcpyDeviceToHost, ctx->stream));
    if (scores_out) HIP_TRY(ctx, hipMemcpyAsync(scores_out, b.scores, sizeof(uint32_t) * (size_t)b.volume, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t q = 0; q < b.n_query; ++q) {
        const int32_t *o = info_out + 6 * q;
        pose_out[3 * q] = priors[3 * q] + (double)(o[3] - b.m.kx) * b.f.res;
        pose_out[3 * q + 1] = priors[3 * q + 1] + (double)(o[2] - b.m.ky) * b.f.res;
        pose_out[3 * q + 2] = map_match_theta(priors[3 * q + 2], o[1], b.m.n_theta, step_rad);
    }
    return ROAM_OK;
}

static int32_t mm_check_match(roam_ctx *ctx, const roam_map_field *field, int32_t n_query, const double *priors, int32_t n_theta, double step_rad, int32_t kx,
                              int32_t ky, const double *pose_out, const int32_t *info_out, bool with_volume)
{
    LOOP_TRY(mm_check_field(ctx, field));
    if (!map_match_check_window(ctx->err, sizeof(ctx->err), n_query, priors, n_theta, step_rad, kx, ky, with_volume)) return ROAM_E_ARG;
    if (n_query > MM_MAX_QUERIES) { ROAM_SET_ERR(ctx, "map match: n_query at most %d, not %d", MM_MAX_QUERIES, n_query); return ROAM_E_ARG; }
    if (!pose_out || !info_out) { ROAM_SET_ERR(ctx, "map match: %s is null", !pose_out ? "pose_out" : "info_out"); return ROAM_E_ARG; }
    return ROAM_OK;
}

// the clouds of a host call to the device (S_IN1) -> *d_pts, and their counts
static int32_t mm_upload_clouds(roam_ctx *ctx, int n_query, const double *xy, const int64_t *offsets, const double **d_pts, std::vector<int32_t> *count)
{
    count->resize((size_t)n_query);
    for (int q = 0; q < n_query; ++q) (*count)[q] = (int32_t)(offsets[q + 1] - offsets[q]);
    const size_t bytes = sizeof(double) * 2 * (size_t)offsets[n_query];
    double *d = (double *)roam_scratch(ctx, S_IN1, bytes ? bytes : 16);
    if (!d) return ROAM_E_HIP;
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(d, xy, bytes, hipMemcpyHostToDevice, ctx->stream));
    *d_pts = d;
    return ROAM_OK;
}

extern "C" int32_t roam_map_match_clouds(roam_ctx *ctx, roam_map_field *field, int32_t n_query, const double *xy, const int64_t *offsets,
                                         const double *priors, int32_t n_theta, double step_rad, int32_t kx, int32_t ky, double *pose_out,
                                         int32_t *info_out, uint32_t *scores_out)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(mm_check_match(ctx, field, n_query, priors, n_theta, step_rad, kx, ky, pose_out, info_out, scores_out != nullptr));
    if (!map_match_check_clouds(ctx->err, sizeof(ctx->err), n_query, xy, offsets)) return ROAM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const double *d_pts = nullptr;
    std::vector<int32_t> count;
    MmBufs b;
    MmDrain drain{ctx->stream};
    LOOP_TRY(mm_upload_clouds(ctx, n_query, xy, offsets, &d_pts, &count));
    LOOP_TRY(mm_stage(ctx, field, d_pts, n_query, offsets, count.data(), priors, n_theta, step_rad, kx, ky, scores_out != nullptr, &b));
    HIP_TRY(ctx, mm_launch_match(ctx->stream, b));
    const int32_t rc = mm_download(ctx, b, priors, step_rad, pose_out, info_out, scores_out);
    drain.armed = rc != ROAM_OK;                 // a download that returned ROAM_OK has waited for the stream
    return rc;
}

extern "C" int32_t roam_loop_db_map_match(roam_ctx *ctx, roam_loop_db *db, roam_map_field *field, int32_t n_query, const int32_t *index,
                                          const double *priors, int32_t n_theta, double step_rad, int32_t kx, int32_t ky, double *pose_out,
                                          int32_t *info_out, uint32_t *scores_out)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db) { ROAM_SET_ERR(ctx, "map match: db is null"); return ROAM_E_ARG; }
    if (!db->cloud_rows) { ROAM_SET_ERR(ctx, "map match: db keeps no clouds (roam_loop_db_keep_clouds)"); return ROAM_E_STATE; }
    if (db->owner != ctx) { ROAM_SET_ERR(ctx, "map match: db was made on another context"); return ROAM_E_ARG; }
    LOOP_TRY(mm_check_match(ctx, field, n_query, priors, n_theta, step_rad, kx, ky, pose_out, info_out, scores_out != nullptr));
    if (!index) { ROAM_SET_ERR(ctx, "map match: index is null"); return ROAM_E_ARG; }
    std::vector<int64_t> start((size_t)n_query);
    std::vector<int32_t> count((size_t)n_query);
    const int cap = db->max_points < ROAM_ICP_MAX_POINTS ? db->max_points : ROAM_ICP_MAX_POINTS;
    for (int q = 0; q < n_query; ++q) {
        if (index[q] < 0 || index[q] >= db->count) {
            ROAM_SET_ERR(ctx, "map match: index of query %d: entry %d outside the %d stored", q, index[q], db->count);
            return ROAM_E_ARG;
        }
        const int n = db->h_n[index[q]];
        start[q] = (int64_t)index[q] * db->max_points;
        count[q] = n < 0 ? 0 : n > cap ? cap : n;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MmBufs b;
    MmDrain drain{ctx->stream};
    LOOP_TRY(mm_stage(ctx, field, db->cloud, n_query, start.data(), count.data(), priors, n_theta, step_rad, kx, ky, scores_out != nullptr, &b));
    HIP_TRY(ctx, mm_launch_match(ctx->stream, b));
    const int32_t rc = mm_download(ctx, b, priors, step_rad, pose_out, info_out, scores_out);
    drain.armed = rc != ROAM_OK;
    return rc;
}

extern "C" int32_t roam_time_map_match(roam_ctx *ctx, roam_map_field *field, const uint32_t *hits, const uint32_t *views, int32_t min_hits,
                                       int32_t min_views, int32_t radius, const uint8_t *table, int32_t n_query, const double *xy,
                                       const int64_t *offsets, const double *priors, int32_t n_theta, double step_rad, int32_t kx, int32_t ky,
                                       int32_t reps, float *ms)
{
    if (!ctx) return ROAM_E_ARG;
    double pose_unused = 0.0;
    int32_t info_unused = 0;
    LOOP_TRY(mm_check_match(ctx, field, n_query, priors, n_theta, step_rad, kx, ky, &pose_unused, &info_unused, false));
    if (!map_match_check_clouds(ctx->err, sizeof(ctx->err), n_query, xy, offsets)) return ROAM_E_ARG;
    if (!hits || !views || !table) { ROAM_SET_ERR(ctx, "map field: %s is null", !hits ? "hits" : !views ? "views" : "table"); return ROAM_E_ARG; }
    if (!map_field_check(ctx->err, sizeof(ctx->err), field->ox, field->oy, field->res, field->W, field->H, min_hits, min_views, radius)) return ROAM_E_ARG;
    ARG_CHECK(ctx, reps >= 1 && ms);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const double *d_pts = nullptr;
    std::vector<int32_t> count;
    MmBufs b;
    MmDrain drain{st};                           // roam_time_launches waits when it succeeds; a second wait costs nothing
    // the field's build, into scratch: the handle's field stays as it is
    uint32_t *d_grids = nullptr;
    LOOP_TRY(mm_upload_grids(ctx, hits, views, field->W, field->H, &d_grids));
    uint8_t *pad = (uint8_t *)roam_scratch(ctx, S_TMP1, (size_t)(field->W + 2) * (field->H + 2));
    if (!pad) return ROAM_E_HIP;
    const MmTable tab = mm_table(radius, table);
    LOOP_TRY(roam_time_launches(ctx, st, reps, ms, [&] { return mm_launch_field(st, d_grids, field->W, field->H, min_hits, min_views, radius, tab, pad); }));
    LOOP_TRY(mm_upload_clouds(ctx, n_query, xy, offsets, &d_pts, &count));
    LOOP_TRY(mm_stage(ctx, field, d_pts, n_query, offsets, count.data(), priors, n_theta, step_rad, kx, ky, false, &b));
    return roam_time_launches(ctx, st, reps, ms + 1, [&] { return mm_launch_match(st, b); });
}
