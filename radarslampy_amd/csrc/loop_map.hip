// The global map: the loop database's resident peak clouds binned at given poses.  Map of the family: loop.h; the definition:
// include/roam_abi.h ("global map"), the contract tests/global_map_model.py.
//
// A point of entry e goes to the world frame with the entry's pose (the cosine and sine come from the host's libm, the device only
// multiplies) and into a cell of the caller's grid.  What a cell accumulates are integers - hits, the distinct entries (views) and
// the sums of the 16-bit sub-cell positions - so the result does not depend on the order of arrival, and every atomic is an integer
// one.  map_splat_kernel, one workgroup per entry: a point becomes the 64-bit item (cell key << 32 | qx << 16 | qy), one key for
// everything outside; the items are sorted in LDS (bitonic, 8192 x 8 bytes), and a run of equal keys then adds its length and its two
// sums once and counts one view - the workgroup is the entry, so the distinct-entry count needs no word between workgroups.  A run is
// cut at every MAP_SEG-th item so that no lane walks more than MAP_SEG items: a cut run adds its pieces apart (sums of integers), the
// view still once, at the run's head.  The compaction treats the grid as the row-major array it is, in chunks of MAP_CHUNK cells: a
// count per chunk, an exclusive scan over the chunks, then the write - row-major order (v major) by construction, whatever W and H.
// The grid and every other buffer of a call is scratch of the context: the database keeps no map.
#include "loop.h"
#include "peaks_common.h"
#include <cmath>

#define MAP_THREADS 512                          // map_splat_kernel
#define MAP_SEG 16                               // the longest piece of a run one lane adds
#define MAP_RED_THREADS 256                      // the bounds kernel and the compaction
#define MAP_CELLS_PER_LANE 8
#define MAP_CHUNK (MAP_RED_THREADS * MAP_CELLS_PER_LANE)     // cells per chunk of the compaction
#define MAP_SCAN_THREADS 1024                    // map_scan_kernel: one workgroup, at most 2^26 / MAP_CHUNK = 32768 chunks
#define MAP_OUTSIDE 0xffffffffu                  // the key of a point outside the extent (a cell key is below 2^26)

// the clouds and the poses of a call, device pointers
struct MapSrc {
    const double *cloud;         // db->cloud
    const int32_t *cloud_n;
    int max_points;
    const double *poses;         // count x 3
    const double *cs;            // count x 2: cos theta, sin theta
    const int8_t *use;           // count, or null: every entry
};

struct MapGrid {
    unsigned long long *sx, *sy; // W H each
    uint32_t *hits, *views;
    double res, ox, oy;
    int W, H;
};

// ---------------------------------------------------------------------------------------------------------------- device
// the points entry e contributes: 0 for an entry left out
__device__ static inline int map_entry_points(const MapSrc &m, int64_t e)
{
    if (m.use && !m.use[e]) return 0;
    const int n = m.cloud_n[e], cap = m.max_points < ROAM_ICP_MAX_POINTS ? m.max_points : ROAM_ICP_MAX_POINTS;
    return n < 0 ? 0 : n > cap ? cap : n;
}

struct MapPose {
    double c, s, x, y;
};

__device__ static inline MapPose map_pose(const MapSrc &m, int64_t e) { return MapPose{m.cs[2 * e], m.cs[2 * e + 1], m.poses[3 * e], m.poses[3 * e + 1]}; }
__device__ static inline double map_wx(const MapPose &p, double px, double py) { return ((p.c * px) - (p.s * py)) + p.x; }
__device__ static inline double map_wy(const MapPose &p, double px, double py) { return ((p.s * px) + (p.c * py)) + p.y; }

// doubles as unsigned integers of the same order, so that the extremes are integer atomics
__host__ __device__ static inline unsigned long long map_order_key(double d)
{
    unsigned long long b;
    memcpy(&b, &d, sizeof(b));
    return b >> 63 ? ~b : b | 0x8000000000000000ull;
}

__host__ static inline double map_order_value(unsigned long long k)
{
    const unsigned long long b = k >> 63 ? k & 0x7fffffffffffffffull : ~k;
    double d;
    memcpy(&d, &b, sizeof(d));
    return d;
}

// keys: min wx, max wx, min wy, max wy as map_order_key, preset to +inf / -inf.  A zero is +0 (w + 0.0)
__global__ __launch_bounds__(MAP_RED_THREADS) void map_bounds_kernel(MapSrc m, unsigned long long *__restrict__ keys)
{
    __shared__ unsigned long long sh[4];
    const int64_t e = blockIdx.x;
    const int n = map_entry_points(m, e), t = threadIdx.x;
    if (n == 0) return;
    if (t < 4) sh[t] = map_order_key(t & 1 ? -INFINITY : INFINITY);
    __syncthreads();
    const MapPose p = map_pose(m, e);
    const double *pts = m.cloud + 2 * e * m.max_points;
    double lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
    for (int i = t; i < n; i += MAP_RED_THREADS) {
        const double px = pts[2 * i], py = pts[2 * i + 1];
        const double wx = map_wx(p, px, py) + 0.0, wy = map_wy(p, px, py) + 0.0;
        lox = wx < lox ? wx : lox;
        hix = wx > hix ? wx : hix;
        loy = wy < loy ? wy : loy;
        hiy = wy > hiy ? wy : hiy;
    }
    if (t < n) {
        atomicMin(&sh[0], map_order_key(lox));
        atomicMax(&sh[1], map_order_key(hix));
        atomicMin(&sh[2], map_order_key(loy));
        atomicMax(&sh[3], map_order_key(hiy));
    }
    __syncthreads();
    if (t < 4) {
        if (t & 1) atomicMax(keys + t, sh[t]);
        else atomicMin(keys + t, sh[t]);
    }
}

// see the head of the file.  The grid must be zero before the first entry is added
__global__ __launch_bounds__(MAP_THREADS) void map_splat_kernel(MapSrc m, MapGrid g, unsigned long long *__restrict__ n_outside)
{
    __shared__ unsigned long long item[ROAM_ICP_MAX_POINTS];
    const int64_t e = blockIdx.x;
    const int n = map_entry_points(m, e), t = threadIdx.x;
    if (n == 0) return;
    int P = 2;
    while (P < n) P <<= 1;                                // <= ROAM_ICP_MAX_POINTS, a power of two
    const MapPose p = map_pose(m, e);
    const double *pts = m.cloud + 2 * e * m.max_points;
    const double Wd = (double)g.W, Hd = (double)g.H;
    uint32_t out = 0;
    for (int i = t; i < P; i += MAP_THREADS) {
        unsigned long long it = ~0ull;                    // the padding sorts behind everything, with the points outside
        if (i < n) {
            const double px = pts[2 * i], py = pts[2 * i + 1];
            const double dx = (map_wx(p, px, py) - g.ox) / g.res, dy = (map_wy(p, px, py) - g.oy) / g.res;
            if (dx >= 0.0 && dx < Wd && dy >= 0.0 && dy < Hd) {
                const double fu = floor(dx), fv = floor(dy);
                const uint32_t qx = (uint32_t)floor((dx - fu) * 65536.0), qy = (uint32_t)floor((dy - fv) * 65536.0);
                const uint32_t key = (uint32_t)fv * (uint32_t)g.W + (uint32_t)fu;
                it = (unsigned long long)key << 32 | qx << 16 | qy;
            } else {
                ++out;
            }
        }
        item[i] = it;
    }
    if (out) atomicAdd(n_outside, (unsigned long long)out);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = t; q < P / 2; q += MAP_THREADS) {
                const int i = (q & ~(j - 1)) << 1 | (q & (j - 1)), o = i | j;
                const unsigned long long a = item[i], b = item[o];
                if ((a > b) == ((i & k) == 0)) {
                    item[i] = b;
                    item[o] = a;
                }
            }
            __syncthreads();
        }
    for (int i = t; i < n; i += MAP_THREADS) {
        const uint32_t key = (uint32_t)(item[i] >> 32);
        if (key == MAP_OUTSIDE) continue;
        const bool head = i == 0 || (uint32_t)(item[i - 1] >> 32) != key;
        if (!head && i % MAP_SEG) continue;
        uint32_t len = 0;
        unsigned long long ax = 0, ay = 0;
        int j = i;
        do {
            const uint32_t q = (uint32_t)item[j];
            ax += q >> 16;
            ay += q & 0xffffu;
            ++len;
            ++j;
        } while (j < n && j % MAP_SEG && (uint32_t)(item[j] >> 32) == key);
        atomicAdd(g.hits + key, len);
        atomicAdd(g.sx + key, ax);
        atomicAdd(g.sy + key, ay);
        if (head) atomicAdd(g.views + key, 1u);
    }
}

// the qualifying cells among the MAP_CELLS_PER_LANE cells from `first` on, as a bit mask
__device__ static inline uint32_t map_qualifying(const uint32_t *__restrict__ hits, const uint32_t *__restrict__ views, int64_t first, int64_t cells,
                                                 uint32_t min_hits, uint32_t min_views)
{
    uint32_t mask = 0;
    for (int q = 0; q < MAP_CELLS_PER_LANE; ++q)
        if (first + q < cells && hits[first + q] >= min_hits && views[first + q] >= min_views) mask |= 1u << q;
    return mask;
}

__global__ __launch_bounds__(MAP_RED_THREADS) void map_count_kernel(const uint32_t *__restrict__ hits, const uint32_t *__restrict__ views, int64_t cells,
                                                                    uint32_t min_hits, uint32_t min_views, int32_t *__restrict__ chunk_count)
{
    __shared__ int sh[MAP_RED_THREADS / 64];
    const int64_t first = (int64_t)blockIdx.x * MAP_CHUNK + threadIdx.x * MAP_CELLS_PER_LANE;
    int total;
    (void)block_excl_scan(__popc(map_qualifying(hits, views, first, cells, min_hits, min_views)), sh, &total);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// one workgroup: chunk_off = the exclusive scan of chunk_count, *total = the number of map points
__global__ __launch_bounds__(MAP_SCAN_THREADS) void map_scan_kernel(const int32_t *__restrict__ chunk_count, int n_chunks, int32_t *__restrict__ chunk_off,
                                                                    int32_t *__restrict__ total)
{
    __shared__ int sh[MAP_SCAN_THREADS / 64];
    const int items = (n_chunks + MAP_SCAN_THREADS - 1) / MAP_SCAN_THREADS;
    const int lo = min((int)threadIdx.x * items, n_chunks), hi = min(lo + items, n_chunks);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += chunk_count[i];
    int tot;
    int off = block_excl_scan(c, sh, &tot);
    for (int i = lo; i < hi; ++i) {
        chunk_off[i] = off;
        off += chunk_count[i];
    }
    if (threadIdx.x == 0) *total = tot;
}

// the records of the qualifying cells, in cell order; nothing when they do not fit `room`
__global__ __launch_bounds__(MAP_RED_THREADS) void map_write_kernel(MapGrid g, int64_t cells, uint32_t min_hits, uint32_t min_views,
                                                                    const int32_t *__restrict__ chunk_off, const int32_t *__restrict__ total, int32_t room,
                                                                    double *__restrict__ pts, uint32_t *__restrict__ pt_hits, uint32_t *__restrict__ pt_views)
{
    __shared__ int sh[MAP_RED_THREADS / 64];
    if (*total > room) return;
    const int64_t first = (int64_t)blockIdx.x * MAP_CHUNK + threadIdx.x * MAP_CELLS_PER_LANE;
    const uint32_t mask = map_qualifying(g.hits, g.views, first, cells, min_hits, min_views);
    int tot;
    int64_t o = chunk_off[blockIdx.x] + block_excl_scan(__popc(mask), sh, &tot);
    for (int q = 0; q < MAP_CELLS_PER_LANE; ++q) {
        if (!(mask >> q & 1)) continue;
        const int64_t c = first + q;
        const uint32_t h = g.hits[c];
        const double den = 131072.0 * (double)h;
        const double mx = (double)(2 * g.sx[c] + h) / den, my = (double)(2 * g.sy[c] + h) / den;
        pts[2 * o] = g.ox + g.res * ((double)(c % g.W) + mx);
        pts[2 * o + 1] = g.oy + g.res * ((double)(c / g.W) + my);
        pt_hits[o] = h;
        pt_views[o] = g.views[c];
        ++o;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
static void map_pose_cs(int64_t n, const double *poses, double *cs)
{
    for (int64_t e = 0; e < n; ++e) {
        cs[2 * e] = cos(poses[3 * e + 2]);
        cs[2 * e + 1] = sin(poses[3 * e + 2]);
    }
}

extern "C" int32_t roam_map_pose_table(int32_t n, const double *poses, double *cs_out)
{
    if (n < 0 || (n > 0 && (!poses || !cs_out))) return ROAM_E_ARG;
    for (int64_t e = 0; e < n; ++e)
        if (!std::isfinite(poses[3 * e + 2])) return ROAM_E_ARG;
    map_pose_cs(n, poses, cs_out);
    return ROAM_OK;
}

extern "C" int32_t roam_map_plan(double minx, double maxx, double miny, double maxy, double res, double *ox, double *oy, int32_t *W, int32_t *H)
{
    if (!ox || !oy || !W || !H) return ROAM_E_ARG;
    if (!(std::isfinite(minx) && std::isfinite(maxx) && std::isfinite(miny) && std::isfinite(maxy)) || minx > maxx || miny > maxy) return ROAM_E_ARG;
    if (!(std::isfinite(res) && res > 0.0)) return ROAM_E_ARG;
    const double fx = floor(minx / res), fy = floor(miny / res);
    if (!(fabs(fx) <= ROAM_MAP_MAX_INDEX && fabs(fy) <= ROAM_MAP_MAX_INDEX)) return ROAM_E_ARG;      // the margin needs fx - 1 and (fx - 1) res nearly exact
    const double x0 = (fx - 1.0) * res, y0 = (fy - 1.0) * res;
    const double w = floor((maxx - x0) / res) + 2.0, h = floor((maxy - y0) / res) + 2.0;
    if (!(w <= ROAM_MAP_MAX_CELLS && h <= ROAM_MAP_MAX_CELLS && w * h <= ROAM_MAP_MAX_CELLS)) return ROAM_E_CAPACITY;
    *ox = x0; *oy = y0; *W = (int32_t)w; *H = (int32_t)h;
    return ROAM_OK;
}

// what both device entries refuse first: no db, no clouds, null or bad poses
static int32_t map_check_src(roam_ctx *ctx, const roam_loop_db *db, const double *poses)
{
    if (!db) { ROAM_SET_ERR(ctx, "loop db map: db is null"); return ROAM_E_ARG; }
    if (!db->cloud_rows) { ROAM_SET_ERR(ctx, "loop db map: db keeps no clouds (roam_loop_db_keep_clouds)"); return ROAM_E_STATE; }
    if (!poses && db->count) { ROAM_SET_ERR(ctx, "loop db map: poses is null"); return ROAM_E_ARG; }
    for (int64_t e = 0; e < db->count; ++e)
        if (!(fabs(poses[3 * e]) <= ROAM_ICP_MAX_COORD && fabs(poses[3 * e + 1]) <= ROAM_ICP_MAX_COORD && std::isfinite(poses[3 * e + 2]))) {
            ROAM_SET_ERR(ctx, "loop db map: poses of entry %lld: a pose that is not finite or beyond %g m", (long long)e, ROAM_ICP_MAX_COORD);
            return ROAM_E_ARG;
        }
    return ROAM_OK;
}

static int32_t map_check_grid(roam_ctx *ctx, double res, double ox, double oy, int32_t W, int32_t H, int32_t min_hits, int32_t min_views)
{
    if (!(std::isfinite(res) && res > 0.0)) { ROAM_SET_ERR(ctx, "loop db map: res finite and > 0, not %g", res); return ROAM_E_ARG; }
    if (!(std::isfinite(ox) && std::isfinite(oy))) { ROAM_SET_ERR(ctx, "loop db map: the origin ox, oy finite, not %g, %g", ox, oy); return ROAM_E_ARG; }
    if (W < 1 || H < 1) { ROAM_SET_ERR(ctx, "loop db map: W and H >= 1, not %d and %d", W, H); return ROAM_E_ARG; }
    if ((int64_t)W * H > ROAM_MAP_MAX_CELLS) {
        ROAM_SET_ERR(ctx, "loop db map: W H = %lld cells, beyond ROAM_MAP_MAX_CELLS = %d", (long long)((int64_t)W * H), ROAM_MAP_MAX_CELLS);
        return ROAM_E_ARG;
    }
    if (min_hits < 1 || min_views < 1) { ROAM_SET_ERR(ctx, "loop db map: min_hits and min_views >= 1, not %d and %d", min_hits, min_views); return ROAM_E_ARG; }
    return ROAM_OK;
}

// the points the used entries hold, from the host's copy of the counts
static int64_t map_used_points(const roam_loop_db *db, const int8_t *use)
{
    int64_t n = 0;
    for (int e = 0; e < db->count; ++e)
        if (!use || use[e]) n += db->h_n[e];
    return n;
}

// poses, their table and the mask to the device (S_IN0, S_IN1) -> src; cs: host room the caller keeps until the stream has been waited for
static int32_t map_stage(roam_ctx *ctx, const roam_loop_db *db, const double *poses, const int8_t *use, std::vector<double> *cs, MapSrc *src)
{
    const size_t n = (size_t)db->count;
    *src = MapSrc{db->cloud, db->cloud_n, db->max_points, nullptr, nullptr, nullptr};
    if (!n) return ROAM_OK;
    cs->resize(2 * n);
    map_pose_cs((int64_t)n, poses, cs->data());
    double *d_pose = (double *)roam_scratch(ctx, S_IN0, sizeof(double) * 5 * n);
    int8_t *d_use = use ? (int8_t *)roam_scratch(ctx, S_IN1, n) : nullptr;
    if (!d_pose || (use && !d_use)) return ROAM_E_HIP;
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_pose, poses, sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_pose + 3 * n, cs->data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, st));
    if (use) HIP_TRY(ctx, hipMemcpyAsync(d_use, use, n, hipMemcpyHostToDevice, st));
    src->poses = d_pose;
    src->cs = d_pose + 3 * n;
    src->use = d_use;
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_map_bounds(roam_ctx *ctx, roam_loop_db *db, const double *poses, const int8_t *use, double *bounds_out,
                                           int64_t *n_points_out)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(map_check_src(ctx, db, poses));
    if (!bounds_out || !n_points_out) { ROAM_SET_ERR(ctx, "loop db map: %s is null", !bounds_out ? "bounds_out" : "n_points_out"); return ROAM_E_ARG; }
    unsigned long long keys[4];
    for (int q = 0; q < 4; ++q) keys[q] = map_order_key(q & 1 ? -INFINITY : INFINITY);
    const int64_t n_points = map_used_points(db, use);
    if (n_points) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const hipStream_t st = ctx->stream;
        unsigned long long *d_keys = (unsigned long long *)roam_scratch(ctx, S_TMP1, sizeof(keys));
        if (!d_keys) return ROAM_E_HIP;
        std::vector<double> cs;
        MapSrc src;
        LOOP_TRY(map_stage(ctx, db, poses, use, &cs, &src));
        HIP_TRY(ctx, hipMemcpyAsync(d_keys, keys, sizeof(keys), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(map_bounds_kernel, dim3(db->count), dim3(MAP_RED_THREADS), 0, st, src, d_keys);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(keys, d_keys, sizeof(keys), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    for (int q = 0; q < 4; ++q) bounds_out[q] = map_order_value(keys[q]);
    *n_points_out = n_points;
    return ROAM_OK;
}

// the device side of one render: the grid (S_TMP0), the counters and the chunk lists (S_TMP1), the records (S_OUT0 .. S_OUT2)
struct MapBufs {
    MapGrid g;
    int64_t cells;
    int n_chunks;
    int32_t room;                // records the device lists hold
    unsigned long long *n_outside;
    int32_t *total, *chunk_count, *chunk_off;
    double *pts;
    uint32_t *pt_hits, *pt_views;
};

static int32_t map_take(roam_ctx *ctx, double res, double ox, double oy, int W, int H, int64_t room, MapBufs *b)
{
    b->cells = (int64_t)W * H;
    b->n_chunks = (int)((b->cells + MAP_CHUNK - 1) / MAP_CHUNK);
    b->room = (int32_t)(room < b->cells ? room : b->cells);
    char *grid = (char *)roam_scratch(ctx, S_TMP0, 24 * (size_t)b->cells);
    char *lists = (char *)roam_scratch(ctx, S_TMP1, 16 + sizeof(int32_t) * 2 * (size_t)b->n_chunks);
    const size_t room1 = b->room > 0 ? (size_t)b->room : 1;
    b->pts = (double *)roam_scratch(ctx, S_OUT0, sizeof(double) * 2 * room1);
    b->pt_hits = (uint32_t *)roam_scratch(ctx, S_OUT1, sizeof(uint32_t) * room1);
    b->pt_views = (uint32_t *)roam_scratch(ctx, S_OUT2, sizeof(uint32_t) * room1);
    if (!grid || !lists || !b->pts || !b->pt_hits || !b->pt_views) return ROAM_E_HIP;
    unsigned long long *sx = (unsigned long long *)grid;
    uint32_t *hits = (uint32_t *)(sx + 2 * b->cells);
    b->g = MapGrid{sx, sx + b->cells, hits, hits + b->cells, res, ox, oy, W, H};
    b->n_outside = (unsigned long long *)lists;
    b->total = (int32_t *)(lists + 8);
    b->chunk_count = (int32_t *)(lists + 16);
    b->chunk_off = b->chunk_count + b->n_chunks;
    return ROAM_OK;
}

static hipError_t map_launch_clear(hipStream_t st, const MapBufs &b)
{
    const hipError_t e = hipMemsetAsync(b.g.sx, 0, 24 * (size_t)b.cells, st);
    return e != hipSuccess ? e : hipMemsetAsync(b.n_outside, 0, 16, st);
}

static hipError_t map_launch_splat(hipStream_t st, const MapSrc &src, const MapBufs &b, int count)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(map_splat_kernel, dim3(count), dim3(MAP_THREADS), 0, st, src, b.g, b.n_outside);
    return hipGetLastError();
}

static hipError_t map_launch_compact(hipStream_t st, const MapBufs &b, uint32_t min_hits, uint32_t min_views)
{
    hipLaunchKernelGGL(map_count_kernel, dim3(b.n_chunks), dim3(MAP_RED_THREADS), 0, st, b.g.hits, b.g.views, b.cells, min_hits, min_views, b.chunk_count);
    hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(MAP_SCAN_THREADS), 0, st, b.chunk_count, b.n_chunks, b.chunk_off, b.total);
    hipLaunchKernelGGL(map_write_kernel, dim3(b.n_chunks), dim3(MAP_RED_THREADS), 0, st, b.g, b.cells, min_hits, min_views, b.chunk_off, b.total, b.room,
                       b.pts, b.pt_hits, b.pt_views);
    return hipGetLastError();
}

extern "C" int32_t roam_loop_db_map_render(roam_ctx *ctx, roam_loop_db *db, const double *poses, const int8_t *use, double res, double ox, double oy,
                                           int32_t W, int32_t H, int32_t min_hits, int32_t min_views, uint32_t *hits_out, uint32_t *views_out,
                                           double *points_out, uint32_t *point_hits_out, uint32_t *point_views_out, int32_t cap,
                                           int32_t *n_points_out, int64_t *n_outside_out)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(map_check_src(ctx, db, poses));
    LOOP_TRY(map_check_grid(ctx, res, ox, oy, W, H, min_hits, min_views));
    if (cap < 0) { ROAM_SET_ERR(ctx, "loop db map: cap >= 0, not %d", cap); return ROAM_E_ARG; }
    if (!n_points_out || !n_outside_out || (cap > 0 && (!points_out || !point_hits_out || !point_views_out))) {
        ROAM_SET_ERR(ctx, "loop db map: %s is null", !n_points_out ? "n_points_out" : !n_outside_out ? "n_outside_out" : !points_out ? "points_out"
                                                     : !point_hits_out ? "point_hits_out" : "point_views_out");
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    // a cell that qualifies holds a point, so the used entries' points bound the list: the device lists need no more room than that
    const int64_t used = map_used_points(db, use);
    MapBufs b;
    LOOP_TRY(map_take(ctx, res, ox, oy, W, H, used < cap ? used : cap, &b));
    std::vector<double> cs;
    MapSrc src;
    LOOP_TRY(map_stage(ctx, db, poses, use, &cs, &src));
    HIP_TRY(ctx, map_launch_clear(st, b));
    HIP_TRY(ctx, map_launch_splat(st, src, b, db->count));
    HIP_TRY(ctx, map_launch_compact(st, b, (uint32_t)min_hits, (uint32_t)min_views));
    // the read-back: the counters and the grids, then the records the counters announce
    int32_t total = 0;
    unsigned long long outside = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, b.total, sizeof(total), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&outside, b.n_outside, sizeof(outside), hipMemcpyDeviceToHost, st));
    if (hits_out) HIP_TRY(ctx, hipMemcpyAsync(hits_out, b.g.hits, sizeof(uint32_t) * (size_t)b.cells, hipMemcpyDeviceToHost, st));
    if (views_out) HIP_TRY(ctx, hipMemcpyAsync(views_out, b.g.views, sizeof(uint32_t) * (size_t)b.cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *n_points_out = total;
    *n_outside_out = (int64_t)outside;
    if (total > cap) { ROAM_SET_ERR(ctx, "loop db map: %d map points, capacity %d", total, cap); return ROAM_E_CAPACITY; }
    if (total > b.room) { ROAM_SET_ERR(ctx, "loop db map: %d map points from %lld stored points", total, (long long)used); return ROAM_E_STATE; }
    if (total > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(points_out, b.pts, sizeof(double) * 2 * (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(point_hits_out, b.pt_hits, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(point_views_out, b.pt_views, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return ROAM_OK;
}

extern "C" int32_t roam_time_loop_db_map(roam_ctx *ctx, roam_loop_db *db, const double *poses, const int8_t *use, double res, double ox, double oy,
                                         int32_t W, int32_t H, int32_t min_hits, int32_t min_views, int32_t reps, float *ms)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(map_check_src(ctx, db, poses));
    LOOP_TRY(map_check_grid(ctx, res, ox, oy, W, H, min_hits, min_views));
    ARG_CHECK(ctx, reps >= 1 && ms);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    MapBufs b;
    LOOP_TRY(map_take(ctx, res, ox, oy, W, H, map_used_points(db, use), &b));
    std::vector<double> cs;
    MapSrc src;
    LOOP_TRY(map_stage(ctx, db, poses, use, &cs, &src));
    // the splat's launches add up in the grid (integers far from their ends); the compaction is then timed on a grid cleared and splatted once
    LOOP_TRY(roam_time_launches(ctx, st, reps, ms, [&] { return map_launch_clear(st, b); }));
    LOOP_TRY(roam_time_launches(ctx, st, reps, ms + 1, [&] { return map_launch_splat(st, src, b, db->count); }));
    HIP_TRY(ctx, map_launch_clear(st, b));
    HIP_TRY(ctx, map_launch_splat(st, src, b, db->count));
    return roam_time_launches(ctx, st, reps, ms + 2, [&] { return map_launch_compact(st, b, (uint32_t)min_hits, (uint32_t)min_views); });
}
