// Origin-shifted scan contexts (the augmentation of Scan Context++, Kim, Choi, Kim, T-RO 2021): an entry is described again as seen
// from a few virtual origins a lane width or so away, the variants are kept beside it and serve as its queries.  Map of the
// family: loop.h.  Parity is unpinned; the contract is tests/scan_context_offset_model.py.
//
// The rule.  Every polar sample (a, c), a < rows, c < clip, sits at its centre: rho = c + 0.5, (C_a, S_a) = (cos, sin) of
// phi_a = (2.0 * M_PI * (a + 0.5)) / rows from the host's libm.  For the offset (ox, oy) in range bins: x = rho C_a - ox,
// y = rho S_a - oy, q = x x + y y, every operation rounded once in float64 (__dmul_rn / __dadd_rn / __dsub_rn: no contraction).  Ring:
// the r with E_r^2 <= q < E_{r+1}^2 for the integer column edges E_r (exact squares); q >= clip^2 is dropped.  Sector: with the boundary
// directions b_s = (cos, sin)((2.0 * M_PI * row_edges[s]) / rows) of the host's libm and k_s = b_s.x y - b_s.y x, the lowest s with
// k_s >= 0 and k_{(s + 1) mod S} < 0; none: dropped.  A bin holds the mean over the samples that landed in it, 0 when none did.
// The device guesses (a float square root and a table for the ring, a float arctangent for the sector) and then walks with the exact
// float64 tests, so the guess decides nothing.  The computed signs of k_s are >= 0 on one arc of boundaries and < 0 on the other, so
// at most one s passes the test: the s the walk stops at is the rule's lowest.
//
// scan_context_offset_kernel.  One wave per workgroup: (image, offset, block of `rb` rows, tile of at most 4096 bins), lanes along
// range (coalesced reads of a row).  LDS: e2[R + 1] float64 (squared edges), bx[S], by[S] float64, the tile's histogram, ring_of[clip]
// uint8 (the ring of a column, the guess).  u8 codes: the histogram is one 64-bit word per bin, count in the high half and sum in the
// low half (a block's sum stays below 2^32: at most 1024 rows x 4096 columns x 255), updated with one integer LDS atomic per sample
// and flushed with integer global atomics into one slab per (image, offset) - exact, so no order matters.  float32 images: no
// atomics.  The lanes of a wave that hold one bin are summed with an xor butterfly (the others add zero), the leader adds the
// result to the bin; the wave visits the rows of its block and the columns of a row in order, so a block's partial sum is one fixed
// order of additions, the blocks of rows depend on (rows) alone, and the finishing kernel adds the blocks' slabs in block order: the
// same bits whatever the batch and the chunk.  A tile that does not hold a sample's bin skips it; S R <= 4096 bins is one tile.
// scan_context_offset_finish_kernel.  One workgroup per (image, offset, sector): lane r divides the bin's sum by its count, then the
// column's norm by sc_sector_norm and the stored nrm / valid exactly as every other entry gets them.
#include "loop.h"
#include <math.h>
#include <cmath>
#include <type_traits>
#include <vector>

#define SO_TILE_BINS 4096
#define SO_MAX_BLOCKS 128                        // blocks of rows per image: rb = max(4, ceil(rows / 128))
#define SO_FINISH_THREADS 128                    // >= ROAM_SCAN_CONTEXT_MAX_RINGS

static int so_block_rows(int rows) { const int rb = (rows + SO_MAX_BLOCKS - 1) / SO_MAX_BLOCKS; return rb < 4 ? 4 : rb; }
static int so_blocks(int rows) { const int rb = so_block_rows(rows); return (rows + rb - 1) / rb; }

// ---------------------------------------------------------------------------------------------------------------- device
// psum / pcnt: U8: one slab of S R bins per (image, offset), cleared before the launch; float32: nblk slabs, every bin written
template <bool U8>
__global__ __launch_bounds__(64) void scan_context_offset_kernel(ScSrc src, int rows, int clip, int S, int R, int rb, int nblk, double floor_v,
                                                                 int floor_code, const double *__restrict__ trig,
                                                                 const double *__restrict__ off_bins, unsigned long long *__restrict__ psum,
                                                                 uint32_t *__restrict__ pcnt)
{
    extern __shared__ __align__(16) unsigned char so_lds[];
    const int SR = S * R;
    const int lane = threadIdx.x;
    const int64_t z = blockIdx.x;
    const int o = blockIdx.y, n_off = gridDim.y;
    const int tile = blockIdx.z / nblk, blk = blockIdx.z - tile * nblk;
    const int k0 = tile * SO_TILE_BINS, nk = SR - k0 < SO_TILE_BINS ? SR - k0 : SO_TILE_BINS;
    double *e2 = (double *)so_lds;                        // R + 1
    double *bx = e2 + R + 1, *by = bx + S;                // S each
    unsigned long long *h64 = (unsigned long long *)(by + S);      // nk: the packed histogram (u8) or the float64 sums
    uint32_t *hcnt = (uint32_t *)(h64 + nk);              // nk (float32 only)
    uint8_t *ring_of = (uint8_t *)(hcnt + (U8 ? 0 : nk)); // clip
    for (int r = lane; r <= R; r += 64) {
        const int64_t e = (int64_t)r * clip / R;
        e2[r] = (double)(e * e);
    }
    for (int s = lane; s < S; s += 64) {
        bx[s] = trig[2 * rows + s];
        by[s] = trig[2 * rows + S + s];
    }
    for (int i = lane; i < nk; i += 64) {
        h64[i] = 0;
        if (!U8) hcnt[i] = 0;
    }
    for (int c = lane; c < clip; c += 64) ring_of[c] = (uint8_t)((((int64_t)c + 1) * R - 1) / clip);
    __syncthreads();
    const double ox = off_bins[2 * o], oy = off_bins[2 * o + 1];
    const double clip2 = e2[R];
    const int64_t img = src.index ? src.index[z] : z;
    const int a0 = blk * rb, a1 = a0 + rb < rows ? a0 + rb : rows;
    for (int a = a0; a < a1; ++a) {
        const double Ca = trig[a], Sa = trig[rows + a];
        for (int c0 = 0; c0 < clip; c0 += 64) {
            const int c = c0 + lane;
            int key = -1;
            uint32_t code = 0;
            double term = 0.0;
            if (c < clip) {
                // the sample's value first, so that its latency hides behind the geometry (a dropped sample's value is not used)
                if constexpr (U8) {
                    const uint8_t *p = (const uint8_t *)src.base + img * src.image_stride + src.payload_off + c;
                    code = (uint32_t)max((int)p[a * src.row_stride] - floor_code, 0);
                } else {
                    const float *p = (const float *)src.base + img * src.image_stride + c;
                    term = fmax((double)p[a * src.row_stride] - floor_v, 0.0);
                }
                const double rho = (double)c + 0.5;
                const double x = __dsub_rn(__dmul_rn(rho, Ca), ox), y = __dsub_rn(__dmul_rn(rho, Sa), oy);
                const double q = __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y));
                if (q < clip2) {
                    int col = (int)sqrtf((float)q);
                    col = col < clip ? col : clip - 1;
                    int r = ring_of[col];
                    while (r > 0 && q < e2[r]) --r;
                    while (r < R - 1 && q >= e2[r + 1]) ++r;
                    float t = atan2f((float)y, (float)x) * 0.15915494f;
                    t -= floorf(t);
                    int s = (int)(t * (float)S);
                    s = s < 0 ? 0 : s >= S ? S - 1 : s;
                    bool found = false;
                    for (int it = 0; it < S && !found; ++it) {
                        const int n = s + 1 == S ? 0 : s + 1;
                        const double ks = __dsub_rn(__dmul_rn(bx[s], y), __dmul_rn(by[s], x));
                        const double kn = __dsub_rn(__dmul_rn(bx[n], y), __dmul_rn(by[n], x));
                        if (ks >= 0.0 && kn < 0.0) found = true;
                        else s = ks < 0.0 ? (s == 0 ? S - 1 : s - 1) : n;
                    }
                    if (found) {
                        const int k = s * R + r - k0;
                        if (k >= 0 && k < nk) key = k;
                    }
                }
            }
            if constexpr (U8) {
                if (key >= 0) atomicAdd(&h64[key], (1ull << 32) | (unsigned long long)code);
            } else {
                double *hsum = (double *)h64;
                unsigned long long active = __ballot(key >= 0);
                while (active) {                                  // one pass per bin the wave holds, lowest lane first
                    const int leader = __ffsll((long long)active) - 1;
                    const int lk = __shfl(key, leader);
                    const bool mine = key == lk;
                    double v = mine ? term : 0.0;
                    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
                    const unsigned long long m = __ballot(mine);
                    if (lane == leader) {
                        hsum[lk] += v;
                        hcnt[lk] += (uint32_t)__popcll(m);
                    }
                    active &= ~m;
                }
            }
        }
    }
    __syncthreads();
    if constexpr (U8) {
        const int64_t base = (z * n_off + o) * SR + k0;
        for (int i = lane; i < nk; i += 64) {
            const unsigned long long v = h64[i];
            if (v >> 32) {
                atomicAdd(&psum[base + i], v & 0xffffffffull);
                atomicAdd(&pcnt[base + i], (uint32_t)(v >> 32));
            }
        }
    } else {
        const int64_t base = ((z * n_off + o) * nblk + blk) * SR + k0;
        for (int i = lane; i < nk; i += 64) {
            psum[base + i] = h64[i];
            pcnt[base + i] = hcnt[i];
        }
    }
}

// slabs -> the variant (z, o): desc, and nrm / valid when asked for
template <bool U8>
__global__ __launch_bounds__(SO_FINISH_THREADS) void scan_context_offset_finish_kernel(const unsigned long long *__restrict__ psum,
                                                                                        const uint32_t *__restrict__ pcnt, int nslab, int S, int R,
                                                                                        int Rp, float *__restrict__ vdesc, double *__restrict__ vnrm,
                                                                                        int32_t *__restrict__ vvalid)
{
    __shared__ float dv[SO_FINISH_THREADS];
    __shared__ double nv;
    const int s = blockIdx.z, r = threadIdx.x;
    const int64_t zo = (int64_t)blockIdx.x * gridDim.y + blockIdx.y;
    if (r < R) {
        unsigned long long isum = 0, cnt = 0;
        double fsum = 0.0;
        for (int b = 0; b < nslab; ++b) {
            const int64_t i = ((zo * nslab + b) * S + s) * R + r;
            if constexpr (U8) isum += psum[i];
            else fsum += __longlong_as_double((long long)psum[i]);
            cnt += pcnt[i];
        }
        float d = 0.0f;
        if (cnt) d = U8 ? (float)((double)isum / (255.0 * (double)cnt)) : (float)(fsum / (double)cnt);
        dv[r] = d;
    }
    __syncthreads();
    if (r == 0) nv = sc_sector_norm(dv, R);
    __syncthreads();
    const double norm = nv;
    const int64_t row = zo * S + s;
    if (r < R) vdesc[row * R + r] = dv[r];
    if (vnrm && r < Rp) vnrm[row * Rp + r] = r < R ? sc_normalised(dv[r], norm) : 0.0;
    if (vvalid && r == 0) vvalid[row] = norm > 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- host
void sc_offset_table(int rows, int S, double *out)
{
    for (int a = 0; a < rows; ++a) {
        const double phi = (2.0 * M_PI * ((double)a + 0.5)) / (double)rows;
        out[a] = cos(phi);
        out[rows + a] = sin(phi);
    }
    for (int s = 0; s < S; ++s) {
        const double beta = (2.0 * M_PI * (double)((int64_t)s * rows / S)) / (double)rows;
        out[2 * rows + s] = cos(beta);
        out[2 * rows + S + s] = sin(beta);
    }
}

extern "C" int32_t roam_scan_context_offset_table(int32_t rows, int32_t sectors, double *cos_row, double *sin_row, double *cos_edge,
                                                  double *sin_edge)
{
    if (sectors < 2 || sectors > ROAM_SCAN_CONTEXT_MAX_SECTORS || rows < sectors || rows > SC_MAX_ROWS) return ROAM_E_ARG;
    if (!cos_row || !sin_row || !cos_edge || !sin_edge) return ROAM_E_ARG;
    std::vector<double> t(2 * (size_t)rows + 2 * (size_t)sectors);
    sc_offset_table(rows, sectors, t.data());
    for (int a = 0; a < rows; ++a) { cos_row[a] = t[a]; sin_row[a] = t[rows + a]; }
    for (int s = 0; s < sectors; ++s) { cos_edge[s] = t[2 * rows + s]; sin_edge[s] = t[2 * rows + sectors + s]; }
    return ROAM_OK;
}

int64_t sc_offset_part_bytes(bool u8, int rows, int S, int R, int n_off)
{
    return (int64_t)(u8 ? 1 : so_blocks(rows)) * n_off * S * R * (int64_t)(sizeof(unsigned long long) + sizeof(uint32_t));
}

int32_t sc_launch_offsets(roam_ctx *ctx, bool u8, const ScSrc &src, int n, int rows, int clip, int S, int R, double floor_v, int floor_code,
                          const ScOffsets &offs, int64_t first)
{
    const hipStream_t st = ctx->stream;
    const int SR = S * R, Rp = (R + 3) & ~3, n_off = offs.n_off;
    const int rb = so_block_rows(rows), nblk = so_blocks(rows), tiles = (SR + SO_TILE_BINS - 1) / SO_TILE_BINS;
    const int nslab = u8 ? 1 : nblk;
    const size_t bins = (size_t)n * n_off * nslab * SR;
    unsigned long long *psum = (unsigned long long *)roam_scratch(ctx, S_TMP5, sizeof(unsigned long long) * bins);
    uint32_t *pcnt = (uint32_t *)roam_scratch(ctx, S_TMP6, sizeof(uint32_t) * bins);
    if (!psum || !pcnt) return ROAM_E_HIP;
    const int nk = SR < SO_TILE_BINS ? SR : SO_TILE_BINS;
    const size_t lds = sizeof(double) * (size_t)(R + 1 + 2 * S) + (size_t)nk * (u8 ? 8 : 12) + (size_t)clip;
    const dim3 grid(n, n_off, nblk * tiles);
    float *vd = offs.vdesc + first * n_off * SR;
    double *vn = offs.vnrm ? offs.vnrm + first * n_off * S * Rp : nullptr;
    int32_t *vv = offs.vvalid ? offs.vvalid + first * n_off * S : nullptr;
    const dim3 fgrid(n, n_off, S);
    if (u8) {
        HIP_TRY(ctx, hipMemsetAsync(psum, 0, sizeof(unsigned long long) * bins, st));
        HIP_TRY(ctx, hipMemsetAsync(pcnt, 0, sizeof(uint32_t) * bins, st));
        hipLaunchKernelGGL(scan_context_offset_kernel<true>, grid, dim3(64), lds, st, src, rows, clip, S, R, rb, nblk, floor_v, floor_code, offs.trig,
                           offs.off_bins, psum, pcnt);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(scan_context_offset_finish_kernel<true>, fgrid, dim3(SO_FINISH_THREADS), 0, st, psum, pcnt, nslab, S, R, Rp, vd, vn, vv);
    } else {
        hipLaunchKernelGGL(scan_context_offset_kernel<false>, grid, dim3(64), lds, st, src, rows, clip, S, R, rb, nblk, floor_v, floor_code,
                           offs.trig, offs.off_bins, psum, pcnt);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(scan_context_offset_finish_kernel<false>, fgrid, dim3(SO_FINISH_THREADS), 0, st, psum, pcnt, nslab, S, R, Rp, vd, vn, vv);
    }
    HIP_TRY(ctx, hipGetLastError());
    return ROAM_OK;
}

// ---- the variant store of a database
void sc_offsets_free(roam_loop_db *db)
{
    for (void **q : {(void **)&db->vdesc, (void **)&db->vnrm, (void **)&db->vvalid, (void **)&db->off_bins, (void **)&db->off_m, (void **)&db->off_trig}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    db->n_off = db->off_rows = 0;
}

// what the offsets of roam_loop_db_keep_offsets / roam_scan_context_offsets_f32 must be
static int32_t so_check_offsets(roam_ctx *ctx, int32_t n_offsets, const double *offsets_m, double range_resolution_m)
{
    if (n_offsets < 1 || n_offsets > ROAM_LOOP_MAX_OFFSETS) {
        ROAM_SET_ERR(ctx, "scan context offsets: n_offsets in [1, %d], not %d", ROAM_LOOP_MAX_OFFSETS, n_offsets);
        return ROAM_E_ARG;
    }
    if (!offsets_m) { ROAM_SET_ERR(ctx, "scan context offsets: offsets_m is null"); return ROAM_E_ARG; }
    if (!(std::isfinite(range_resolution_m) && range_resolution_m > 0.0)) {
        ROAM_SET_ERR(ctx, "scan context offsets: range_resolution_m finite and > 0, not %g", range_resolution_m);
        return ROAM_E_ARG;
    }
    for (int i = 0; i < n_offsets; ++i) {
        const double x = offsets_m[2 * i], y = offsets_m[2 * i + 1];
        if (!(std::isfinite(x) && std::isfinite(y) && fabs(x) <= ROAM_ICP_MAX_COORD && fabs(y) <= ROAM_ICP_MAX_COORD)) {
            ROAM_SET_ERR(ctx, "scan context offsets: offsets_m[%d] is not finite or beyond %g m", i, ROAM_ICP_MAX_COORD);
            return ROAM_E_ARG;
        }
        if (x == 0.0 && y == 0.0) {
            ROAM_SET_ERR(ctx, "scan context offsets: offsets_m[%d] is (0, 0) - variant 0 is the plain descriptor already", i);
            return ROAM_E_ARG;
        }
    }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_keep_offsets(roam_ctx *ctx, roam_loop_db *db, int32_t n_offsets, const double *offsets_m, double range_resolution_m)
{
    if (!ctx) return ROAM_E_ARG;
    if (!db) { ROAM_SET_ERR(ctx, "loop db: db is null"); return ROAM_E_ARG; }
    LOOP_TRY(so_check_offsets(ctx, n_offsets, offsets_m, range_resolution_m));
    if (db->count != 0 || db->n_off) {
        ROAM_SET_ERR(ctx, "loop db: keep_offsets once, on an empty database (%d entries%s)", db->count, db->n_off ? ", keeps offsets already" : "");
        return ROAM_E_ARG;
    }
    const int64_t per = (int64_t)n_offsets * db->S * (sizeof(float) * db->R + sizeof(double) * db->Rp + sizeof(int32_t));
    if (per * db->capacity > SC_DB_BYTES) {
        ROAM_SET_ERR(ctx, "loop db: capacity %d x %d offsets x %lld bytes is beyond the %lld bytes of a variant store", db->capacity, n_offsets,
                     (long long)(per / n_offsets), (long long)SC_DB_BYTES);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t rows = (size_t)db->capacity * n_offsets * db->S;
    const size_t table = 2 * (size_t)SC_MAX_ROWS + 2 * (size_t)db->S;
    if (hipMalloc(&db->vdesc, sizeof(float) * rows * db->R) != hipSuccess || hipMalloc(&db->vnrm, sizeof(double) * rows * db->Rp) != hipSuccess ||
        hipMalloc(&db->vvalid, sizeof(int32_t) * rows) != hipSuccess || hipMalloc(&db->off_bins, sizeof(double) * 2 * n_offsets) != hipSuccess ||
        hipMalloc(&db->off_m, sizeof(double) * 2 * n_offsets) != hipSuccess || hipMalloc(&db->off_trig, sizeof(double) * table) != hipSuccess) {
        ROAM_SET_ERR(ctx, "loop db: hipMalloc of %lld bytes of variants failed", (long long)(per * db->capacity));
        sc_offsets_free(db);
        return ROAM_E_HIP;
    }
    std::vector<double> bins(2 * (size_t)n_offsets);
    for (int i = 0; i < 2 * n_offsets; ++i) bins[i] = offsets_m[i] / range_resolution_m;
    const hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(db->off_bins, bins.data(), sizeof(double) * bins.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(db->off_m, offsets_m, sizeof(double) * bins.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    db->n_off = n_offsets;
    return ROAM_OK;
}

int32_t sc_offsets_of_db(roam_ctx *ctx, roam_loop_db *db, int rows, ScOffsets *out)
{
    if (db->off_rows != rows) {
        std::vector<double> t(2 * (size_t)rows + 2 * (size_t)db->S);
        sc_offset_table(rows, db->S, t.data());
        HIP_TRY(ctx, hipMemcpyAsync(db->off_trig, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // the table is a local
        db->off_rows = rows;
    }
    *out = ScOffsets{db->n_off, db->off_trig, db->off_bins, db->vdesc, db->vnrm, db->vvalid};
    return ROAM_OK;
}

int32_t sc_offsets_clear(roam_ctx *ctx, const roam_loop_db *db, int64_t first, int n)
{
    const size_t rows = (size_t)n * db->n_off * db->S, at = (size_t)first * db->n_off * db->S;
    HIP_TRY(ctx, hipMemsetAsync(db->vdesc + at * db->R, 0, sizeof(float) * rows * db->R, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(db->vnrm + at * db->Rp, 0, sizeof(double) * rows * db->Rp, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(db->vvalid + at, 0, sizeof(int32_t) * rows, ctx->stream));
    return ROAM_OK;
}

static int32_t so_check_entry(roam_ctx *ctx, const roam_loop_db *db, int32_t index, const void *p)
{
    if (!db || !p) { ROAM_SET_ERR(ctx, "loop db variants: %s is null", db ? "desc" : "db"); return ROAM_E_ARG; }
    if (!db->n_off) { ROAM_SET_ERR(ctx, "loop db variants: db keeps no offsets (roam_loop_db_keep_offsets)"); return ROAM_E_STATE; }
    if (index < 0 || index >= db->count) { ROAM_SET_ERR(ctx, "loop db variants: index %d outside the %d entries stored", index, db->count); return ROAM_E_ARG; }
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_set_variants(roam_ctx *ctx, roam_loop_db *db, int32_t index, const float *desc)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(so_check_entry(ctx, db, index, desc));
    const int64_t per = (int64_t)db->n_off * db->S * db->R;
    for (int64_t q = 0; q < per; ++q)
        if (!std::isfinite(desc[q])) { ROAM_SET_ERR(ctx, "loop db variants: desc element %lld is not finite", (long long)q); return ROAM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const int64_t n_rows = (int64_t)db->n_off * db->S, at = (int64_t)index * n_rows;
    HIP_TRY(ctx, hipMemcpyAsync(db->vdesc + at * db->R, desc, sizeof(float) * per, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, sc_launch_norm_rows(st, db->vdesc + at * db->R, n_rows, db->R, db->Rp, db->vnrm + at * db->Rp, db->vvalid + at));      // as add_desc
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return ROAM_OK;
}

extern "C" int32_t roam_loop_db_get_variants(roam_ctx *ctx, roam_loop_db *db, int32_t index, float *desc_out, int32_t *valid_out)
{
    if (!ctx) return ROAM_E_ARG;
    LOOP_TRY(so_check_entry(ctx, db, index, desc_out));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n_rows = (int64_t)db->n_off * db->S, at = (int64_t)index * n_rows;
    HIP_TRY(ctx, hipMemcpyAsync(desc_out, db->vdesc + at * db->R, sizeof(float) * n_rows * db->R, hipMemcpyDeviceToHost, ctx->stream));
    if (valid_out) HIP_TRY(ctx, hipMemcpyAsync(valid_out, db->vvalid + at, sizeof(int32_t) * n_rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ROAM_OK;
}

extern "C" int32_t roam_scan_context_offsets_f32(roam_ctx *ctx, const float *polar, int32_t n, int32_t rows, int32_t cols, int64_t row_stride,
                                                 int64_t image_stride, int32_t clip_px, int32_t sectors, int32_t rings, double floor,
                                                 int32_t n_offsets, const double *offsets_m, double range_resolution_m, float *desc_out)
{
    if (!ctx) return ROAM_E_ARG;
    int clip;
    LOOP_TRY(sc_check_f32_args(ctx, polar, n, rows, cols, row_stride, image_stride, clip_px, sectors, rings, floor, &clip));
    LOOP_TRY(so_check_offsets(ctx, n_offsets, offsets_m, range_resolution_m));
    if (!desc_out) { ROAM_SET_ERR(ctx, "scan context: desc_out is null"); return ROAM_E_ARG; }
    const int64_t SR = (int64_t)sectors * rings;
    if ((int64_t)n * n_offsets * SR * (int64_t)sizeof(float) > SC_DB_BYTES) {
        ROAM_SET_ERR(ctx, "scan context offsets: %d images x %d offsets do not fit %lld bytes", n, n_offsets, (long long)SC_DB_BYTES);
        return ROAM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    std::vector<double> t(2 * (size_t)rows + 2 * (size_t)sectors + 2 * (size_t)n_offsets);
    sc_offset_table(rows, sectors, t.data());
    double *bins = t.data() + 2 * (size_t)rows + 2 * (size_t)sectors;
    for (int i = 0; i < 2 * n_offsets; ++i) bins[i] = offsets_m[i] / range_resolution_m;
    double *d_t = (double *)roam_scratch(ctx, S_TMP7, sizeof(double) * t.size());
    float *d_desc = (float *)roam_scratch(ctx, S_OUT0, sizeof(float) * (size_t)n * SR);
    float *d_var = (float *)roam_scratch(ctx, S_TMP2, sizeof(float) * (size_t)n * n_offsets * SR);
    if (!d_t || !d_desc || !d_var) return ROAM_E_HIP;
    HIP_TRY(ctx, hipMemcpyAsync(d_t, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, st));
    const ScOffsets offs = {n_offsets, d_t, d_t + 2 * (size_t)rows + 2 * (size_t)sectors, d_var, nullptr, nullptr};
    LOOP_TRY(sc_describe_host_f32(ctx, polar, n, rows, row_stride, image_stride, clip, sectors, rings, floor, d_desc, nullptr, nullptr, 0, nullptr, 0, &offs));
    // desc_out (n, 1 + n_offsets, S, R): variant 0 from the plain kernel, the others behind it
    const size_t A = (size_t)n_offsets + 1;
    HIP_TRY(ctx, hipMemcpy2DAsync(desc_out, sizeof(float) * A * SR, d_desc, sizeof(float) * SR, sizeof(float) * SR, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpy2DAsync(desc_out + SR, sizeof(float) * A * SR, d_var, sizeof(float) * n_offsets * SR, sizeof(float) * n_offsets * SR, n,
                                  hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return ROAM_OK;
}
