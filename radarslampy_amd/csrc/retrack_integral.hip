// retrack_integral.hip - K1 / K2 of the device-side feature (re)detection (overview: retrack.hip): the float64 integral image
#include "retrack_geom.h"

// ------------------------------------------------------------------------------------------------ K1 / K2: integral image
// Two ways to the integral image, chosen on the device by the number of detections of the chunk (only the device knows it):
//   * rt_integral_kernel (below): one workgroup per detection, the image written once, but a chain of ~950 dependent phases
//     (64 rows x 64 columns each) per detection: milliseconds per chunk whatever its size
//   * rt_integ_cols_kernel (+ the band fix-up by its last workgroups) + rt_integ_rows_kernel: thousands of threads per detection, three times the
//     traffic, 0.26 ms for one alone
// Both are launched; the one whose regime it is not returns at once.
// Column pass, parallel over bands of RC_BAND rows.  A pixel is a float32 of at least 2^-18 (code / 255 times a weight product that is a
// multiple of 2^-10) or zero, i.e. a multiple of 2^-41, and a column of at most 4094 of them sums to less than 2^12: every partial
// sum is EXACT in float64, in any order.  So the 64 rows of a band's column are four threads of 16 rows each (round 6; one thread per
// band column until then: 16 dependent pairs of round trips - map word, then taps - were 48 of a lone detection's 54 us in this pass):
// all 16 map words leave at once, then all 64 taps, the quarters' totals meet in LDS; the workgroup writes the band-local sums and the
// band's total; the last workgroup of a column group turns the totals into what lies above each band, and the row pass adds that in as
// it loads (all exact = NumPy's values).
#define RT_TWO_PASS_Z 8                      // detections of a chunk the two-pass kernels work on at a time (grid z / y)
#define RC_BAND 64
#define RC_Q 16                              // rows per thread: RC_BAND / 4
__global__ __launch_bounds__(256) void rt_integ_cols_kernel(RtArgs a, int first, int P)
{
    // (the detections of the chunk are walked gridDim.z at a time: a grid of one slab per possible detection was 204 800 workgroups per
    // chunk that only returned whenever the chunk belonged to the one-sweep kernel or was empty - 1 to 9 ms of dispatch beside other kernels)
    const int nls = rt_one_sweep(a, first) ? 0 : min(min(RT_TWO_PASS_SLOTS, P), *a.rt_n - first);      // (P: the chunk's scratch slots)
    if ((int)blockIdx.z >= nls) return;
    __shared__ double tot[4][64];
    __shared__ float lut[256];
    __shared__ int last_s;
    lut[threadIdx.x] = rt_code_to_f32(threadIdx.x);
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, W = a.W, band = blockIdx.y, nb = (W + RC_BAND - 1) / RC_BAND;
    for (int ls = blockIdx.z; ls < nls; ls += (int)gridDim.z) {
    const int slot = first + ls;
    const uint8_t *p = a.pool + (int64_t)a.rt_scan[slot] * a.rec_bytes + a.payload_off;
    double *S = a.S + (int64_t)ls * a.SP * W;
    const int rows = a.rows, cols = a.cols, stride = a.stride;
    const int r0 = band * RC_BAND + q * RC_Q;
    uint32_t m[RC_Q];
#pragma unroll
    for (int k = 0; k < RC_Q; k++) m[k] = (c < W && r0 + k < W) ? a.map[(int64_t)(r0 + k) * W + c] : 0xfffu;     // (bin 4095: beyond any scan, a zero pixel)
    __syncthreads();                                   // (the table; the map words are on their way)
    float v[RC_Q];
#pragma unroll
    for (int k = 0; k < RC_Q; k++) v[k] = rt_pixel(m[k], p, rows, cols, stride, lut);      // (= warp_pixel: two 16-bit loads, table decode)
    double s[RC_Q], acc = 0;
#pragma unroll
    for (int k = 0; k < RC_Q; k++) { acc = __dadd_rn(acc, (double)v[k]); s[k] = acc; }
    tot[q][lane] = acc;
    __syncthreads();
    double base = 0;
    for (int j = 0; j < q; j++) base = __dadd_rn(base, tot[j][lane]);
    if (c < W) {
#pragma unroll
        for (int k = 0; k < RC_Q; k++)
            if (r0 + k < W) S[(int64_t)(r0 + k) * a.SP + c] = __dadd_rn(base, s[k]);
        if (q == 3) __hip_atomic_store(a.colT + ((int64_t)ls * nb + band) * W + c, __dadd_rn(base, acc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // band totals -> sum of the bands above (exclusive prefix per column; exact, see above), by the workgroup of this column group that
    // finishes LAST (a kernel of its own until round 6: one launch more in the chain every step enqueues); the totals are loaded 32 at a
    // time (one round trip instead of one per band).  col_done[detection][column group] counts the finished bands and is left at zero.
    // The totals cross between workgroups - between XCDs, each with an L2 of its own - as device-scope atomic stores and loads, the
    // counter after them: a __threadfence() here writes the XCD's whole L2 back, 32 MB of integral image included (151 us instead of 18).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx942__) && !defined(__gfx950__)
#error "rt_integ_cols_kernel's band totals reach the last workgroup relying on gfx94x/95x storing with write-through and counting stores in vmcnt: s_waitcnt vmcnt(0) + relaxed atomics, no release/acquire pair"
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) last_s = atomicAdd(a.col_done + ls * 64 + (int)blockIdx.x, 1) == nb - 1;
    __syncthreads();
    if (last_s) {
    if (q == 0 && c < W) {
        double *T = a.colT + (int64_t)ls * nb * W + c;
        double run = 0.0;
        for (int b0 = 0; b0 < nb; b0 += 32) {
            double tv[32];
#pragma unroll
            for (int j = 0; j < 32; j++) tv[j] = b0 + j < nb ? __hip_atomic_load(T + (int64_t)(b0 + j) * W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
            for (int j = 0; j < 32; j++)
                if (b0 + j < nb) { T[(int64_t)(b0 + j) * W] = run; run = __dadd_rn(run, tv[j]); }
        }
    }
    if (threadIdx.x == 0) a.col_done[ls * 64 + (int)blockIdx.x] = 0;
    }
    __syncthreads();                                   // (tot / last_s are the next detection's)
    }
}

// Row pass: a workgroup per 16 rows; 16 lanes of wave 0, lane = row, walk sequentially along the row (the reference's summation order);
// the image streams through LDS in 16 x 256 tiles so that global accesses stay coalesced (all four waves load and store, 2 KB per row).
// Round 6, for the lone detection of a single sequence (197 us until then, for a chain of 2 024 additions):
//   * the tiles of the next RR_DEPTH steps are in flight in registers (the loads of tile i + 1 used to leave one 32-column chain ahead
//     of their use: 64 tiles x one HBM round trip);
//   * 16 rows per workgroup instead of 64: 127 workgroups instead of 32 - a CU moves ~36 GB/s of this pattern, and 32 of them needed
//     57 us for the 65 MB whatever the chain cost (ablation: profiles/r06_detection_experiments.txt);
//   * the next 16 values of the chain are read from LDS while the current 16 are added.
#define RR_DEPTH 4
#define RR_ROWS 16
#define RR_COLS 256
__global__ __launch_bounds__(256) void rt_integ_rows_kernel(RtArgs a, int first, int P)
{
    static_assert(RC_BAND % RR_ROWS == 0, "the rows of a workgroup lie in one band of the column pass");
    // (one buffer: a thread stores, and then overwrites, its own elements only; a row pitch of 258 doubles: every access below is a 16-byte one,
    // and the 16 chain lanes - 4 banks each, 4 apart - cover the 64 banks exactly)
    __shared__ __align__(16) double tile[RR_ROWS][RR_COLS + 2];
    const int nls = rt_one_sweep(a, first) ? 0 : min(min(RT_TWO_PASS_SLOTS, P), *a.rt_n - first);      // (P: the chunk's scratch slots)      // (as in the column pass: gridDim.y detections at a time)
    if ((int)blockIdx.y >= nls) return;
    const int W = a.W, H = a.W, nb = (W + RC_BAND - 1) / RC_BAND;
    const int r0 = blockIdx.x * RR_ROWS;
    for (int ls = blockIdx.y; ls < nls; ls += (int)gridDim.y) {
    double *S = a.S + (int64_t)ls * a.SP * W;          // (rows are 128-byte aligned: SP is a multiple of 16)
    const double *T = a.colT + ((int64_t)ls * nb + r0 / RC_BAND) * W;     // column sums of the bands above this one
    // a lane moves PAIRS of columns (16-byte loads and stores: 18 memory instructions per tile and lane, so that RR_DEPTH - 1 tiles in
    // flight stay below the 64 a wave can have outstanding): 128 lanes per row, 2 rows per instruction of the workgroup
    const int lc = 2 * (threadIdx.x & 127), lr = threadIdx.x >> 7;
    const int ntiles = (W + RR_COLS - 1) / RR_COLS;
    double2 reg[RR_DEPTH][8], off[RR_DEPTH];
    // (loads are unconditional, from clamped addresses, and what lies outside the image is zeroed when the tile is USED: a conditional load
    // is a branch whose join waits for the data - the prefetch would be gone)
    const int ce = (W - 1) & ~1;                                          // the last even column: ce + 1 < SP
    auto fetch = [&](double2 (&x)[8], double2 &o, int i) {
        const int c = i * RR_COLS + lc;
        o.x = T[min(c, W - 1)];
        o.y = T[min(c + 1, W - 1)];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = *reinterpret_cast<const double2 *>(S + (int64_t)min(r0 + 2 * k + lr, H - 1) * a.SP + min(c, ce));
    };
#pragma unroll
    for (int d = 0; d < RR_DEPTH; d++) fetch(reg[d], off[d], min(d, ntiles - 1));
    double acc = 0;
    // tile i out of its registers, the tile RR_DEPTH steps later into them.  Nothing between two uses of a register set is conditional:
    // the compiler's wait for "these loads" counts the memory instructions that are CERTAIN to have followed them - behind `if`s, none
    auto step = [&](double2 (&x)[8], double2 &o, int i) {
        const int c = i * RR_COLS + lc;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool rin = r0 + 2 * k + lr < H;
            *reinterpret_cast<double2 *>(&tile[2 * k + lr][lc]) =
                make_double2(rin && c < W ? __dadd_rn(x[k].x, o.x) : 0.0, rin && c + 1 < W ? __dadd_rn(x[k].y, o.y) : 0.0);
        }
        fetch(x, o, min(i + RR_DEPTH, ntiles - 1));                       // (past the end: the last tile again, never used)
        __syncthreads();
        if (threadIdx.x < RR_ROWS) {
            // (columns past the image hold zeros: the chain runs through them, nothing of it is stored)
            double2 *row = reinterpret_cast<double2 *>(tile[threadIdx.x]);
            double2 y[8], z[8];
#pragma unroll
            for (int j = 0; j < 8; j++) y[j] = row[j];
            for (int j0 = 0; j0 < RR_COLS / 2; j0 += 16) {                // (two chunks of 16 columns per turn: y and z swap roles, no copies)
#pragma unroll
                for (int j = 0; j < 8; j++) z[j] = row[j0 + 8 + j];
#pragma unroll
                for (int j = 0; j < 8; j++) { acc = __dadd_rn(acc, y[j].x); y[j].x = acc; acc = __dadd_rn(acc, y[j].y); y[j].y = acc; }
#pragma unroll
                for (int j = 0; j < 8; j++) row[j0 + j] = y[j];
                const int jn = min(j0 + 16, RR_COLS / 2 - 8);
#pragma unroll
                for (int j = 0; j < 8; j++) y[j] = row[jn + j];
#pragma unroll
                for (int j = 0; j < 8; j++) { acc = __dadd_rn(acc, z[j].x); z[j].x = acc; acc = __dadd_rn(acc, z[j].y); z[j].y = acc; }
#pragma unroll
                for (int j = 0; j < 8; j++) row[j0 + 8 + j] = z[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int r = r0 + 2 * k + lr;
            const double2 t2 = *reinterpret_cast<const double2 *>(&tile[2 * k + lr][lc]);
            if (r < H && c + 1 < W) *reinterpret_cast<double2 *>(S + (int64_t)r * a.SP + c) = t2;
            else if (r < H && c < W) S[(int64_t)r * a.SP + c] = t2.x;
        }
    };
    int i0 = 0;
    for (; i0 + RR_DEPTH <= ntiles; i0 += RR_DEPTH) {
#pragma unroll
        for (int d = 0; d < RR_DEPTH; d++) step(reg[d], off[d], i0 + d);
    }
#pragma unroll
    for (int d = 0; d < RR_DEPTH - 1; d++)
        if (i0 + d < ntiles) step(reg[d], off[d], i0 + d);
    __syncthreads();                                   // (the tile is the next detection's)
    }
}

// ------------------------------------------------------------------------------------------------ K1+K2 fused: one sweep
// One workgroup per detection walks the image in bands of RI_ROWS = 64 rows and, inside a band, tile by tile (64 columns): a "phase" is
// one (band, tile), 64 x 64 pixels.  The four column waves are stacked: wave w owns the band's rows 16 w .. 16 w + 15 (a "quarter"),
// lane = column; the fifth wave is the row wave, lane = row of the band.  For every phase i:
//   A1(i) column waves: the quarter's 16 pixels of the lane's column (computed from the polar record, see rt_pixel) -> v[], their
//         sum -> tot[w][column]; the wave that owns the tile's column sums (tile & 3) publishes what lies above the band -> cb[column]
//   A2(i) column waves: cb + the totals of the quarters above + the quarter's pixels one after the other -> tile[row][column]; the
//         owner adds the four totals to its running sum.  (Every partial column sum is EXACT in float64 in any order - see the
//         column pass above - so the quarters change no bit of NumPy's sequential cumsum.)
//   B(i)  the row wave: the row's running sum walks through the tile's 64 columns (carried in a register from tile to tile) - the
//         second cumsum, in place, in NumPy's order: the only rounding chain of the kernel, 64 dependent additions a phase
//   C(i)  the row wave, two rows per instruction: the quarters of the tile that are read go to the integral image
// Tiles and tot / cb are double-buffered by the phase's parity; one barrier per phase.  Between barriers i and i + 1 the column waves
// run A2(i), then A1(i+1), on buffer i & 1, and the row wave B(i-1), then C(i-1), on the other buffer; tot / cb of phase i are read while
// those of phase i + 1 are written.  (With C in the column waves - every wave its own quarter, two phases behind - they were what a
// phase waited for: taps 66 %, C 16 % of their time, the row wave idle for 79 % of it.)
// Before that a phase was 16 rows x 256 columns (the column waves side by side): the same pixels, but 256 dependent additions and
// 128 LDS instructions of the row wave per phase with 16 of its lanes, which the column waves waited for (profiles/ROUNDS.md).
// The float64 image is written ONCE (32.8 MB per detection instead of the 98.6 MB moved by the two-pass kernels above, which stay
// for small chunks - see rt_one_sweep - and for image sizes above 2048).
#define RI_ROWS 64                          // rows of a band
#define RI_WAVES 4                          // column waves = quarters of a band
#define RI_Q (RI_ROWS / RI_WAVES)           // rows of a quarter: the height of a tile of the need / lit matrices and of boxtab
#define RI_TILES (2048 / 64)                // tiles of a band of the largest image
#define RI_OWN (RI_TILES / RI_WAVES)        // tiles whose column sums a column wave carries
#ifndef RI_BD
#define RI_BD 4                             // batches of eight columns the row wave reads ahead of its chain
#endif
#define RI_TP 66                            // tile pitch in doubles: even, the row wave moves two columns per LDS instruction; lane-per-row 16-byte
                                            // reads start at bank (4 r + 2 c) mod 64: no conflict within an instruction's lane groups
#define RI_LDS_BYTES (2 * RI_ROWS * RI_TP * 8)                // two tile buffers (the same 67 584 bytes as 2 x 4 tiles of 16 rows)
// static LDS beside them: tot 4 096 + cb 1 024 (new with the quarters), the boxes, the code table 1 024.  Two workgroups per CU have
// 81 920 bytes each: the phase list left LDS (scalar loads from a.phlist) and a box shrank 2 560 -> 2 048 bytes (a few more patches on
// the gather path; 1 536 -> 2 560 was worth 2 %)
#define RI_BOX 2048
static_assert(RI_LDS_BYTES + 2 * RI_WAVES * 64 * 8 + 2 * 64 * 8 + RI_WAVES * RI_BOX + 256 * 4 <= 81920, "two workgroups per CU");
// the polar footprint of every (quarter, tile) patch - 16 rows x 64 columns - of the sweep depends on the sampling map only: computed
// once per engine (one wave per patch, the reduction the integral kernel used to redo for every detection and phase: 24 cross-lane
// exchanges).  Entry (4 band + wave) * RI_TILES + tile; a quarter below the image is empty.
__global__ __launch_bounds__(64) void rt_boxtab_kernel(const uint32_t *__restrict__ map, int W, int cols, uint32_t *__restrict__ boxtab)
{
    const int H = W, lane = threadIdx.x;
    const int idx = blockIdx.x, tile = idx % RI_TILES, quarter = idx / RI_TILES;
    const int c = min(tile * 64 + lane, W - 1);
    int mnx = 0x7fffffff, mxx = -1, mny = 0x7fffffff, mxy = -1;
    for (int k = 0; k < RI_Q; k++) {
        if (quarter * RI_Q + k >= H) break;
        const uint32_t m = map[(int64_t)(quarter * RI_Q + k) * W + c];
        const int ix = m & 4095, iy = (m >> 12) & 1023;
        if (ix < cols) { mnx = min(mnx, ix); mxx = max(mxx, ix); mny = min(mny, iy); mxy = max(mxy, iy); }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, d)); mxx = max(mxx, __shfl_xor(mxx, d));
        mny = min(mny, __shfl_xor(mny, d)); mxy = max(mxy, __shfl_xor(mxy, d));
    }
    if (lane == 0) {
        boxtab[2 * idx] = mxx < 0 ? 0xffff0000u : ((uint32_t)mnx | ((uint32_t)mxx << 16));
        boxtab[2 * idx + 1] = mxx < 0 ? 0u : ((uint32_t)mny | ((uint32_t)mxy << 16));
    }
}

// a phase-list entry: band | tile << 8 | (quarters of the tile the determinant kernel reads, one bit per column wave) << 16
#define RI_E_BAND(e) ((int)((e) & 63u))
#define RI_E_TILE(e) ((int)(((e) >> 8) & 31u))
#define RI_E_BITS(e) ((uint32_t)(((e) >> 16) & 15u))
#define RI_E_MAKE(band, tile, bits) ((uint32_t)(band) | ((uint32_t)(tile) << 8) | ((uint32_t)(bits) << 16))

#ifdef RI_PROF
__device__ unsigned long long ri_prof[16];
extern "C" int roam_debug_integral_prof(unsigned long long *out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(ri_prof), sizeof(ri_prof)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(ri_prof), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#define RI_P(k) { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); rip_[k] += tn_ - rit_; rit_ = tn_; }
#else
#define RI_P(k)
#endif
__global__ __launch_bounds__(64 * (RI_WAVES + 1)) void rt_integral_kernel(RtArgs a, int first)
{
#ifdef RI_PROF
    unsigned long long rip_[8] = {0}, rit_ = __builtin_amdgcn_s_memtime();
#endif
    extern __shared__ __align__(16) double ri_lds[];
    const int ls = (int)blockIdx.x, slot = first + ls;
    if (slot >= *a.rt_n || !rt_one_sweep(a, first) || a.fused) return;
    typedef double Tile[RI_ROWS][RI_TP];
    Tile *tiles = reinterpret_cast<Tile *>(ri_lds);                        // [2]
    const int W = a.W, H = a.W, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    __shared__ float lut[256];
    __shared__ __align__(4) uint8_t box[RI_WAVES][RI_BOX];
    __shared__ double tot[2][RI_WAVES][64];                                // the quarters' column totals of a phase
    __shared__ double cb[2][64];                                           // the tile's column sums above the band
    if (t < 256) lut[t] = rt_code_to_f32(t);
    // the phases to walk, in sweep order (retrack_build_phases: a phase is left out when nothing in it is lit and its row sums are
    // either still zero or never read again).  Every wave reads the entries it needs as scalars, a few phases ahead of their use (the
    // list does not change while kernels run: the constant address space makes the loads scalar ones)
    typedef const uint32_t __attribute__((address_space(4))) *RiConstPtr;
    const RiConstPtr phc = (RiConstPtr)(uintptr_t)a.phlist;
    const int nph = (int)phc[0];
    auto ph_ent = [&](int i) { return i < nph ? phc[1 + i] : 0u; };
    __syncthreads();
    if (wave < RI_WAVES) {
        // ------------------------------------------------------------------------------------ column waves: A2(i), A1(i+1)
        const uint8_t *p = a.pool + (int64_t)a.rt_scan[slot] * a.rec_bytes + a.payload_off;
        double *S = a.S + (int64_t)ls * a.SP * W;
        const int SP = a.SP;
        const int rows = a.rows, cols = a.cols, stride = a.stride;
        const int wave_u = __builtin_amdgcn_readfirstlane(wave);
        // the running sums of the columns of the tiles this wave owns (tile & 3 == wave).  own[0] is always the sum of the tile group
        // `gcur` (tile >> 2): the array is rotated until it is (8 register moves a step; an array indexed by the group was kept in scratch
        // memory by the compiler: 16 MB of extra HBM writes per detection); the phases the list leaves out have dark pixels only
        double own[RI_OWN];
#pragma unroll
        for (int g = 0; g < RI_OWN; g++) own[g] = 0.0;
        int gcur = 0;
        uint32_t m[RI_Q];                                                  // the map words of the NEXT A1, in flight
        uint32_t ext0 = 0, ext1 = 0;                                       // the polar footprint (boxtab) of the patch of the A1 after the next, in flight
        uint32_t cur0 = 0xffff0000u, cur1 = 0;                             // ... of the next A1 (wave-uniform)
        uint32_t raw[8];                                                   // the first eight pieces of the next A1's box, in flight (prefetch_box)
        auto fetch = [&](uint32_t e) {
            const int c = min(RI_E_TILE(e) * 64 + lane, W - 1), r0 = RI_E_BAND(e) * RI_ROWS + wave_u * RI_Q;
#pragma unroll
            for (int k = 0; k < RI_Q; k++) m[k] = a.map[(int64_t)min(r0 + k, H - 1) * W + c];
        };
        auto fetch_ext = [&](uint32_t e) {
            const uint32_t *bt = a.boxtab + 2 * ((RI_E_BAND(e) * RI_WAVES + wave_u) * RI_TILES + RI_E_TILE(e));
            ext0 = bt[0]; ext1 = bt[1];
        };
        // geometry of a patch's polar box out of its table entry (all wave-uniform)
        struct Box { int mnx, mxx, mny, mxy, bh, bp, nrg, ncb; bool staged, inside; };
        auto geom = [&](uint32_t e0, uint32_t e1) {
            Box b;
            b.mnx = e0 & 0xffff; b.mxx = (e0 >> 16) == 0xffff ? -1 : (int)(e0 >> 16); b.mny = e1 & 0xffff; b.mxy = e1 >> 16;
            const int bw = b.mxx - b.mnx + 2;
            b.bh = b.mxy - b.mny + 2; b.bp = (bw + 3) & ~3;
            b.nrg = (b.bh + 3) >> 2; b.ncb = (b.bp + 63) >> 6;             // pieces of 4 polar rows x 64 bytes, one load instruction each
            b.staged = b.mxx >= 0 && b.bp * b.bh <= RI_BOX && cols >= 4;
            // the box lies inside the scan with a margin: no azimuth wrap, no bin past the last one
            b.inside = b.staged && b.mny >= 1 && b.mny - 1 + 4 * b.nrg <= rows && b.mnx + 64 * b.ncb <= cols;
            return b;
        };
        const int sub = lane >> 4, c4 = (lane & 15) * 4;
        // pieces q0 .. q0 + 7 of an `inside` box: a piece is "uniform base + the lane's own offset" for the load and for the LDS store
        auto load_pieces = [&](const Box &b, int q0) {
            const uint8_t *pl = p + (sub * stride + c4);
            const int npiece = b.nrg * b.ncb;
            int kg = (q0 / b.ncb) * 4, cb_ = (q0 % b.ncb) * 64;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (q0 + u < npiece) raw[u] = reinterpret_cast<const RtU32 *>(pl + ((b.mny - 1 + kg) * stride + b.mnx + cb_))->v;
                cb_ += 64;
                if (cb_ >= b.bp) { cb_ = 0; kg += 4; }
            }
        };
        auto store_pieces = [&](const Box &b, int q0, uint8_t *bx) {
            uint8_t *bl = bx + (sub * b.bp + c4);
            const int npiece = b.nrg * b.ncb;
            int kg = (q0 / b.ncb) * 4, cb_ = (q0 % b.ncb) * 64;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if (q0 + u < npiece && sub < b.bh - kg && c4 < b.bp - cb_) *reinterpret_cast<uint32_t *>(bl + (kg * b.bp + cb_)) = raw[u];
                cb_ += 64;
                if (cb_ >= b.bp) { cb_ = 0; kg += 4; }
            }
        };
        // The first eight pieces of the NEXT A1's box leave one phase ahead (its extent came out of the table a phase before that): their
        // HBM / L2 round trip - 37 % of a column wave's time when the loads were issued inside the phase that needs them (s_memtime) -
        // passes while the row wave works on the tile in between
        auto prefetch_box = [&]() {
            cur0 = __builtin_amdgcn_readfirstlane(ext0); cur1 = __builtin_amdgcn_readfirstlane(ext1);
            const Box b = geom(cur0, cur1);
            if (b.inside) load_pieces(b, 0);
        };
        float v[RI_Q];                                                     // the pixels of the phase A1 has prepared for A2
        double vtot = 0.0;                                                 // ... and their sum
        // the owner of a tile's column sums brings them to own[0]
        auto rotate_to = [&](int g) {
            while (gcur != g) {
                const double s0 = own[0];
#pragma unroll
                for (int q = 0; q + 1 < RI_OWN; q++) own[q] = own[q + 1];
                own[RI_OWN - 1] = s0;
                gcur = (gcur + 1) % RI_OWN;
            }
        };
        auto A1 = [&](int i, uint32_t e_i, uint32_t e_n1, uint32_t e_n2) {  // phase i of the list: the patch's pixels -> v[]; e_n1 / e_n2: the entries of the next two phases
            // The polar footprint of the wave's 64 x 16 pixel patch is a small box (range span x azimuth span, a few hundred bytes):
            // it is copied into LDS with a handful of coalesced row loads (16 lanes per polar row, four rows per instruction) and
            // the 4 taps per pixel become LDS byte reads; per-lane byte gathers from global memory (two 16-bit loads per pixel,
            // 32 wave-level gathers per phase) kept the texture addresser busy for 8 of this kernel's 19 us.  Patches whose box
            // does not fit (next to the image centre, across the 0 / 2 pi seam) gather as before.
            // extent of the patch's polar footprint: out of the table (the same for every detection), as wave-uniform values
            const Box b = geom(cur0, cur1);
            const int mnx = b.mnx, mny = b.mny, bh = b.bh, bp = b.bp;
            if (b.mxx < 0) {
#pragma unroll
                for (int k = 0; k < RI_Q; k++) v[k] = 0.f;                 // beyond the maximum range, or a quarter below the image
            } else if (b.staged) {
                uint8_t *bx = box[wave];
                if (b.inside) {
                    // (the general form below spends ~20 instructions per piece on clamps and addresses: a sixth of this kernel)
                    const int npiece = b.nrg * b.ncb;
                    for (int q0 = 0; q0 < npiece; q0 += 8) {
                        if (q0 > 0) load_pieces(b, q0);                    // (the first eight came with prefetch_box)
                        store_pieces(b, q0, bx);
                    }
                } else
                for (int kg = 0; kg < bh; kg += 4) {
                    const int kk = kg + sub;
                    int r = mny + kk - 1;
                    if (r < 0) r += rows; else if (r >= rows) r -= rows;
                    for (int cb_ = 0; cb_ < bp; cb_ += 64) {
                        const int cc = cb_ + c4;
                        if (kk < bh && cc < bp) {
                            // bytes beyond the scan's last range bin read as zero: the load is moved back inside the row and shifted
                            const int x0 = mnx + cc, xl = min(x0, cols - 4), sh = 8 * (x0 - xl);
                            uint32_t rw = 0;
                            if (sh < 32) rw = reinterpret_cast<const RtU32 *>(p + r * stride + xl)->v >> sh;
                            *reinterpret_cast<uint32_t *>(bx + kk * bp + cc) = rw;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < RI_Q; k++) {
                    const uint32_t mk = m[k];
                    const int ix = mk & 4095, iy = (mk >> 12) & 1023;
                    float r_ = 0.f;
                    if (ix < cols) {
                        const float wx1 = __fmul_rn((float)((mk >> 22) & 31), 1.f / 32.f), wx0 = __fsub_rn(1.f, wx1);
                        const float wy1 = __fmul_rn((float)(mk >> 27), 1.f / 32.f), wy0 = __fsub_rn(1.f, wy1);
                        const uint8_t *q = bx + (iy - mny) * bp + (ix - mnx);
                        const float s00 = lut[q[0]], s01 = lut[q[1]], s10 = lut[q[bp]], s11 = lut[q[bp + 1]];   // lut[0] = 0: bins past the scan
                        r_ = __fmul_rn(s00, __fmul_rn(wy0, wx0));
                        r_ = __fadd_rn(r_, __fmul_rn(s01, __fmul_rn(wy0, wx1)));
                        r_ = __fadd_rn(r_, __fmul_rn(s10, __fmul_rn(wy1, wx0)));
                        r_ = __fadd_rn(r_, __fmul_rn(s11, __fmul_rn(wy1, wx1)));
                    }
                    v[k] = r_;
                }
            } else {
#pragma unroll
                for (int k = 0; k < RI_Q; k++) v[k] = rt_pixel(m[k], p, rows, cols, stride, lut);
            }
            // the next phase's map words leave now; they land while the row wave works
            if (i + 1 < nph) {
                fetch(e_n1);
                prefetch_box();
                if (i + 2 < nph) fetch_ext(e_n2);
            }
            // the quarter's total (rows below the image - their map words are the last row's - count as zero: s + 0.0 = s), and what
            // lies above the band from the tile's owner
            const int nlive = H - (RI_E_BAND(e_i) * RI_ROWS + wave_u * RI_Q);
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < RI_Q; k++) {
                if (k >= nlive) v[k] = 0.f;
                s = __dadd_rn(s, (double)v[k]);
            }
            vtot = s;
            tot[i & 1][wave][lane] = s;
            if ((RI_E_TILE(e_i) & (RI_WAVES - 1)) == wave_u) {
                rotate_to(RI_E_TILE(e_i) / RI_WAVES);
                cb[i & 1][lane] = own[0];
            }
        };
        auto A2 = [&](int i, uint32_t e_i) {                               // (after the barrier behind A1(i): the other waves' totals)
            const bool owner = (RI_E_TILE(e_i) & (RI_WAVES - 1)) == wave_u;    // (own[0] is this tile's sum since A1(i))
            double s = cb[i & 1][lane], sum = vtot;
#pragma unroll
            for (int q = 0; q < RI_WAVES; q++) {
                if (q == wave_u || !(q < wave_u || owner)) continue;       // (wave-uniform: at most four LDS reads for a wave that owns nothing here)
                const double tq = tot[i & 1][q][lane];
                if (q < wave_u) s = __dadd_rn(s, tq);
                sum = __dadd_rn(sum, tq);
            }
            if (owner) own[0] = __dadd_rn(own[0], sum);
            double (*tl)[RI_TP] = tiles[i & 1] + wave * RI_Q;
#pragma unroll
            for (int k = 0; k < RI_Q; k++) {
                s = __dadd_rn(s, (double)v[k]);
                tl[k][lane] = s;
            }
        };
        // entries of phases i .. i + 3 as scalars
        uint32_t e_0 = ph_ent(0), e_1 = ph_ent(1), e_2 = ph_ent(2), e_3 = ph_ent(3);
        if (nph > 0) {
            fetch(e_0);
            fetch_ext(e_0);
            prefetch_box();
            if (nph > 1) fetch_ext(e_1);
            A1(0, e_0, e_1, e_2);
        }
#pragma unroll 1
        for (int i = 0; i < nph + 1; i++) {
            const uint32_t e_4 = ph_ent(i + 4);                            // (lands while this phase runs)
            RI_P(0)
            __syncthreads();                                               // A1(i), A2(i-1), B(i-2) and C(i-2) are complete
            RI_P(1)
            if (i < nph) A2(i, e_0);
            RI_P(2)
            if (i + 1 < nph) A1(i + 1, e_1, e_2, e_3);
            RI_P(3)
            e_0 = e_1; e_1 = e_2; e_2 = e_3; e_3 = e_4;
        }
    } else {
        // ------------------------------------------------------------------------------------ the row wave: B(i-1), C(i-1)
        double *S = a.S + (int64_t)ls * a.SP * W;
        const int SP = a.SP;
        const int half = lane >> 5, c2 = 2 * (lane & 31);                  // C: a lane moves two columns, an instruction two rows
        double carry = 0.0;                                                // running sum of row band * RI_ROWS + lane
        int pband = -1;
        uint32_t e_nx = ph_ent(0);
        for (int i = 0; i < nph + 1; i++) {
            const uint32_t e = e_nx;                                       // the entry of phase i - 1
            if (i >= 1) e_nx = ph_ent(i);
            RI_P(5)
            __syncthreads();
            RI_P(6)
            if (i < 1) continue;
            const int band = RI_E_BAND(e), tile = RI_E_TILE(e);
            if (band != pband) { carry = 0.0; pband = band; }              // (the phases a band leaves out on its left have sums of zero)
            if (band * RI_ROWS + lane < H) {
                const int ncols = min(64, W - tile * 64);
                double *row = tiles[(i - 1) & 1][lane];
                int j = 0;
                if (ncols >= 16) {
                    // batches of eight columns (eight dependent float64 additions), 16-byte LDS accesses (two columns per instruction)
                    auto rd = [&](double(&x)[8], int jj) {
                        const double2 *q = reinterpret_cast<const double2 *>(row + jj);
#pragma unroll
                        for (int u = 0; u < 4; u++) { const double2 v2 = q[u]; x[2 * u] = v2.x; x[2 * u + 1] = v2.y; }
                    };
                    auto chain_wr = [&](double(&x)[8], int jj) {
#pragma unroll
                        for (int u = 0; u < 8; u++) { carry = __dadd_rn(carry, x[u]); x[u] = carry; }
                        double2 *q = reinterpret_cast<double2 *>(row + jj);
#pragma unroll
                        for (int u = 0; u < 4; u++) q[u] = make_double2(x[2 * u], x[2 * u + 1]);
                    };
                    // RI_BD batches of eight columns are in flight ahead of the chain: beside eight column waves' tap reads an LDS read
                    // takes several hundred cycles to come back, and one batch ahead the chain waited for it at every batch
                    double xr[RI_BD][8];
#pragma unroll
                    for (int u = 0; u < RI_BD; u++)
                        if (8 * u + 8 <= ncols) rd(xr[u], 8 * u);
                    for (; j + 8 * RI_BD <= ncols; j += 8 * RI_BD) {
#pragma unroll
                        for (int u = 0; u < RI_BD; u++) {
                            chain_wr(xr[u], j + 8 * u);
                            if (j + 8 * (RI_BD + u) + 8 <= ncols) rd(xr[u], j + 8 * (RI_BD + u));
                        }
                    }
                    // (what is left of the tile - fewer than RI_BD batches - is in the registers already)
#pragma unroll
                    for (int u = 0; u < RI_BD; u++)
                        if (j + 8 <= ncols) { chain_wr(xr[u], j); j += 8; }
                }
                for (; j < ncols; j++) {
                    carry = __dadd_rn(carry, row[j]);
                    row[j] = carry;
                }
            }
            RI_P(7)
            // C: the quarters of the tile that are read go to the image, 16-byte accesses (W and SP are even: a pair of columns is inside
            // the image or outside, and aligned); eight row pairs in flight
            if (tile * 64 + c2 < W) {
                const double (*tl)[RI_TP] = tiles[(i - 1) & 1];
                double *q = S + (int64_t)(band * RI_ROWS + half) * SP + tile * 64 + c2;
                for (int w = 0; w < RI_WAVES; w++) {
                    if (!((RI_E_BITS(e) >> w) & 1u)) continue;             // does anything read this quarter of the tile?
                    double2 x[RI_Q / 2];
#pragma unroll
                    for (int k = 0; k < RI_Q / 2; k++) x[k] = *reinterpret_cast<const double2 *>(&tl[w * RI_Q + 2 * k + half][c2]);
#pragma unroll
                    for (int k = 0; k < RI_Q / 2; k++)
                        if (band * RI_ROWS + w * RI_Q + 2 * k + half < H) *reinterpret_cast<double2 *>(q + (int64_t)(w * RI_Q + 2 * k) * SP) = x[k];
                }
            }
        }
    }
#ifdef RI_PROF
    if (lane == 0 && (wave == 0 || wave == RI_WAVES)) for (int k = 0; k < 8; k++) atomicAdd(&ri_prof[k + (wave == 0 ? 0 : 8)], rip_[k]);
#endif
}

size_t retrack_boxtab_words(int W) { return 2 * (size_t)((W + RI_ROWS - 1) / RI_ROWS) * RI_WAVES * RI_TILES; }

hipError_t launch_retrack_boxtab(hipStream_t st, const uint32_t *map, int W, int cols, uint32_t *boxtab)
{
    hipLaunchKernelGGL(rt_boxtab_kernel, dim3((unsigned)(retrack_boxtab_words(W) / 2)), dim3(64), 0, st, map, W, cols, boxtab);
    return hipGetLastError();
}
// ---- which phases of the one-sweep integral kernel matter (host code, once per engine; geometry only).
// The determinant kernel never reads the blocks of the integral image that only dark steps would touch (rt_darktab_kernel), so a 16-row x
// 64-column QUARTER TILE none of its strips loads need not be written; and a (band, tile) PHASE none of whose quarters is needed need
// not be computed when its row sums cannot matter: on a band's left while every column so far has seen no lit pixel down to the band's
// last row (the sums are exactly zero), on its right once nothing further along the band is needed.  Needed quarters contain every lit
// pixel (a lit pixel lies in the window of a lit step), so a phase that is left out has dark pixels only: the columns' running sums
// pass it unchanged.  out[0] = number of phases, out[1..] = RI_E_MAKE(band, tile, needed quarters) in sweep order.
size_t retrack_phase_words(int W) { return 1 + (size_t)((W + RI_ROWS - 1) / RI_ROWS) * RI_TILES; }
int retrack_band_rows() { return RI_ROWS; }

bool retrack_build_phases(const uint32_t *map, const uint32_t *darktab, int W, int cols, uint32_t *out)
{
    const int H = W, nbands = (H + RI_ROWS - 1) / RI_ROWS, ns = (W + SD_OUT - 1) / SD_OUT, nt = H / SD_T + 1, NT = RI_TILES;
    static_assert(RI_ROWS % SD_T == 0 && RI_Q % SD_T == 0, "a quarter of a band of the integral kernel is one or more blocks of the determinant kernel");
    const int ndet = (H + SD_T - 1) / SD_T;
    if (W > 64 * RI_TILES) return false;
    // need / lit: per (quarter, tile), 16 rows x 64 columns
    std::vector<uint8_t> need((size_t)nbands * RI_WAVES * NT, 0), lit((size_t)nbands * RI_WAVES * NT, 0);
    std::vector<int> firstlit(W, H);
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++)
            if ((int)(map[(size_t)r * W + c] & 4095u) < cols) {
                lit[(size_t)(r / RI_Q) * NT + c / 64] = 1;
                if (firstlit[c] == H) firstlit[c] = r;
            }
    for (int s = 0; s < ns; s++) {
        const uint32_t *T = darktab + (size_t)s * SD_DT_WORDS;
        const int t_first = (int)T[16], t_last = (int)T[17];
        if (t_first >= nt) continue;                                        // the strip sees nothing
        const int tb = t_first >= 1 ? ((t_first - 1) & ~3) : 0, te = std::min(nt, t_last + 2);
        const int cbase = s * SD_OUT - 1 - SD_HL, c_lo = std::max(cbase, 0), c_hi = std::min(cbase + SD_BP, W) - 1;
        for (int j = tb; j <= te + 3 && j < ndet; j++) {
            const bool in_loop = j >= tb + 4;                               // (the four blocks of the prologue are always loaded)
            if (in_loop && ((T[8 + ((j - 4) >> 5)] >> ((j - 4) & 31)) & 1u)) continue;
            for (int k = c_lo / 64; k <= c_hi / 64; k++) need[(size_t)(j * SD_T / RI_Q) * NT + k] = 1;
        }
    }
    const int ntile = (W + 63) / 64;
    int n = 0;
    bool sound = true;
    for (int b = 0; b < nbands; b++) {
        bool zero[RI_TILES];
        uint32_t bits[RI_TILES];
        const int rend = std::min(b * RI_ROWS + RI_ROWS - 1, H - 1);
        for (int k = 0; k < ntile; k++) {
            bits[k] = 0; zero[k] = true;
            for (int w = 0; w < RI_WAVES; w++) if (need[(size_t)(b * RI_WAVES + w) * NT + k]) bits[k] |= 1u << w;
            for (int c = k * 64; c < std::min(W, (k + 1) * 64); c++) if (firstlit[c] <= rend) { zero[k] = false; break; }
        }
        for (int k = 0; k < ntile; k++) {
            bool skipL = !bits[k], skipR = true;
            for (int q = 0; q <= k && skipL; q++) skipL = zero[q];
            for (int q = k; q < ntile && skipR; q++) skipR = !bits[q];
            if (skipL || skipR) {
                for (int w = 0; w < RI_WAVES; w++) if (lit[(size_t)(b * RI_WAVES + w) * NT + k]) sound = false;      // (cannot happen: see above)
                continue;
            }
            out[1 + n++] = RI_E_MAKE(b, k, bits[k]);
        }
    }
    if (!sound) {                                                           // belt and braces: walk everything, write everything
        n = 0;
        for (int b = 0; b < nbands; b++)
            for (int k = 0; k < ntile; k++) {
                uint32_t all = 0;
                for (int w = 0; w < RI_WAVES; w++) if (b * RI_ROWS + w * RI_Q < H) all |= 1u << w;
                out[1 + n++] = RI_E_MAKE(b, k, all);
            }
    }
    out[0] = (uint32_t)n;
    return true;
}

// pixels of the integral image the phases of a list write: its needed quarter tiles, clipped to the image
int64_t retrack_phase_pixels(const uint32_t *ph, int W)
{
    int64_t px = 0;
    for (uint32_t i = 0; i < ph[0]; i++) {
        const uint32_t e = ph[1 + i];
        const int wcols = std::max(0, std::min(64, W - RI_E_TILE(e) * 64));
        for (int w = 0; w < RI_WAVES; w++)
            if ((RI_E_BITS(e) >> w) & 1u) px += (int64_t)std::max(0, std::min(RI_Q, W - (RI_E_BAND(e) * RI_ROWS + w * RI_Q))) * wcols;
    }
    return px;
}

hipError_t retrack_integral_init() { return hipFuncSetAttribute(reinterpret_cast<const void *>(rt_integral_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, RI_LDS_BYTES); }

hipError_t launch_retrack_integral(hipStream_t st, const RtArgs &a, int first, int P, bool one_sweep)
{
    if (one_sweep) hipLaunchKernelGGL(rt_integral_kernel, dim3(P), dim3(64 * (RI_WAVES + 1)), RI_LDS_BYTES, st, a, first);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;      // (a refused launch - LDS attribute, grid - surfaces here, not after the chain)
    // (the two-pass form of chunks below RT_TWO_PASS_SLOTS detections; its band totals live in a.colT, RT_TWO_PASS_SLOTS entries)
    const int W = a.W, P2 = min(P, RT_TWO_PASS_SLOTS);
    hipLaunchKernelGGL(rt_integ_cols_kernel, dim3((W + 63) / 64, (W + RC_BAND - 1) / RC_BAND, min(P2, RT_TWO_PASS_Z)), dim3(256), 0, st, a, first, P2);
    hipLaunchKernelGGL(rt_integ_rows_kernel, dim3((W + RR_ROWS - 1) / RR_ROWS, min(P2, RT_TWO_PASS_Z)), dim3(256), 0, st, a, first, P2);
    return hipGetLastError();
}
