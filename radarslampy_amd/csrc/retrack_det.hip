// retrack_det.hip - K3 of the device-side feature (re)detection (overview: retrack.hip): determinants + maxima, and K1-K3 fused
#include "doh_common.h"
#include "retrack_geom.h"

// A maximum goes straight onto the detection's candidate list, in whatever order the workgroups get there; rt_emit_kernel sorts the
// list into the reference's (row, column, layer) order.  (Round 2's first version wrote a 1-byte mask per pixel plus row counts
// and had the emission kernel scan the mask and compute every candidate's determinant again from global memory: 4 MB more
// traffic per detection and 1.1-1.7 ms of latency per chunk.)
__device__ __forceinline__ void rt_push_maxima(const RtArgs &a, int ls, int r, int c, uint32_t bits, double v0, double v1)
{
#pragma unroll
    for (int l = 0; l < 2; l++)
        if ((bits >> l) & 1u) {
            const int o = atomicAdd(&a.cand_n[ls], 1);
            if (o < BP_MAX_PTS) {
                a.cand_rc[(int64_t)ls * BP_MAX_PTS + o] = ((uint32_t)r << 16) | ((uint32_t)c << 2) | (uint32_t)(l + 1);
                a.cand_val[(int64_t)ls * BP_MAX_PTS + o] = l ? v1 : v0;
            }
        }
}

// ------------------------------------------------------------------------------------------------ K3: determinants + maxima (strip march)
// Box sizes (15, 30) = int(3 sigma) of the engine's detector parameters, compile-time.  Round 2's kernel staged a 62 x 94 block of the
// integral image per 30 x 62 outputs: every byte of the image was fetched 3.1 times and the L2 captured none of it (PMC: 53.7 GB per
// 512 detections against 16.8 GB algorithmic).  Here a workgroup of 8 waves owns a column STRIP of 62 outputs (SD_HALVES = 2: 16
// waves, 126 outputs) and marches DOWN the image: the rows of the integral image live in an LDS ring of 64 rows x 94 columns, every
// step loads the SD_T NEW rows only (prefetched into registers three steps ahead) and computes SD_T x 64 determinant positions, so
// a byte is fetched 94 / 62 = 1.5 times before L2 and 1.36 times from HBM (PMC; SD_HALVES = 2: 1.25 / 1.06, but one workgroup per
// CU and 10 % slower) and the vertical halos (box rows and the 3 x 3 x 3 maxima) cost nothing: the maxima of a step's last row are
// decided one step later from a two-row seam kept with the per-position maxima.
//   * ONE barrier per step: the rows step t + 1 needs are written into ring slots that step t does not read (64 slots, 46 live
//     rows, 16 new ones), the per-position maxima are double-buffered - staging, the maxima of step t - 1 and the determinants of
//     step t run between the same two barriers, on different waves at different times.
//   * ring addressing without arithmetic: the step loop is unrolled by four, so the ring row of (step phase, position row, box
//     offset) is a compile-time constant; the wave's own row term (0..7) sits in the base register, and rows 0..7 of the ring are
//     stored twice (also as rows 64..71) so that "constant + wave" never wraps.  DS offsets are 16 bits: two base registers per
//     column (ring rows 0..35 / 36..71).
//   * columns are clipped like skimage's _integ ONCE per thread: the twelve clipped corner columns of the dxx / dyy boxes are byte
//     offsets in registers, so the strips along the left / right image border run the same code as interior ones; rows need clipping
//     in the first and the last steps only (a variant with computed row offsets).  The dxy boxes (where dxx * dyy can pass the
//     threshold: ~4 % of the wave-rows) compute their addresses on the fly.
//   * the boxes of a thread and step are ONE stream of pairs, the reads of pair i + 1 issued before the arithmetic of pair i, and the
//     xx-side pair of a layer is read only by the waves in which a bound from dyy and the xx-mid box cannot rule dxx * dyy > threshold
//     out (sd_tile_fast: three waves in four skip it on the benchmark's scene); max(0, box) is the clamp modifier of the box's last subtraction (the ring
//     holds the image scaled by 2^-10).
//   * workgroup -> strip mapping is XCD-aware: the strips of a detection are consecutive workgroups of ONE XCD, started together
//     and marching in step, so that the cache lines neighbouring strips share come from that XCD's L2 (hit rate 25 %).
//   * a step whose window lies beyond the maximum range - the corners of the image - skips its boxes, and the blocks only such steps
//     would read are neither loaded nor staged (rt_darktab_kernel: a bit table per strip, geometry only).
#define SD_RING 64
#define SD_DUP 8
#define SD_PITCHB (SD_BP * 8)
#define SD_SPLIT 36
#define SD_THREADS (512 * SD_HALVES)
#define SD_RING_BYTES ((SD_RING + SD_DUP) * SD_PITCHB)
#define SD_M2_ROWS (SD_T + 2)
#define SD_LDS_BYTES (SD_RING_BYTES + 2 * SD_M2_ROWS * SD_PC * 8)
#define SD_NST ((SD_T * SD_BP + SD_THREADS - 1) / SD_THREADS)   // staged elements per thread and step (3)
extern __shared__ __align__(16) char sd_smem[];

// The ring holds the integral image scaled by 2^-10 (an exact operation that commutes with every rounding below), so that a box sum -
// at most 30 x 30 pixels of at most 1.0 - stays below 1 and skimage's max(0, sum) is the CLAMP output modifier of the box's last
// subtraction instead of a v_max_f64 of its own (8 of a position's 46 vector instructions); the 1 / size^2 factors carry the 2^10.
#define SD_SCALE 0.0009765625
#define SD_UNSCALE 1024.0
__device__ __forceinline__ double sd_box(double a, double d, double b, double c)
{
    const double t = __dsub_rn(__dadd_rn(a, d), b);
    double r;
    asm("v_add_f64 %0, %1, -%2 clamp" : "=v"(r) : "v"(t), "v"(c));
    return r;
}
// max of two determinants (never NaN): one v_max_f64 - fmax() canonicalises both operands first (three instructions)
__device__ __forceinline__ double sd_max(double x, double y)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
template <int SIZE> __device__ __forceinline__ double sd_wi() { return __dmul_rn(__ddiv_rn(__ddiv_rn(1.0, (double)SIZE), (double)SIZE), SD_UNSCALE); }

__device__ __forceinline__ double sd_ldr(const uint32_t (&ca)[12], const uint32_t (&cb)[12], int row, int j)
{
    const int rr = ((row % SD_RING) + SD_RING) % SD_RING;                  // (constants after unrolling)
    return rr < SD_SPLIT ? *reinterpret_cast<const double *>(sd_smem + (ca[j] + rr * SD_PITCHB))
                         : *reinterpret_cast<const double *>(sd_smem + (cb[j] + (rr - SD_SPLIT) * SD_PITCHB));
}

// dxx * dyy (hessian_det_pruned's first product) of a thread's two positions in a step whose box rows need no clipping; PH = step & 3.
// The boxes are ONE stream of pairs (the same box of both positions): the eight corner reads of pair i + 1 are issued before the
// arithmetic of pair i (the compiler's own order waited for every box's reads before it issued the next four), and the two
// positions' dependent float64 chains alternate instruction by instruction, so that a wave that is alone on its SIMD - the tail of
// every step: the hardware favours the oldest wave, the youngest finish last - still issues back to back.
//
// The xx-side box is read only where a bound cannot rule the product out.  A product at or below the threshold is used for one fact only,
// that it is at or below the threshold (rt_det_strip_kernel: no dxy term, no candidate, nothing a passing neighbour could not exceed), and
// most of that fact is known before the last box is read: the side box lies inside its mid box and every box sum is clamped at 0, so
// mid - 3 side lies in [-2 mid, mid] and dxx = -(mid - 3 side) w_i in [-mid w_i, 2 mid w_i].  With dyy exact (the bound from an exact dyy
// rules out more than the one from an exact dxx: profiles/det_screen_rate.py) and the product positive, dxx dyy > thr needs
//     |dyy| k mid_xx w_i > thr,    k = 2 where dyy > 0 (dxx > 0: side > mid / 3), k = 1 where dyy < 0 (dxx < 0: side < mid / 3).
// The stream is therefore, per layer, yy-mid, yy-side, xx-mid - six pairs, read ahead as before - and then the xx-side pair of a layer
// only if some lane of the wave, for either of its positions, is not ruled out (one ballot per layer; layer 15's is taken while layer
// 30's reads are in flight).  A layer the wave skips holds 0.0, as a dark step's positions do.
// The margin - a position is ruled out only if  fl(fl(|dyy| mid_xx) c_k) <= fl(thr - SD_SKIP_ABS),  c_k = fl(k w_i (1 + SD_SKIP_REL)):
//   * rounding: the bound rounds four times (c_k, its two products, thr - SD_SKIP_ABS), the kernel's dxx dyy four times (3 side,
//     mid - 3 side, the factor w_i, the product; dyy is the same number on both sides), every one monotone: together below 8 x 2^-53
//     relative, against SD_SKIP_REL = 2^-20.  A product that underflows is below 1e-300, and SD_SKIP_ABS covers that.
//   * a COMPUTED side sum can exceed its computed mid sum by the rounding of the integral image, delta (in image units).  The ~1e-9
//     quoted above rt_darktab_kernel is what one sees; the worst case of 8 corners x (H + W) roundings of half an ulp of H W is 1.5e-5
//     at the engine's 2024 x 2024 and 1.2e-4 at the 4094 x 4094 the launcher accepts.  Only k = 2 is touched (side >= 0 holds exactly,
//     so mid - 3 side <= mid does too): |mid - 3 side| <= 2 mid + 3 delta, and the product grows by at most |dyy| 3 delta / size^2
//     <= 6 delta / 225 (|dyy| <= 2: a box holds at most size^2 pixels of at most 1.0).  SD_SKIP_ABS = 2^-18 covers delta <= 1.4e-4.
//   * the 2^-10 that the ring's box sums carry is undone by w_i = 2^10 / size^2 (sd_wi), which the bound multiplies by as the kernel
//     does: both scalings are exact, and delta enters as delta 2^-10 w_i = delta / size^2, as used above.
// So: ruled out => the product as the kernel rounds it is at or below thr.  Never the reverse - a position that is not ruled out may
// still come out below - and a threshold below SD_SKIP_ABS rules nothing out, since a bound is never negative.  Against a threshold
// of 5e-4 the two margins cost no measurable skip rate.
#define SD_SKIP_REL 9.5367431640625e-07
#define SD_SKIP_ABS 3.814697265625e-06
template <int PH>
__device__ __forceinline__ void sd_tile_fast(const uint32_t (&ca)[12], const uint32_t (&cb)[12], double thr_s, double (&d0)[SD_T / 8], double (&d1)[SD_T / 8])
{
    static_assert(SD_T == 16, "two positions per thread and step");
    double v[2][2][4];                                                     // [pair slot][position][corner]
    auto issue = [&](int L, int q, double(&o)[2][4]) {                     // q: xx-mid, xx-side, yy-mid, yy-side (hessian_box 4..7)
        const int SIZE = L ? 30 : 15, s2 = (SIZE - 1) / 2, s3 = SIZE / 3;
        const int ra = q < 2 ? -s3 + 1 : (q == 2 ? -s2 : -(s3 / 2)), rb = ra + (q < 2 ? 2 * s3 - 1 : (q == 2 ? SIZE : s3));
        const int ja = 6 * L + (q == 0 ? 0 : (q == 1 ? 2 : 4)), jb = ja + 1;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int R0 = SD_T * PH + 8 * k;
            o[k][0] = sd_ldr(ca, cb, R0 + ra, ja); o[k][1] = sd_ldr(ca, cb, R0 + rb, jb);
            o[k][2] = sd_ldr(ca, cb, R0 + ra, jb); o[k][3] = sd_ldr(ca, cb, R0 + rb, ja);
        }
    };
    // the two positions' box sums of a pair, then -(mid - 3 side) w_i: the chains of the two positions alternate
    auto boxes = [&](const double(&x)[2][4], double(&b)[2]) {
        double t0 = __dadd_rn(x[0][0], x[0][1]), t1 = __dadd_rn(x[1][0], x[1][1]);
        t0 = __dsub_rn(t0, x[0][2]); t1 = __dsub_rn(t1, x[1][2]);
        asm("v_add_f64 %0, %1, -%2 clamp" : "=v"(b[0]) : "v"(t0), "v"(x[0][3]));
        asm("v_add_f64 %0, %1, -%2 clamp" : "=v"(b[1]) : "v"(t1), "v"(x[1][3]));
    };
    auto deriv = [&](int L, const double(&mid)[2], const double(&side)[2], double(&e)[2]) {
        const double w_i = L ? sd_wi<30>() : sd_wi<15>();
        const double m0 = __dmul_rn(3.0, side[0]), m1 = __dmul_rn(3.0, side[1]);
        const double e0 = __dsub_rn(mid[0], m0), e1 = __dsub_rn(mid[1], m1);
        e[0] = __dmul_rn(-e0, w_i); e[1] = __dmul_rn(-e1, w_i);
    };
    issue(0, 2, v[0]);
    double mid[2], b[2], dyy[2][2], xm[2][2];                              // dyy, xx-mid: [layer][position]
    bool need[2];                                                          // (wave-uniform) the layer's xx-side pair has to be read
#pragma unroll
    for (int i = 0; i < 6; i++) {                                          // per layer: yy-mid, yy-side, xx-mid
        const int L = i / 3, j = i % 3;
        if (i + 1 < 6) issue((i + 1) / 3, (i + 1) % 3 == 0 ? 2 : ((i + 1) % 3 == 1 ? 3 : 0), v[(i + 1) & 1]);
        boxes(v[i & 1], j == 0 ? mid : (j == 1 ? b : xm[L]));
        if (j == 1) deriv(L, mid, b, dyy[L]);
        if (j == 2) {
            const double w1 = __dmul_rn(L ? sd_wi<30>() : sd_wi<15>(), 1.0 + SD_SKIP_REL), w2 = __dmul_rn(2.0, w1);
            const double u0 = __dmul_rn(__dmul_rn(fabs(dyy[L][0]), xm[L][0]), dyy[L][0] > 0.0 ? w2 : w1);
            const double u1 = __dmul_rn(__dmul_rn(fabs(dyy[L][1]), xm[L][1]), dyy[L][1] > 0.0 ? w2 : w1);
            need[L] = __builtin_amdgcn_ballot_w64(u0 > thr_s || u1 > thr_s) != 0;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (need[0]) issue(0, 1, v[0]);
    if (need[1]) issue(1, 1, v[1]);
    d0[0] = 0.0; d0[1] = 0.0; d1[0] = 0.0; d1[1] = 0.0;
    if (need[0]) {
        double e[2];
        boxes(v[0], b); deriv(0, xm[0], b, e);
        d0[0] = __dmul_rn(e[0], dyy[0][0]); d0[1] = __dmul_rn(e[1], dyy[0][1]);
    }
    if (need[1]) {
        double e[2];
        boxes(v[1], b); deriv(1, xm[1], b, e);
        d1[0] = __dmul_rn(e[0], dyy[1][0]); d1[1] = __dmul_rn(e[1], dyy[1][1]);
    }
}

// the same product with the box rows clipped to the image (first / last steps of a strip): r = image row of the position (wave-uniform)
template <int SIZE, int L>
__device__ __forceinline__ double sd_det_rows(const uint32_t (&ca)[12], int w8, int r, int H)
{
    constexpr int s2 = (SIZE - 1) / 2, s3 = SIZE / 3, w = SIZE, J = 6 * L;
    const double w_i = sd_wi<SIZE>();
    auto ld = [&](int row, int j) { return *reinterpret_cast<const double *>(sd_smem + (ca[j] + (uint32_t)(((row & (SD_RING - 1)) - w8) * SD_PITCHB))); };
    const int xa = clipi(r - s3 + 1, 0, H - 1), xb = clipi(xa + 2 * s3 - 1, 0, H - 1);
    double mid = sd_box(ld(xa, J + 0), ld(xb, J + 1), ld(xa, J + 1), ld(xb, J + 0));
    double side = sd_box(ld(xa, J + 2), ld(xb, J + 3), ld(xa, J + 3), ld(xb, J + 2));
    double dxx = __dsub_rn(mid, __dmul_rn(3.0, side));
    dxx = __dmul_rn(-dxx, w_i);
    const int ya = clipi(r - s2, 0, H - 1), yb = clipi(ya + w, 0, H - 1), za = clipi(r - s3 / 2, 0, H - 1), zb = clipi(za + s3, 0, H - 1);
    mid = sd_box(ld(ya, J + 4), ld(yb, J + 5), ld(ya, J + 5), ld(yb, J + 4));
    side = sd_box(ld(za, J + 4), ld(zb, J + 5), ld(za, J + 5), ld(zb, J + 4));
    double dyy = __dsub_rn(mid, __dmul_rn(3.0, side));
    dyy = __dmul_rn(-dyy, w_i);
    return __dmul_rn(dxx, dyy);
}

// the dxy term of a position whose dxx * dyy passes the threshold (rare): addresses computed on the fly, clipping included
template <int SIZE>
__device__ __forceinline__ double sd_dxy(double det, int r, int c, int H, int W, int cbase)
{
    constexpr int s3 = SIZE / 3;
    const double w_i = sd_wi<SIZE>();
    const int r0 = clipi(r - s3, 0, H - 1), r1 = clipi(r0 + s3, 0, H - 1), r2 = clipi(r + 1, 0, H - 1), r3 = clipi(r2 + s3, 0, H - 1);
    const int c0 = clipi(c - s3, 0, W - 1), c1 = clipi(c0 + s3, 0, W - 1), c2 = clipi(c + 1, 0, W - 1), c3 = clipi(c2 + s3, 0, W - 1);
    auto at = [&](int rr, int cc) { return *reinterpret_cast<const double *>(sd_smem + (((rr & (SD_RING - 1)) * SD_BP + (cc - cbase)) * 8)); };
    const double tl = sd_box(at(r0, c0), at(r1, c1), at(r0, c1), at(r1, c0));
    const double br = sd_box(at(r2, c2), at(r3, c3), at(r2, c3), at(r3, c2));
    const double bl = sd_box(at(r0, c2), at(r1, c3), at(r0, c3), at(r1, c2));
    const double tr = sd_box(at(r2, c0), at(r3, c1), at(r2, c1), at(r3, c0));
    double dxy = __dsub_rn(__dsub_rn(__dadd_rn(bl, tr), tl), br);
    dxy = __dmul_rn(-dxy, w_i);
    return __dsub_rn(det, __dmul_rn(0.81, __dmul_rn(dxy, dxy)));
}

// ---- which steps of a strip see nothing: geometry only, once per engine.
// The Cartesian pixels beyond the maximum range (sampling-map word with ix >= cols: 21 % of the image, its four corners) are zero whatever
// the scan holds.  A step whose whole window - position rows 16 t .. 16 t + 15 with their box rows -14 .. +16, the strip's position columns
// with their box columns -14 .. +16 - lies there has box sums of exactly nothing (up to the rounding of the integral image's cumulative
// sums, ~1e-9, against a threshold of 5e-4): its determinants can neither pass the threshold nor exceed a passing neighbour, they count as
// 0.  Such a step skips the boxes; a 16-row block of the integral image that only such steps would read (steps j - 1, j, j + 1 for
// block j) is not loaded.  The lit steps of a strip are ONE run (the range limit is a circle): the march starts just above it and stops
// just below - the dark steps outside cost a barrier and a ring fill each, 40 % of a lit step.  Per strip SD_DT_WORDS words: [0, 8) bit
// t = step t is dark, [8, 16) bit t = the block loaded AT step t (block t + 4) can be skipped, [16] / [17] = first / last lit step
// (nt / -1: none).
// (Round 3's first version tested the block's sum out of the ring in every wave and step - four LDS reads and a wait in front of every
// step's boxes - and loaded every block.)
__global__ __launch_bounds__(256) void rt_darktab_kernel(const uint32_t *__restrict__ map, int W, int cols, uint32_t *__restrict__ tab)
{
    const int H = W, strip = blockIdx.x, t = blockIdx.y, c0 = strip * SD_OUT;
    const int ra = max(SD_T * t - SD_HL, 0), rb = min(SD_T * t + SD_T - 1 + SD_HR, H - 1);
    const int xa = max(c0 - 1 - SD_HL, 0), xb = min(c0 - 1 + SD_PC - 1 + SD_HR, W - 1);
    const int nx = xb - xa + 1, n = max(0, rb - ra + 1) * max(0, nx);
    int lit = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int r = ra + i / nx, c = xa + i % nx;
        if ((int)(map[(int64_t)r * W + c] & 4095u) < cols) lit = 1;
    }
    lit = __syncthreads_or(lit);
    if (threadIdx.x == 0 && !lit) atomicOr(&tab[strip * SD_DT_WORDS + (t >> 5)], 1u << (t & 31));
}
__global__ __launch_bounds__(256) void rt_darkskip_kernel(int nt, uint32_t *__restrict__ tab)
{
    uint32_t *T = tab + blockIdx.x * SD_DT_WORDS;
    const int t = threadIdx.x;
    auto dark = [&](int q) { return q < 0 || q >= nt || ((T[q >> 5] >> (q & 31)) & 1u); };     // steps that do not exist read nothing
    auto skip = [&](int j) { return dark(j - 1) && dark(j) && dark(j + 1); };
    if (skip(t + 4)) atomicOr(&T[8 + (t >> 5)], 1u << (t & 31));
    if (t == 0) {
        int first = nt, last = -1;
        for (int q = 0; q < nt; q++)
            if (!dark(q)) { if (first == nt) first = q; last = q; }
        T[16] = (uint32_t)first; T[17] = (uint32_t)last;
    }
}

template <int P> struct SdTag { static constexpr int value = P; };

__global__ __launch_bounds__(SD_THREADS) void rt_det_strip_kernel(RtArgs a, int first, int P, int nstrips)
{
    const int nact = min(P, max(0, *a.rt_n - first));
    if (a.fused && rt_one_sweep(a, first)) return;                          // rt_fused_kernel's chunk
    // XCD-aware order: workgroup id -> (XCD = id % 8, j = id / 8); XCD x owns the x-th contiguous eighth of the (detection, strip) list
    const int total = nact * nstrips, per = (total + 7) >> 3;
    const int xcd = blockIdx.x & 7, jq = blockIdx.x >> 3;
    const int work = xcd * per + jq;
    if (jq >= per || work >= total) return;
    const int ls = work / nstrips, strip = work - ls * nstrips;
    const int W = a.W, H = a.W, SP = a.SP;
    const double thr = a.threshold, thr_s = __dsub_rn(thr, SD_SKIP_ABS);   // thr_s: what sd_tile_fast's bound is held against
    typedef const uint32_t __attribute__((address_space(4))) *SdConstPtr;     // constant address space + uniform address = scalar load
    const SdConstPtr dtab = (SdConstPtr)(uintptr_t)(a.darktab + strip * SD_DT_WORDS);
    uint32_t dk_w = 0, skf_w = 0;                                           // the words of the current 32 steps: dark / skip the load
    const double *__restrict__ S = a.S + (int64_t)ls * SP * W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), w8 = wave & 7, half = wave >> 3;   // half < SD_HALVES
    const int c0 = strip * SD_OUT, cbase = c0 - 1 - SD_HL;
    const int pc = half * 64 + lane, c = c0 - 1 + pc;
    const bool cvalid = c >= 0 && c < W;
    const bool wave_live = c0 - 1 + half * 64 < W;                          // some column of this wave lies inside the image
    // per-position maxima max(layer 15, layer 30), two buffers by step parity, SD_M2_ROWS x SD_PC each: rows 0, 1 = the seam (rows 14, 15
    // of the step before), row 2 + r = position row r.  mb = this thread's column in row 0 of buffer 0 (byte offset)
    constexpr int M2ROW = SD_PC * 8, M2BUF = SD_M2_ROWS * M2ROW;
    const uint32_t mb = (uint32_t)(SD_RING_BYTES + w8 * M2ROW + pc * 8);
    auto m2at = [&](int buf, int row, int dc) -> double & { return *reinterpret_cast<double *>(sd_smem + (mb + (uint32_t)(buf * M2BUF + (row - w8) * M2ROW + dc * 8))); };
    // the twelve clipped corner columns (skimage _integ: c' = clip(c + off), c'' = clip(c' + width)) as ring byte offsets
    uint32_t ca[12], cb[12];
    {
        constexpr int off[6][2] = {{-7, 15}, {-2, 5}, {-4, 9}, {-14, 30}, {-5, 10}, {-9, 19}};
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const int x0 = clipi(c + off[q][0], 0, W - 1), x1 = clipi(x0 + off[q][1], 0, W - 1);
            ca[2 * q] = (uint32_t)((w8 * SD_BP + (x0 - cbase)) * 8);
            ca[2 * q + 1] = (uint32_t)((w8 * SD_BP + (x1 - cbase)) * 8);
        }
#pragma unroll
        for (int q = 0; q < 12; q++) cb[q] = ca[q] + SD_SPLIT * SD_PITCHB;
    }
    // staging: the SD_T x SD_BP new elements of a step in linear order over the threads (element e = tid + SD_THREADS j: a wave reads runs
    // of 512 contiguous bytes); a thread's (row, column) pairs are fixed, the image base moves: loads are "uniform base + lane offset".
    // The rows of step t are loaded three steps ahead into one of two register sets (HBM latency is longer than a step)
    const bool strip_inside = cbase >= 0 && cbase + SD_BP <= W;
    uint32_t goff[SD_NST], loff[SD_NST];                                   // byte offsets: image (from row 16 t + 16, column cbase) / ring (from slot 16 q)
    int srow[SD_NST], scol[SD_NST];
#pragma unroll
    for (int j = 0; j < SD_NST; j++) {
        const int e = tid + SD_THREADS * j;
        srow[j] = e / SD_BP; scol[j] = e - srow[j] * SD_BP;
        goff[j] = (uint32_t)((srow[j] * SP + scol[j]) * 8);
        loff[j] = (uint32_t)(srow[j] * SD_PITCHB + scol[j] * 8);
    }
    double stage[2][SD_NST];
    const int nt = H / SD_T + 1;                                           // the last step's last row lies outside the image
    // the march covers the strip's lit steps [first, last] only: it starts on the multiple of four at or below first - 1 (a dark step, or
    // step 0: nothing above it is read; the per-position maxima of "the step before" start as zeros, which is what dark steps hold) and
    // ends with step last + 1, whose zeros close the maxima of step last
    const int t_first = (int)dtab[16], t_last = (int)dtab[17];
    if (t_first >= nt) return;                                             // nothing but the corners: no candidates (uniform: before any barrier)
    const int tb = t_first >= 1 ? ((t_first - 1) & ~3) : 0, te = min(nt, t_last + 2);
    int frow = SD_T * tb;                                                  // first image row of the next load: 16 t + 16, t = tb - 1, tb, ..
    // (skip: only dark steps would read the block - its loads are pointed at the strip's first block instead, lines this workgroup has
    // in its L1 since the prologue: the same instructions on both paths keep the compiler's vmcnt bookkeeping exact, a branch around
    // the loads made every later wait a wait for ALL outstanding loads and cost more than the traffic it saved)
    auto fetch = [&](double(&st)[SD_NST], bool skip = false) {
        const bool whole = frow >= 0 && frow + SD_T <= H && strip_inside;
        const char *base = reinterpret_cast<const char *>(S + (int64_t)((skip && whole) ? 0 : frow) * SP + cbase);       // (wave-uniform)
        if (whole) {
#pragma unroll
            for (int j = 0; j < SD_NST; j++)
                if (SD_THREADS * (j + 1) <= SD_T * SD_BP || tid + SD_THREADS * j < SD_T * SD_BP) st[j] = *reinterpret_cast<const double *>(base + goff[j]);
        } else {
#pragma unroll
            for (int j = 0; j < SD_NST; j++) {
                const int gr = frow + srow[j], col = cbase + scol[j];
                if (srow[j] < SD_T && gr >= 0 && gr < H && col >= 0 && col < W) st[j] = *reinterpret_cast<const double *>(base + goff[j]);
            }
        }
        frow += SD_T;
    };
    // ring slot of row 16 t + 16 + srow = 16 ((t + 1) & 3) + srow; slots 0..7 are mirrored at 64..71
    auto put = [&](int quarter, const double(&st)[SD_NST]) {
#pragma unroll
        for (int j = 0; j < SD_NST; j++)
            if (SD_THREADS * (j + 1) <= SD_T * SD_BP || tid + SD_THREADS * j < SD_T * SD_BP) {
                double *d = reinterpret_cast<double *>(sd_smem + (loff[j] + (uint32_t)(quarter * SD_T * SD_PITCHB)));
                const double v = __dmul_rn(st[j], SD_SCALE);
                *d = v;
                if (quarter == 0 && srow[j] < SD_DUP) d[SD_RING * SD_BP] = v;
            }
    };
    double d0[SD_T / 8], d1[SD_T / 8], p0 = 0.0, p1 = 0.0;                 // this step's determinants; the last row of the step before
    uint32_t cand = 0, pcand = 0;                                          // bit k: position k of the step holds a determinant above the threshold
#pragma unroll
    for (int k = 0; k < SD_T / 8; k++) { d0[k] = 0.0; d1[k] = 0.0; }
    // 3 x 3 x 3 maxima out of buffer `buf`: rr2 = row in the buffer (2 + position row; 1 = the seam row), r = image row
    auto decide = [&](int buf, int rr2, int r, double v0, double v1) {
        if (pc < 1 || pc > SD_OUT || c >= W || r >= H) return;
        double mx = m2at(buf, rr2, 0);
#pragma unroll
        for (int dr = -1; dr <= 1; dr++)
#pragma unroll
            for (int dc = -1; dc <= 1; dc++) { const double u = m2at(buf, rr2 + dr, dc); mx = u > mx ? u : mx; }
        const uint32_t bits = ((v0 > thr && !(mx > v0)) ? 1u : 0u) | ((v1 > thr && !(mx > v1)) ? 2u : 0u);
        if (bits) rt_push_maxima(a, first + ls, r, c, bits, v0, v1);
    };
    // maxima of step pt (rows 0 .. SD_T - 2) and of the last row of the step before it; everything they need is in step pt's buffer
    auto maxima = [&](int pt, int buf) {
        if (w8 == 7) {
            if (pcand) decide(buf, 1, SD_T * pt - 1, p0, p1);
            p0 = d0[SD_T / 8 - 1]; p1 = d1[SD_T / 8 - 1]; pcand = cand >> (SD_T / 8 - 1);
        }
        if (cand) {
#pragma unroll
            for (int k = 0; k < SD_T / 8; k++) {
                const int rr = 8 * k + w8;
                if (((cand >> k) & 1u) && rr < SD_T - 1) decide(buf, 2 + rr, SD_T * pt + rr, d0[k], d1[k]);
            }
        }
    };
    // prologue: per-position maxima cleared (rows above the image count as zero), rows 0..31 of the image, loads of steps 1 and 2 in flight
    for (int i = tid; i < 2 * SD_M2_ROWS * SD_PC; i += SD_THREADS) reinterpret_cast<double *>(sd_smem + SD_RING_BYTES)[i] = 0.0;
    fetch(stage[1]);
    fetch(stage[0]);
    put(0, stage[1]);
    put(1, stage[0]);
    fetch(stage[1]);
    fetch(stage[0]);
    __syncthreads();
    auto step = [&](auto tag, int t) {
        constexpr int PH = decltype(tag)::value, WB = PH & 1;
        // rows of step t + 1 (loaded two steps ago) into slots that step t does not read; then the loads of step t + 3 - unless only
        // dark steps would read them (rt_darktab_kernel)
        const uint32_t tb = 1u << (t & 31);
        put((PH + 2) & 3, stage[(PH + 1) & 1]);
        fetch(stage[(PH + 1) & 1], (skf_w & tb) != 0);
        if (t >= 1) maxima(t - 1, WB ^ 1);
        const int rbase = SD_T * t;
        const bool fast = t >= 1 && rbase + SD_T - 1 + SD_HR <= H - 1;
        const bool dark = (dk_w & tb) != 0;                                 // every box of every position of this step lies beyond the maximum range
        if (!wave_live || dark) {
#pragma unroll
            for (int k = 0; k < SD_T / 8; k++) { d0[k] = 0.0; d1[k] = 0.0; }
        } else if (fast) {
            sd_tile_fast<PH>(ca, cb, thr_s, d0, d1);
        } else {
#pragma unroll
            for (int k = 0; k < SD_T / 8; k++) {
                const int r = rbase + 8 * k + w8;
                d0[k] = r < H ? sd_det_rows<15, 0>(ca, w8, r, H) : 0.0;
                d1[k] = r < H ? sd_det_rows<30, 1>(ca, w8, r, H) : 0.0;
            }
        }
        cand = 0;
#pragma unroll
        for (int k = 0; k < SD_T / 8; k++) {
            const int rr = 8 * k + w8, r = rbase + rr;
            double mx = sd_max(d0[k], d1[k]);
            if (mx > thr) {
                // (rare) the dxy term, hessian_det_pruned's second half.  A product that stays at or below the threshold can neither
                // pass nor exceed a passing neighbour, so it goes to the maxima buffer as it is
                if (d0[k] > thr) d0[k] = sd_dxy<15>(d0[k], r, c, H, W, cbase);
                if (d1[k] > thr) d1[k] = sd_dxy<30>(d1[k], r, c, H, W, cbase);
                if (!cvalid) { d0[k] = 0.0; d1[k] = 0.0; }                 // outside the image: nothing that could exceed a maximum
                mx = sd_max(d0[k], d1[k]);
                if (mx > thr) cand |= 1u << k;
            }
            if (k == SD_T / 8 - 1 && w8 >= 6) m2at(WB, rr - (SD_T - 2), 0) = m2at(WB ^ 1, 2 + rr, 0);   // the seam: the last two rows of the step before
            m2at(WB, 2 + rr, 0) = mx;
        }
        __syncthreads();
    };
    for (int t = tb; t < te; t += 4) {
        if ((t & 31) == 0 || t == tb) { dk_w = dtab[t >> 5]; skf_w = dtab[8 + (t >> 5)]; }
        step(SdTag<0>(), t);
        if (t + 1 < te) step(SdTag<1>(), t + 1);
        if (t + 2 < te) step(SdTag<2>(), t + 2);
        if (t + 3 < te) step(SdTag<3>(), t + 3);
    }
    maxima(te - 1, (te - 1) & 1);
}

#include "retrack_fused.inc"

size_t retrack_darktab_words(int W) { return (size_t)((W + SD_OUT - 1) / SD_OUT) * SD_DT_WORDS; }

hipError_t launch_retrack_darktab(hipStream_t st, const uint32_t *map, int W, int cols, uint32_t *darktab)
{
    const int ns = (W + SD_OUT - 1) / SD_OUT, nt = W / SD_T + 1;
    if (nt > 256) return hipErrorInvalidValue;                               // (the sampling map addresses 4095 range bins: W <= 4094, nt <= 256)
    hipLaunchKernelGGL(rt_darktab_kernel, dim3(ns, nt), dim3(256), 0, st, map, W, cols, darktab);
    hipLaunchKernelGGL(rt_darkskip_kernel, dim3(ns), dim3(256), 0, st, nt, darktab);
    return hipGetLastError();
}

size_t retrack_fused_boxtab_words(int W) { return 2 * (size_t)((W + SD_OUT - 1) / SD_OUT + 1) * (size_t)((W + SD_T - 1) / SD_T); }
size_t retrack_fused_halo_words(int W) { return (size_t)((W + SD_T - 1) / SD_T) * SD_T * FD_HALO; }

hipError_t launch_retrack_fused_tables(hipStream_t st, const uint32_t *map, int W, int cols, uint32_t *mapT, uint32_t *boxtab, uint32_t *darktab)
{
    const int nband = (W + SD_OUT - 1) / SD_OUT, nblk = (W + SD_T - 1) / SD_T;
    hipLaunchKernelGGL(rf_mapT_kernel, dim3((W + 31) / 32, (W + 31) / 32), dim3(256), 0, st, map, W, mapT);
    hipLaunchKernelGGL(rf_boxtab_kernel, dim3(nblk, nband + 1), dim3(64), 0, st, mapT, W, cols, nblk, boxtab);
    // the dark steps of a band = the dark steps of a strip of the transposed image: rt_darktab_kernel on the transposed map
    return launch_retrack_darktab(st, mapT, W, cols, darktab);
}

hipError_t retrack_det_init()
{
    if (hipError_t ef = hipFuncSetAttribute(reinterpret_cast<const void *>(rt_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, FD_LDS_BYTES); ef != hipSuccess) return ef;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(rt_det_strip_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SD_LDS_BYTES);
}

hipError_t launch_det(hipStream_t st, const RtArgs &a, int first, int P)
{
    if (a.size1 != 15 || a.size2 != 30) return hipErrorInvalidValue;      // the engine's fixed detector parameters (box sizes are compile-time)
    const int ns = (a.W + SD_OUT - 1) / SD_OUT;
    hipLaunchKernelGGL(rt_det_strip_kernel, dim3((unsigned)(((int64_t)P * ns + 7) / 8 * 8)), dim3(SD_THREADS), SD_LDS_BYTES, st, a, first, P, ns);
    return hipGetLastError();
}

hipError_t launch_retrack_fused(hipStream_t st, const RtArgs &a, int first, int P, int dbg)
{
    hipLaunchKernelGGL(rt_fused_kernel, dim3(P), dim3(FD_THREADS), FD_LDS_BYTES, st, a, first, dbg);
    return hipGetLastError();
}
