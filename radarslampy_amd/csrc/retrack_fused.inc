// retrack_fused.inc - part of retrack_det.hip (included there, after the strip-march determinant kernel whose helpers it uses).
//
// K1 + K2 + K3 in ONE kernel: integral image, Hessian determinants and 3 x 3 x 3 maxima of a detection without the float64 integral
// image ever leaving the CU (getFeatures.py:39-51, skimage blob_doh: integral_image -> _hessian_matrix_det -> peak_local_max).
// Until round 4 rt_integral_kernel wrote the image (32.8 MB per detection) and rt_det_strip_kernel read it back 1.25 times: 65.6 of the
// 66.4 algorithmic MB of a detection, both kernels at a third of the HBM roofline and at half of the LDS / VALU ceilings.
//
// What makes the fusion possible is the DIRECTION of the march.  skimage's integral image is cumsum(axis 0) then cumsum(axis 1): the
// column sums are exact in float64 (every pixel is a multiple of 2^-41 below 1: any order, any grouping), the ROW sums are rounded and
// must be added strictly left to right.  rt_det_strip_kernel marches DOWN column strips, so a strip would need the rounded running
// sum of every row from the strip on its left - a serial dependence between workgroups.  Here one workgroup owns a BAND of 62 output
// rows and marches RIGHT in steps of 16 image columns: the rounded running sum of a row is a register of the lane that owns the row,
// carried from step to step for the whole band; what crosses bands is exact: the column totals of everything above (2 K doubles) and
// the 32 finished rows the next band's boxes overlap (read back 16 x 32 doubles per step; per detection 34 MB through L2 / HBM instead
// of 80 MB, and no second kernel).  One workgroup per DETECTION runs its 34 bands one after the other: no inter-workgroup
// synchronisation at all.
//
//   axes:   "march" = image column c (16 per step),  "lane" = image row r.  The LDS ring of rt_det_strip_kernel is kept as it is with the
//           two axes exchanged: ring slot (c & 63) holds column c as 96 consecutive doubles, rows rbase .. rbase + 95 of the band
//           (rbase = first output row - 15); lanes read consecutive rows: conflict-free ds_read_b64 as before.  Box corners keep
//           skimage's operand order ((S[r,c] + S[r2,c2]) - S[r,c2]) - S[r2,c] (fd_tile_fast: the B and C operands trade places
//           against sd_tile_fast).
//   waves:  0..7 "det waves" (512 threads: pixels, determinants, maxima), 8 the "chain wave" (row sums).
//   a step t has two halves, one barrier each:
//     alpha(t):  maxima of step t - 1;  PC(t + 2): the 62 x 16 float32 pixels of block t + 2 (a block = 16 columns) from the polar record
//                (the arithmetic of rt_integral_kernel / warp.hip; polar footprint staged in LDS), lane = row, two columns per wave, the
//                exact column sums as a DPP prefix over the lanes + the column's carry from the bands above -> CS tile;  the 32 halo
//                rows of block t + 2 (prefetched from the previous band's hand-off) -> ring;  hand-off of the last 32 rows of block
//                t + 1 -> global;  loads for block t + 3 issued (sampling-map words, polar box, halo, column carries)
//     beta(t):   chain wave: R(t + 2): carry[row] += CS[col][row] for the 16 columns in order (THE rounded sum), scaled by 2^-10 into the
//                ring slot nobody reads;  det waves: polar box of block t + 3 registers -> LDS; D(t): determinants of step t from ring
//                blocks t - 1, t, t + 1 (the code of rt_det_strip_kernel)
//   LDS: ring 55 296 + maxima 9 216 (single buffer: the halves separate its readers from its writers) + CS 8 192 + box 2 048 + table
//   1 024 = 75 776 B: two workgroups per CU.
#define FD_NEW0 32                          // ring row of the band's first new row (rows 0..31 come from the band above)
#define FD_HALO 32
#define FD_M2_BYTES (SD_M2_ROWS * 64 * 8)
#define FD_CS_OFF (SD_RING_BYTES + FD_M2_BYTES)
#define FD_CS_BYTES (SD_T * 64 * 8)
#define FD_BOX_OFF (FD_CS_OFF + FD_CS_BYTES)
#define FD_BOX 2048
#define FD_LUT_OFF (FD_BOX_OFF + FD_BOX)
#define FD_LDS_BYTES (FD_LUT_OFF + 1024)
#define FD_THREADS 576
#define FD_DARKWORD 0x00000fffu             // a sampling-map word beyond the maximum range (ix = 4095)
static_assert(SD_HALVES == 1 && SD_T == 16 && SD_BP == 96 && SD_OUT == 62, "the fused kernel shares the ring geometry of the 8-wave strip kernel");

// ---- geometry tables of the fused kernel, once per engine
// the sampling map transposed (lane = row reads consecutive words)
__global__ __launch_bounds__(256) void rf_mapT_kernel(const uint32_t *__restrict__ map, int W, uint32_t *__restrict__ mapT)
{
    __shared__ uint32_t tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) { const int r = by + j, c = bx + tx; tile[j][tx] = (r < W && c < W) ? map[(int64_t)r * W + c] : FD_DARKWORD; }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) { const int c = bx + j, r = by + tx; if (r < W && c < W) mapT[(int64_t)c * W + r] = tile[tx][j]; }
}
// polar footprint of the (band, block) patch: rows 62 k + 17 .. + 61 (k = blockIdx.y - 1), columns 16 b .. 16 b + 15; the format of rt_boxtab_kernel
__global__ __launch_bounds__(64) void rf_boxtab_kernel(const uint32_t *__restrict__ mapT, int W, int cols, int nblk, uint32_t *__restrict__ tab)
{
    const int lane = threadIdx.x, b = blockIdx.x, k = (int)blockIdx.y - 1;
    const int r = SD_OUT * k + 17 + lane;
    int mnx = 0x7fffffff, mxx = -1, mny = 0x7fffffff, mxy = -1;
    if (lane < SD_OUT && r >= 0 && r < W)
        for (int j = 0; j < SD_T; j++) {
            const int c = SD_T * b + j;
            if (c >= W) break;
            const uint32_t m = mapT[(int64_t)c * W + r];
            const int ix = m & 4095, iy = (m >> 12) & 1023;
            if (ix < cols) { mnx = min(mnx, ix); mxx = max(mxx, ix); mny = min(mny, iy); mxy = max(mxy, iy); }
        }
    for (int d = 32; d >= 1; d >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, d)); mxx = max(mxx, __shfl_xor(mxx, d));
        mny = min(mny, __shfl_xor(mny, d)); mxy = max(mxy, __shfl_xor(mxy, d));
    }
    if (lane == 0) {
        const int idx = (int)blockIdx.y * nblk + b;
        tab[2 * idx] = mxx < 0 ? 0xffff0000u : ((uint32_t)mnx | ((uint32_t)mxx << 16));
        tab[2 * idx + 1] = mxx < 0 ? 0u : ((uint32_t)mny | ((uint32_t)mxy << 16));
    }
}

// dxx * dyy of a thread's two positions (march positions w8 and 8 + w8 of the step) where no box COLUMN needs clipping: sd_tile_fast with
// the axes exchanged.  A box ((S[ra,ca] + S[rb,cb]) - S[ra,cb]) - S[rb,ca]: rows are the lane's clipped offsets ca[] / cb[] (pair 0: -s2,+w;
// pair 1: -(s3/2),+s3; pair 2: -s3+1,+2s3-1), columns the immediates.
template <int PH>
__device__ __forceinline__ void fd_tile_fast(const uint32_t (&ca)[12], const uint32_t (&cb)[12], double (&d0)[SD_T / 8], double (&d1)[SD_T / 8])
{
    double v[2][2][4];                                                     // [pair slot][position][corner]
    auto issue = [&](int i, double(&o)[2][4]) {
        const int L = (i >> 2) & 1, q = i & 3;                             // q: xx-mid, xx-side, yy-mid, yy-side (hessian_box 4..7)
        const int SIZE = L ? 30 : 15, s2 = (SIZE - 1) / 2, s3 = SIZE / 3;
        const int ma = q == 0 ? -s2 : (q == 1 ? -(s3 / 2) : -s3 + 1), mb = ma + (q == 0 ? SIZE : (q == 1 ? s3 : 2 * s3 - 1));
        const int ja = 6 * L + (q < 2 ? 4 : (q == 2 ? 0 : 2)), jb = ja + 1;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int M0 = SD_T * PH + 8 * k;
            o[k][0] = sd_ldr(ca, cb, M0 + ma, ja); o[k][1] = sd_ldr(ca, cb, M0 + mb, jb);
            o[k][2] = sd_ldr(ca, cb, M0 + mb, ja); o[k][3] = sd_ldr(ca, cb, M0 + ma, jb);
        }
    };
    issue(0, v[0]);
    double mid[2] = {0.0, 0.0}, dxx[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (i + 1 < 8) issue(i + 1, v[(i + 1) & 1]);
        const int L = (i >> 2) & 1, q = i & 3;
        const double(&x)[2][4] = v[i & 1];
        double t0 = __dadd_rn(x[0][0], x[0][1]), t1 = __dadd_rn(x[1][0], x[1][1]);
        t0 = __dsub_rn(t0, x[0][2]); t1 = __dsub_rn(t1, x[1][2]);
        double b0, b1;
        asm("v_add_f64 %0, %1, -%2 clamp" : "=v"(b0) : "v"(t0), "v"(x[0][3]));
        asm("v_add_f64 %0, %1, -%2 clamp" : "=v"(b1) : "v"(t1), "v"(x[1][3]));
        if (q == 0 || q == 2) { mid[0] = b0; mid[1] = b1; }
        else {
            const double w_i = L ? sd_wi<30>() : sd_wi<15>();
            double m0 = __dmul_rn(3.0, b0), m1 = __dmul_rn(3.0, b1);
            double e0 = __dsub_rn(mid[0], m0), e1 = __dsub_rn(mid[1], m1);
            e0 = __dmul_rn(-e0, w_i); e1 = __dmul_rn(-e1, w_i);
            if (q == 1) { dxx[0] = e0; dxx[1] = e1; }
            else if (L) { d1[0] = __dmul_rn(dxx[0], e0); d1[1] = __dmul_rn(dxx[1], e1); }
            else { d0[0] = __dmul_rn(dxx[0], e0); d0[1] = __dmul_rn(dxx[1], e1); }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the same product with the box COLUMNS clipped to the image (first / last steps of a band): c = image column of the position (wave-uniform)
template <int SIZE, int L>
__device__ __forceinline__ double fd_det_cols(const uint32_t (&ca)[12], int w8, int c, int W)
{
    constexpr int s2 = (SIZE - 1) / 2, s3 = SIZE / 3, w = SIZE, J = 6 * L;
    const double w_i = sd_wi<SIZE>();
    auto ld = [&](int col, int j) { return *reinterpret_cast<const double *>(sd_smem + (ca[j] + (uint32_t)(((col & (SD_RING - 1)) - w8) * SD_PITCHB))); };
    const int xa = clipi(c - s2, 0, W - 1), xb = clipi(xa + w, 0, W - 1), za = clipi(c - s3 / 2, 0, W - 1), zb = clipi(za + s3, 0, W - 1);
    double mid = sd_box(ld(xa, J + 4), ld(xb, J + 5), ld(xb, J + 4), ld(xa, J + 5));
    double side = sd_box(ld(za, J + 4), ld(zb, J + 5), ld(zb, J + 4), ld(za, J + 5));
    double dxx = __dsub_rn(mid, __dmul_rn(3.0, side));
    dxx = __dmul_rn(-dxx, w_i);
    const int ya = clipi(c - s3 + 1, 0, W - 1), yb = clipi(ya + 2 * s3 - 1, 0, W - 1);
    mid = sd_box(ld(ya, J + 0), ld(yb, J + 1), ld(yb, J + 0), ld(ya, J + 1));
    side = sd_box(ld(ya, J + 2), ld(yb, J + 3), ld(yb, J + 2), ld(ya, J + 3));
    double dyy = __dsub_rn(mid, __dmul_rn(3.0, side));
    dyy = __dmul_rn(-dyy, w_i);
    return __dmul_rn(dxx, dyy);
}

// the dxy term of a position whose dxx * dyy passes the threshold (rare): sd_dxy with the ring's axes exchanged
template <int SIZE>
__device__ __forceinline__ double fd_dxy(double det, int r, int c, int H, int W, int rbase)
{
    constexpr int s3 = SIZE / 3;
    const double w_i = sd_wi<SIZE>();
    const int r0 = clipi(r - s3, 0, H - 1), r1 = clipi(r0 + s3, 0, H - 1), r2 = clipi(r + 1, 0, H - 1), r3 = clipi(r2 + s3, 0, H - 1);
    const int c0 = clipi(c - s3, 0, W - 1), c1 = clipi(c0 + s3, 0, W - 1), c2 = clipi(c + 1, 0, W - 1), c3 = clipi(c2 + s3, 0, W - 1);
    auto at = [&](int rr, int cc) { return *reinterpret_cast<const double *>(sd_smem + (((cc & (SD_RING - 1)) * SD_BP + (rr - rbase)) * 8)); };
    const double tl = sd_box(at(r0, c0), at(r1, c1), at(r0, c1), at(r1, c0));
    const double br = sd_box(at(r2, c2), at(r3, c3), at(r2, c3), at(r3, c2));
    const double bl = sd_box(at(r0, c2), at(r1, c3), at(r0, c3), at(r1, c2));
    const double tr = sd_box(at(r2, c0), at(r3, c1), at(r2, c1), at(r3, c0));
    double dxy = __dsub_rn(__dsub_rn(__dadd_rn(bl, tr), tl), br);
    dxy = __dmul_rn(-dxy, w_i);
    return __dsub_rn(det, __dmul_rn(0.81, __dmul_rn(dxy, dxy)));
}

// one step of an exact inclusive prefix sum over the wave's lanes (float64 through two 32-bit DPP moves; lanes without a source add 0)
#define FD_SCAN_STEP(S, CTRL, RMASK)                                                                                        \
    {                                                                                                                       \
        const long long b_ = __double_as_longlong(S);                                                                       \
        const int lo_ = __builtin_amdgcn_update_dpp(0, (int)(b_ & 0xffffffffll), CTRL, RMASK, 0xf, false);                  \
        const int hi_ = __builtin_amdgcn_update_dpp(0, (int)(b_ >> 32), CTRL, RMASK, 0xf, false);                           \
        S = __dadd_rn(S, __longlong_as_double(((long long)hi_ << 32) | (long long)(uint32_t)lo_));                          \
    }
__device__ __forceinline__ double fd_wave_prefix(double s)
{
    FD_SCAN_STEP(s, 0x111, 0xf);        // row_shr:1
    FD_SCAN_STEP(s, 0x112, 0xf);        // row_shr:2
    FD_SCAN_STEP(s, 0x114, 0xf);        // row_shr:4
    FD_SCAN_STEP(s, 0x118, 0xf);        // row_shr:8
    FD_SCAN_STEP(s, 0x142, 0xa);        // row_bcast:15 -> rows 1 and 3
    FD_SCAN_STEP(s, 0x143, 0xc);        // row_bcast:31 -> rows 2 and 3
    return s;
}
// a load that never hits this CU's L1 (bytes the workgroup itself stored a band ago)
__device__ __forceinline__ double fd_load_l2(const double *p)
{
    return __longlong_as_double(__hip_atomic_load(reinterpret_cast<const long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

__global__ __launch_bounds__(FD_THREADS) void rt_fused_kernel(RtArgs a, int first, int dbg)
{
    const int ls = blockIdx.x, slot = first + ls;
    if (slot >= *a.rt_n || !rt_one_sweep(a, first)) return;
    const int W = a.W, H = a.W;
    const double thr = a.threshold;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), w8 = wave & 7;
    const bool chain = wave == 8;
    const int nblk = (W + SD_T - 1) / SD_T, nt = W / SD_T + 1, nband = (H + SD_OUT - 1) / SD_OUT;
    const uint8_t *p = a.pool + (int64_t)a.rt_scan[slot] * a.rec_bytes + a.payload_off;
    const int rows = a.rows, cols = a.cols, stride = a.stride;
    float *lut = reinterpret_cast<float *>(sd_smem + FD_LUT_OFF);
    uint8_t *bx = reinterpret_cast<uint8_t *>(sd_smem + FD_BOX_OFF);
    double *cs = reinterpret_cast<double *>(sd_smem + FD_CS_OFF);
    double *hbuf = a.fd_halo + (int64_t)ls * 2 * a.fd_halo_words;         // two hand-off buffers: band k reads [k & 1], writes [(k + 1) & 1]
    double *ccg = a.fd_cc + (int64_t)ls * 2048;                           // column totals of the bands above
    double *Sdbg = (dbg & 1) ? a.S + (int64_t)ls * a.SP * W : nullptr;
    // ablations (measurement only: results are wrong): 2 no taps, 4 no prefix, 8 no determinants, 16 no row chain, 32 no hand-off / halo,
    // 64 no polar box staging, 128 no maxima, 256 no sampling-map / carry loads
    const bool ab_taps = dbg & 2, ab_scan = dbg & 4, ab_det = dbg & 8, ab_chain = dbg & 16, ab_halo = dbg & 32, ab_box = dbg & 64, ab_max = dbg & 128, ab_ld = dbg & 256, ab_px = dbg & 512, ab_il = dbg & 1024;
    if (tid < 256) lut[tid] = rt_code_to_f32(tid);
    typedef const uint32_t __attribute__((address_space(4))) *FdConstPtr;
    // hand-off element of this thread: column e >> 5 of a block, halo row e & 31
    const int hcol = (tid >> 5) & 15, hrow = tid & 31;
    struct Box { int mnx, mxx, mny, mxy, bh, bp, nrg, ncb; bool staged; };
    auto geom = [&](uint32_t e0, uint32_t e1) {
        Box b;
        b.mnx = e0 & 0xffff; b.mxx = (e0 >> 16) == 0xffff ? -1 : (int)(e0 >> 16); b.mny = e1 & 0xffff; b.mxy = e1 >> 16;
        const int bw = b.mxx - b.mnx + 2;
        b.bh = b.mxy - b.mny + 2; b.bp = (bw + 3) & ~3;
        b.nrg = (b.bh + 3) >> 2; b.ncb = (b.bp + 63) >> 6;                 // pieces of 4 polar rows x 64 bytes, one load instruction each
        b.staged = b.mxx >= 0 && b.bp * b.bh <= FD_BOX && cols >= 4 && b.nrg * b.ncb <= 16;
        return b;
    };
    const int sub = lane >> 4, c4 = (lane & 15) * 4;

    for (int k = -1; k < nband; k++) {
        const int r0 = SD_OUT * k, rbase = r0 - 1 - SD_HL;
        const int r = r0 - 1 + lane;                                       // this lane's position row (det waves)
        const bool rvalid = r >= 0 && r < H;
        const int rn = rbase + FD_NEW0 + lane;                             // this lane's new row (pixel / chain lanes 0..61)
        const bool rn_ok = lane < SD_OUT && rn >= 0 && rn < H;
        const FdConstPtr dtab = (FdConstPtr)(uintptr_t)(a.fd_darktab + max(k, 0) * SD_DT_WORDS);
        const FdConstPtr btab = (FdConstPtr)(uintptr_t)(a.fd_boxtab + (int64_t)2 * (k + 1) * nblk);
        const double *hin = hbuf + (int64_t)(k & 1) * a.fd_halo_words;
        double *hout = hbuf + (int64_t)((k + 1) & 1) * a.fd_halo_words;
        // determinant steps of the band: its lit steps, one dark (or the first) step before them, the step after them (rt_det_strip_kernel)
        int tb = nt, te = 0;
        if (k >= 0) {
            const int t_first = (int)dtab[16], t_last = (int)dtab[17];
            if (t_first < nt) { tb = max(0, t_first - 1); te = min(nt, t_last + 2); }
        }
        uint32_t ca[12], cb[12];
        {
            constexpr int off[6][2] = {{-7, 15}, {-2, 5}, {-4, 9}, {-14, 30}, {-5, 10}, {-9, 19}};
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const int x0 = clipi(r + off[q][0], 0, H - 1), x1 = clipi(x0 + off[q][1], 0, H - 1);
                // (band -1 computes no determinants; keep its offsets inside the ring anyway)
                ca[2 * q] = (uint32_t)((w8 * SD_BP + clipi(x0 - rbase, 0, SD_BP - 1)) * 8);
                ca[2 * q + 1] = (uint32_t)((w8 * SD_BP + clipi(x1 - rbase, 0, SD_BP - 1)) * 8);
            }
#pragma unroll
            for (int q = 0; q < 12; q++) cb[q] = ca[q] + SD_SPLIT * SD_PITCHB;
        }
        constexpr int M2ROW = 64 * 8;
        const uint32_t mb = (uint32_t)(SD_RING_BYTES + w8 * M2ROW + lane * 8);
        auto m2at = [&](int row, int dl) -> double & { return *reinterpret_cast<double *>(sd_smem + (mb + (uint32_t)((row - w8) * M2ROW + dl * 8))); };
        for (int i = tid; i < SD_M2_ROWS * 64; i += FD_THREADS) reinterpret_cast<double *>(sd_smem + SD_RING_BYTES)[i] = 0.0;
        double d0[2] = {0.0, 0.0}, d1[2] = {0.0, 0.0}, p0 = 0.0, p1 = 0.0;
        uint32_t cand = 0, pcand = 0, dk_w = 0;
        double carry = 0.0;                                                // chain wave: THE running sum of row rn
        // in flight for the next block: sampling-map words, column carries, the halo element, two pieces of the polar box, its footprint
        uint32_t m[2] = {FD_DARKWORD, FD_DARKWORD}, raw[2] = {0, 0};
        double ccv[2] = {0.0, 0.0}, hreg = 0.0;
        uint32_t cur0 = 0xffff0000u, cur1 = 0, nxt0 = 0xffff0000u, nxt1 = 0;   // footprint of the block whose pixels come next / of the one after
        auto decide = [&](int rr2, int c, double v0, double v1) {
            if (lane < 1 || lane > SD_OUT || r >= H || c >= W) return;
            double mx = m2at(rr2, 0);
#pragma unroll
            for (int dm = -1; dm <= 1; dm++)
#pragma unroll
                for (int dl = -1; dl <= 1; dl++) { const double u = m2at(rr2 + dm, dl); mx = u > mx ? u : mx; }
            const uint32_t bits = ((v0 > thr && !(mx > v0)) ? 1u : 0u) | ((v1 > thr && !(mx > v1)) ? 2u : 0u);
            if (bits) rt_push_maxima(a, first + ls, r, c, bits, v0, v1);
        };
        auto maxima = [&](int pt) {
            if (w8 == 7) {
                if (pcand) decide(1, SD_T * pt - 1, p0, p1);
                p0 = d0[1]; p1 = d1[1]; pcand = cand >> 1;
            }
            if (cand) {
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const int pp = 8 * q + w8;
                    if (((cand >> q) & 1u) && pp < SD_T - 1) decide(2 + pp, SD_T * pt + pp, d0[q], d1[q]);
                }
            }
        };
        // loads for block b (everything its PC / put need), issued a step ahead
        auto issue_loads = [&](int b) {
            cur0 = nxt0; cur1 = nxt1;
            if (b + 1 < nblk) { nxt0 = btab[2 * (b + 1)]; nxt1 = btab[2 * (b + 1) + 1]; }
            const int c0 = SD_T * b + 2 * w8;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int c = c0 + j;
                m[j] = (rn_ok && c < W && !ab_ld) ? a.fd_mapT[(int64_t)c * W + rn] : FD_DARKWORD;
                ccv[j] = (k >= 0 && c < W && !ab_ld) ? fd_load_l2(ccg + c) : 0.0;
            }
            hreg = (k >= 0 && !ab_halo) ? fd_load_l2(hin + ((int64_t)(SD_T * b + hcol) * FD_HALO + hrow)) : 0.0;
            const Box g = geom(cur0, cur1);
            if (g.staged && !ab_box) {
                const int npiece = g.nrg * g.ncb;
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int q = w8 + 8 * i, kg = (q / g.ncb) * 4, cbo = (q % g.ncb) * 64, kk = kg + sub, cc = cbo + c4;
                    raw[i] = 0;
                    if (q < npiece && kk < g.bh && cc < g.bp) {
                        int pr = g.mny + kk - 1;
                        if (pr < 0) pr += rows; else if (pr >= rows) pr -= rows;
                        // bytes beyond the scan's last range bin read as zero: the load is moved back inside the row and shifted
                        const int x0 = g.mnx + cc, xl = min(x0, cols - 4), sh = 8 * (x0 - xl);
                        if (sh < 32) raw[i] = reinterpret_cast<const RtU32 *>(p + pr * stride + xl)->v >> sh;
                    }
                }
            }
        };
        auto store_box = [&]() {                                            // the polar box of the block loaded last, registers -> LDS
            const Box g = geom(cur0, cur1);
            if (g.staged && !ab_box) {
                const int npiece = g.nrg * g.ncb;
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int q = w8 + 8 * i, kg = (q / g.ncb) * 4, cbo = (q % g.ncb) * 64, kk = kg + sub, cc = cbo + c4;
                    if (q < npiece && kk < g.bh && cc < g.bp) *reinterpret_cast<uint32_t *>(bx + kk * g.bp + cc) = raw[i];
                }
            }
        };
        // pixels + exact column sums of block b -> CS tile; its footprint is cur (issue_loads(b) came last)
        auto pixels = [&](int b) {
            const Box g = geom(cur0, cur1);
            const int c0 = SD_T * b + 2 * w8;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const uint32_t mk = m[j];
                const int ix = mk & 4095, iy = (mk >> 12) & 1023;
                float v = 0.f;
                if (g.mxx < 0 || ab_taps) v = 0.f;
                else if (g.staged) {
                    if (ix < cols) {
                        const float wx1 = __fmul_rn((float)((mk >> 22) & 31), 1.f / 32.f), wx0 = __fsub_rn(1.f, wx1);
                        const float wy1 = __fmul_rn((float)(mk >> 27), 1.f / 32.f), wy0 = __fsub_rn(1.f, wy1);
                        const uint8_t *q = bx + (iy - g.mny) * g.bp + (ix - g.mnx);
                        const float s00 = lut[q[0]], s01 = lut[q[1]], s10 = lut[q[g.bp]], s11 = lut[q[g.bp + 1]];   // lut[0] = 0: bins past the scan
                        v = __fmul_rn(s00, __fmul_rn(wy0, wx0));
                        v = __fadd_rn(v, __fmul_rn(s01, __fmul_rn(wy0, wx1)));
                        v = __fadd_rn(v, __fmul_rn(s10, __fmul_rn(wy1, wx0)));
                        v = __fadd_rn(v, __fmul_rn(s11, __fmul_rn(wy1, wx1)));
                    }
                } else v = rt_pixel(mk, p, rows, cols, stride, lut);
                const double s = ab_scan ? (double)v : fd_wave_prefix((double)v);                // exact: sum of this column's pixels in rows <= rn of the band
                const double tot = __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(__double_as_longlong(s) >> 32), 63) << 32) |
                                                        (long long)(uint32_t)__builtin_amdgcn_readlane((int)(__double_as_longlong(s) & 0xffffffffll), 63));
                cs[(2 * w8 + j) * 64 + lane] = __dadd_rn(ccv[j], s);
                if (lane == 0 && c0 + j < W) ccg[c0 + j] = __dadd_rn(ccv[j], tot);
            }
        };
        // block b: the halo rows (from the band above) into the ring, scaled
        auto put_halo = [&](int b) {
            const int sl = (SD_T * b + hcol) & (SD_RING - 1);
            double *d = reinterpret_cast<double *>(sd_smem + (sl * SD_PITCHB + hrow * 8));
            const double v = __dmul_rn(hreg, SD_SCALE);
            *d = v;
            if (sl < SD_DUP) d[SD_RING * SD_BP] = v;
        };
        // block b (finished): its last 32 rows to the band below
        auto hand_off = [&](int b) {
            const int sl = (SD_T * b + hcol) & (SD_RING - 1);
            const double v = *reinterpret_cast<const double *>(sd_smem + (sl * SD_PITCHB + (SD_OUT + hrow) * 8));
            hout[(int64_t)(SD_T * b + hcol) * FD_HALO + hrow] = __dmul_rn(v, SD_UNSCALE);
        };
        // chain wave: THE row sums of block b, in place of nothing: CS -> ring
        auto row_chain = [&](int b) {
            double x[SD_T];
#pragma unroll
            for (int j = 0; j < SD_T; j++) x[j] = cs[j * 64 + lane];
#pragma unroll
            for (int j = 0; j < SD_T; j++) {
                carry = __dadd_rn(carry, x[j]);
                const int c = SD_T * b + j, sl = c & (SD_RING - 1);
                double *d = reinterpret_cast<double *>(sd_smem + (sl * SD_PITCHB + (FD_NEW0 + lane) * 8));
                const double v = __dmul_rn(carry, SD_SCALE);
                *d = v;
                if (sl < SD_DUP) d[SD_RING * SD_BP] = v;
                if (Sdbg && rn_ok && c < W) Sdbg[(int64_t)rn * a.SP + c] = carry;
            }
        };
        // D(t): determinants of step t (rt_det_strip_kernel's step without its staging)
        auto det_step = [&](int t) {
            const int cbase_ = SD_T * t;
            const bool fast = t >= 1 && cbase_ + SD_T - 1 + SD_HR <= W - 1;
            const bool dark = (dk_w >> (t & 31)) & 1u;
            if (dark) {
#pragma unroll
                for (int q = 0; q < 2; q++) { d0[q] = 0.0; d1[q] = 0.0; }
            } else if (fast) {
                switch (t & 3) {
                case 0: fd_tile_fast<0>(ca, cb, d0, d1); break;
                case 1: fd_tile_fast<1>(ca, cb, d0, d1); break;
                case 2: fd_tile_fast<2>(ca, cb, d0, d1); break;
                default: fd_tile_fast<3>(ca, cb, d0, d1); break;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const int c = cbase_ + 8 * q + w8;
                    d0[q] = c < W ? fd_det_cols<15, 0>(ca, w8, c, W) : 0.0;
                    d1[q] = c < W ? fd_det_cols<30, 1>(ca, w8, c, W) : 0.0;
                }
            }
            cand = 0;
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int pp = 8 * q + w8, c = cbase_ + pp;
                double mx = sd_max(d0[q], d1[q]);
                if (mx > thr) {
                    if (d0[q] > thr) d0[q] = fd_dxy<15>(d0[q], r, c, H, W, rbase);
                    if (d1[q] > thr) d1[q] = fd_dxy<30>(d1[q], r, c, H, W, rbase);
                    if (!rvalid) { d0[q] = 0.0; d1[q] = 0.0; }
                    mx = sd_max(d0[q], d1[q]);
                    if (mx > thr) cand |= 1u << q;
                }
                if (q == 1 && w8 >= 6) m2at(pp - (SD_T - 2), 0) = m2at(2 + pp, 0);       // the seam: the last two positions of the step before
                m2at(2 + pp, 0) = mx;
            }
        };

        if (!chain) {
            nxt0 = btab[0]; nxt1 = btab[1];
        }
        __syncthreads();                                                   // M2 cleared, table in place, the previous band's LDS reads done
        for (int t = -3; t <= nt; t++) {                      // (nt >= nblk: the maxima of the last determinant step close at t = nt)
            // ---------------------------------------------------------------------------------------------- alpha(t)
            if (!chain) {
                if (t >= 1 && t - 1 >= tb && t - 1 < te && !ab_max) maxima(t - 1);
                if (t + 2 >= 0 && t + 2 < nblk) { if (!ab_px) pixels(t + 2); if (!ab_halo) put_halo(t + 2); }
                if (t + 1 >= 0 && t + 1 < nblk && !ab_halo) hand_off(t + 1);
                if (t + 3 >= 0 && t + 3 < nblk && !ab_il) issue_loads(t + 3);
            }
            __syncthreads();
            // ---------------------------------------------------------------------------------------------- beta(t)
            if (chain) {
                if (t + 2 >= 0 && t + 2 < nblk && !ab_chain) row_chain(t + 2);
            } else {
                if (t + 3 >= 0 && t + 3 < nblk) store_box();
                if (t >= tb && t < te && !ab_det) {
                    if ((t & 31) == 0 || t == tb) dk_w = dtab[t >> 5];
                    det_step(t);
                }
            }
            __syncthreads();
        }
        // the band's stores (hand-off rows, column carries) are what the next band loads
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
    }
}
