// Stand-alone sanitizer program for the host side of the Fourier-Mellin passes (profiles/asan_auto_prior.sh builds and runs it; no GPU
// is touched and nothing is loaded into Python): the argument checks and the size arithmetic of roam_fmt_auto_plan over valid, limit
// and refused configurations; the bytes per pair of both halves, the chunk and the slab of the in-step pass and the bytes per pair of
// the blocking passes against the figures of the commit before the passes got one workspace; the carve of the three kinds of pass;
// and the host table makers the pass uploads - the forward warpPolar tables and the Hanning factors of both planes - written into
// buffers of exactly the size the pass allocates for them.
#include "../radarslampy_amd/csrc/fmt.h"
#include <math.h>
#include <stdlib.h>

void *roam_scratch(roam_ctx *, int, size_t) { return nullptr; }          // (api.hip's; the blocking entries are not called here)

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); fails++; } } while (0)

// Figures printed by commit 69a4381 (fft.hip still held the drivers, thirteen scratch slots), from a program that included that file.
// The in-step pass {rows, cols, clip, R, Rc, lanes}: bytes per pair of the rotation and translation half, their sum, chunk, slab bytes
static const struct { FmtAutoCfg cfg; size_t rot, trans, per_pair, chunk, slab; } AUTO_AT_69A4381[] = {
    {{400, 2025, 1012, 101, 101, 3, 0.0, 0.0}, 2585000u, 2939224u, 5524224u, 3u, 10782464u},              // the live shape of the tests
    {{400, 1012, 1012, 101, 50, 4096, 0.0, 0.0}, 2585000u, 640056u, 3225056u, 650u, 1733143808u},        // Oxford: downsample 10, cart 20
    {{400, 2048, 8, 4, 2048, 3, 0.0, 0.0}, 16680u, 1073741880u, 1073758560u, 1u, 1073834752u},           // the limits
    {{8, 2606, 2606, 1303, 1, 3, 0.0, 0.0}, 364070888u, 312u, 364071200u, 3u, 1092365568u},
};
// The blocking passes on the shapes of tests/fmt_register_cases.py {rows, cols, clip, R, Rc}: bytes per pair of roam_fmt_batch_run for
// (resident, host contiguous, host strided) x (log-polar output off, on), and of roam_fmt_register_run for (resident, host) x (turned-source
// output off, on)
static const struct { int rows, cols, clip, R, Rc; size_t rot[6], reg[4]; } BLOCKING_AT_69A4381[] = {
    {400, 2025, 1012, 101, 101, {2585000u, 2841136u, 9065000u, 9321136u, 5823400u, 6079536u}, {5524224u, 5687440u, 12004224u, 12167440u}},
    {400, 2025, 1012, 101, 405, {2585000u, 2841136u, 9065000u, 9321136u, 5823400u, 6079536u}, {44575456u, 47199856u, 51055456u, 53679856u}},
    {64, 128, 128, 64, 128, {937992u, 1040904u, 1003528u, 1106440u, 1003528u, 1106440u}, {5132352u, 5394496u, 5197888u, 5460032u}},
    {64, 128, 128, 64, 42, {937992u, 1040904u, 1003528u, 1106440u, 1003528u, 1106440u}, {1448096u, 1476320u, 1513632u, 1541856u}},
    {399, 497, 497, 71, 71, {1295152u, 1421816u, 2881576u, 3008240u, 2881576u, 3008240u}, {2617736u, 2698392u, 4204160u, 4284816u}},
};

// a carve over a real base: every part it gives is 256-byte aligned and inside the slab, no two overlap (sizes restated here from the
// shapes), what the pass does not have is null, and the null-slab carve counts the same bytes
static void check_carve(const FmtPass &s)
{
    const size_t total = fmt_carve(s, nullptr, nullptr);
    uint8_t *base = (uint8_t *)aligned_alloc(256, total ? total : 256);
    FmtWork w;
    EXPECT(fmt_carve(s, base, &w) == total);
    const size_t dw = (size_t)rint((double)s.R), dh = (size_t)rint((double)s.R * M_PI), S = 2 * (size_t)s.Rc, c = s.chunk, L = s.lanes, per = L ? L : c;
    const size_t Mt = (size_t)optimal_dft_size((int)S), nr = (size_t)optimal_dft_size((int)dh) * optimal_dft_size((int)dw), nt = Mt * Mt;
    const size_t nmn = nr > nt ? nr : nt, nblk = (size_t)(pc_peak_grid(nr).nblk > pc_peak_grid(nt).nblk ? pc_peak_grid(nr).nblk : pc_peak_grid(nt).nblk);
    const struct { const void *p; size_t bytes; } parts[] = {
        {w.idx, 4 * (L ? 12 * L : s.nin ? 0 : 2 * c)}, {w.in, 4 * 2 * c * s.nin}, {w.tab, 8 * (3 * dh + dw) + 4 * dw}, {w.win, 8 * 2 * S},
        {w.pc.f, 8 * 7 * nmn * c}, {w.pc.pv, 8 * nblk * c}, {w.pc.pi, 4 * nblk * c}, {w.pc.out, 8 * 3 * per},
        {w.small, 4 * 2 * c * s.rows * s.R}, {w.cart_r, 4 * 2 * c * 4 * (size_t)s.R * s.R}, {w.cart_t, 4 * 2 * c * S * S},
        {w.lp, s.lp ? 4 * 2 * c * dh * dw : 0}, {w.rot, s.rot ? 4 * c * S * S : 0}, {w.trans3, 8 * 3 * L}, {w.ang, 8 * L}, {w.M, s.Rc ? 8 * 6 * per : 0},
    };
    size_t sum = 0;
    for (auto &a : parts) {
        const uint8_t *p = (const uint8_t *)a.p;
        EXPECT((a.bytes == 0) == (p == nullptr));
        sum += (a.bytes + 255) & ~(size_t)255;
        if (!p) continue;
        EXPECT(((uintptr_t)p & 255) == 0 && p >= base && p + a.bytes <= base + total);
        for (auto &b : parts) {
            const uint8_t *q = (const uint8_t *)b.p;
            EXPECT(&a == &b || !q || p + a.bytes <= q || q + b.bytes <= p);
        }
    }
    EXPECT(sum == total);              // the parent's sum over its slots, each part rounded up to 256 bytes
    free(base);
}

int main()
{
    roam_ctx ctx;
    FmtAutoPlan plan;
    const FmtAutoCfg ok = {400, 2025, 1012, 101, 101, 3, 0.0, 0.0};
    EXPECT(roam_fmt_auto_plan(&ctx, ok, &plan) == ROAM_OK && plan.chunk == 3 && plan.sz == 317 && plan.slab_bytes > 0);
    printf("live shape: %zu bytes per pair, chunk %zu, slab %zu bytes, log base %.17g\n", plan.per_pair, plan.chunk, plan.slab_bytes, plan.log_base);
    FmtAutoCfg c = ok;
    c.lanes = 100000; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_OK && plan.chunk == ((size_t)2000 << 20) / plan.per_pair);
    setenv("ROAM_FMT_BATCH_CHUNK", "2", 1);
    EXPECT(roam_fmt_auto_plan(&ctx, ok, &plan) == ROAM_OK && plan.chunk == 2);
    unsetenv("ROAM_FMT_BATCH_CHUNK");
    c = ok; c.R = 4; c.clip = 8; c.Rc = 2048; c.cols = 2048; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_OK);        // the limits pass
    c = ok; c.R = 1303; c.clip = 2606; c.cols = 2606; c.Rc = 1; c.rows = 8; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_OK);
    c = ok; c.R = 3; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    c = ok; c.R = 1304; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    c = ok; c.Rc = 0; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    c = ok; c.Rc = 2049; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    c = ok; c.rows = 7; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    c = ok; c.lanes = 0; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    c = ok; c.min_rot = -1e-9; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    c = ok; c.min_trans = NAN; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    c = ok; c.min_trans = INFINITY; EXPECT(roam_fmt_auto_plan(&ctx, c, &plan) == ROAM_E_ARG);
    for (auto &a : AUTO_AT_69A4381) {
        EXPECT(fmt_rot_bytes_per_pair(a.cfg.rows, a.cfg.R, 0, false) == a.rot && fmt_trans_bytes_per_pair(a.cfg.Rc, 0, false) == a.trans);
        EXPECT(roam_fmt_auto_plan(&ctx, a.cfg, &plan) == ROAM_OK && plan.per_pair == a.per_pair && plan.chunk == a.chunk && plan.slab_bytes == a.slab);
        check_carve({a.cfg.rows, a.cfg.R, a.cfg.Rc, a.chunk, (size_t)a.cfg.lanes, 0, false, false});                 // the in-step pass
    }
    for (auto &b : BLOCKING_AT_69A4381) {
        const size_t nin[3] = {0, (size_t)b.rows * b.cols, (size_t)b.rows * b.clip};          // resident; whole rows; the first clip columns
        for (int m = 0; m < 3; m++)
            for (int lp = 0; lp < 2; lp++) {
                EXPECT(fmt_rot_bytes_per_pair(b.rows, b.R, nin[m], lp != 0) == b.rot[2 * m + lp]);
                check_carve({b.rows, b.R, 0, 4, 0, nin[m], lp != 0, false});                                     // rotation only
            }
        for (int host = 0; host < 2; host++)
            for (int rot = 0; rot < 2; rot++) {
                EXPECT(fmt_rot_bytes_per_pair(b.rows, b.R, 0, false) + fmt_trans_bytes_per_pair(b.Rc, nin[host], rot != 0) == b.reg[2 * host + rot]);
                check_carve({b.rows, b.R, b.Rc, 3, 0, nin[host], false, rot != 0});                              // rotation + translation
            }
    }
    // the tables of both planes at the live shape, the small test shape and the limits, in buffers of the pass's exact sizes
    const int shapes[][2] = {{101, 101}, {128, 128}, {4, 1}, {1303, 2048}};
    for (auto &s : shapes) {
        const int R = s[0], S = 2 * s[1], dw = (int)rint((double)R), dh = (int)rint((double)R * M_PI);
        double *cs = (double *)malloc(sizeof(double) * 2 * dh), *wr = (double *)malloc(sizeof(double) * dh), *wc = (double *)malloc(sizeof(double) * dw);
        float *br = (float *)malloc(sizeof(float) * dw);
        double *win = (double *)malloc(sizeof(double) * S);
        roam_warp_polar_tables(dw, dh, (double)(2 * R) / 2.0, true, br, cs);
        roam_hanning_factors(dh, wr); roam_hanning_factors(dw, wc); roam_hanning_factors(S, win);
        EXPECT(isfinite(cs[2 * dh - 1]) && isfinite(br[dw - 1]) && wr[0] == 0.0 && win[0] == 0.0 && fabs(win[S - 1]) < 1e-12);
        free(cs); free(wr); free(wc); free(br); free(win);
    }
    EXPECT(roam_normalize_angle(3.0 * M_PI) == roam_normalize_angle(M_PI) && roam_normalize_angle(0.25) == 0.25 - 0.0);
    EXPECT(roam_fmt_scale(plan.log_base, 0.0) == 1.0);
    printf(fails ? "%d checks FAILED\n" : "all checks passed (%d failed)\n", fails);
    return fails ? 1 : 0;
}
