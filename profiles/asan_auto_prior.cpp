// Stand-alone sanitizer program for the host side of the in-step motion prior (profiles/asan_auto_prior.sh builds and runs it; no GPU
// is touched and nothing is loaded into Python): the argument checks and the size arithmetic of roam_fmt_auto_plan over valid, limit
// and refused configurations, and the host table makers the pass uploads - the forward warpPolar tables and the Hanning factors of both
// planes - written into buffers of exactly the size the pass allocates for them.
#include "../radarslampy_amd/csrc/roam_internal.h"
#include <math.h>
#include <stdlib.h>

void *roam_scratch(roam_ctx *, int, size_t) { return nullptr; }          // (api.hip's; the blocking entries are not called here)

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); fails++; } } while (0)

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
