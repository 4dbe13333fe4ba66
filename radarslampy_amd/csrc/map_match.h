// map_match.h - the host half of the map matching (map_match.hip): the smear table, the angle table and the checks of every argument
// that can be checked without a device.  Plain C++ with the host's libm and nothing of HIP, so that profiles/asan_map_match.cpp
// compiles it alone; internal.  The definition is include/roam_abi.h ("map matching"), the contract tests/map_match_model.py.
// Which unit owns what: this header owns the tables and the argument checks; map_match.hip owns the handle (roam_map_field), the
// kernels (mm_field_kernel, mm_match_kernel, mm_finish_kernel) and every entry; loop_map.hip owns the render the field is made from
// and is not called from here; the database's resident clouds are read through loop.h's roam_loop_db and nothing of it is written.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../include/roam_abi.h"

#define MM_FAIL(err, cap, ...)                              \
    do {                                                    \
        if (err) snprintf(err, cap, __VA_ARGS__);           \
        return false;                                       \
    } while (0)

// T[dv + r][du + r] = (uint8) floor(255 exp(-(du du + dv dv) / (2 sigma sigma)) + 0.5); false: radius or sigma refused, table null
static inline bool map_field_table(double sigma, int32_t radius, uint8_t *table)
{
    if (!table || radius < 0 || radius > ROAM_MATCH_MAX_RADIUS || !(std::isfinite(sigma) && sigma > 0.0)) return false;
    const int side = 2 * radius + 1;
    const double den = 2.0 * sigma * sigma;
    if (!(den > 0.0)) return false;              // a sigma whose square underflows: 0 / 0 at the centre
    for (int dv = -radius; dv <= radius; ++dv)
        for (int du = -radius; du <= radius; ++du)
            table[(dv + radius) * side + du + radius] = (uint8_t)floor(255.0 * exp(-(double)(du * du + dv * dv) / den) + 0.5);
    return true;
}

// what the field's creation refuses besides null pointers.  err may be null
static inline bool map_field_check(char *err, size_t cap, double ox, double oy, double res, int32_t W, int32_t H, int32_t min_hits, int32_t min_views,
                                   int32_t radius)
{
    if (!(std::isfinite(res) && res > 0.0)) MM_FAIL(err, cap, "map field: res finite and > 0, not %g", res);
    if (!(std::isfinite(ox) && std::isfinite(oy))) MM_FAIL(err, cap, "map field: the origin ox, oy finite, not %g, %g", ox, oy);
    if (W < 1 || H < 1) MM_FAIL(err, cap, "map field: W and H >= 1, not %d and %d", W, H);
    if ((int64_t)W * H > ROAM_MAP_MAX_CELLS)
        MM_FAIL(err, cap, "map field: W H = %lld cells, beyond ROAM_MAP_MAX_CELLS = %d", (long long)((int64_t)W * H), ROAM_MAP_MAX_CELLS);
    if (min_hits < 1 || min_views < 1) MM_FAIL(err, cap, "map field: min_hits and min_views >= 1, not %d and %d", min_hits, min_views);
    if (radius < 0 || radius > ROAM_MATCH_MAX_RADIUS) MM_FAIL(err, cap, "map field: radius in [0, %d], not %d", ROAM_MATCH_MAX_RADIUS, radius);
    return true;
}

// the window and the priors of a match
static inline bool map_match_check_window(char *err, size_t cap, int32_t n_query, const double *priors, int32_t n_theta, double step_rad, int32_t kx,
                                          int32_t ky, bool with_volume)
{
    if (n_query < 1) MM_FAIL(err, cap, "map match: n_query >= 1, not %d", n_query);
    if (!priors) MM_FAIL(err, cap, "map match: priors is null");
    if (n_theta < 1 || n_theta > ROAM_MATCH_MAX_ANGLES || n_theta % 2 == 0)
        MM_FAIL(err, cap, "map match: n_theta odd in [1, %d], not %d", ROAM_MATCH_MAX_ANGLES, n_theta);
    if (!(std::isfinite(step_rad) && step_rad >= 0.0)) MM_FAIL(err, cap, "map match: step_rad finite and >= 0, not %g", step_rad);
    if (kx < 0 || kx > ROAM_MATCH_MAX_SHIFT) MM_FAIL(err, cap, "map match: kx in [0, %d], not %d", ROAM_MATCH_MAX_SHIFT, kx);
    if (ky < 0 || ky > ROAM_MATCH_MAX_SHIFT) MM_FAIL(err, cap, "map match: ky in [0, %d], not %d", ROAM_MATCH_MAX_SHIFT, ky);
    for (int64_t q = 0; q < n_query; ++q) {
        const double *p = priors + 3 * q;
        const double reach = (double)((n_theta - 1) / 2) * step_rad;          // the outermost angles must stay finite too
        if (!(fabs(p[0]) <= ROAM_ICP_MAX_COORD && fabs(p[1]) <= ROAM_ICP_MAX_COORD && std::isfinite(p[2] - reach) && std::isfinite(p[2] + reach)))
            MM_FAIL(err, cap, "map match: priors of query %lld: a pose that is not finite or beyond %g m", (long long)q, ROAM_ICP_MAX_COORD);
    }
    if (with_volume) {
        const int64_t per = (int64_t)n_theta * (2 * ky + 1) * (2 * kx + 1);
        if ((int64_t)n_query * per > ROAM_MATCH_MAX_VOLUME)
            MM_FAIL(err, cap, "map match: scores_out of %lld entries, beyond ROAM_MATCH_MAX_VOLUME = %d", (long long)((int64_t)n_query * per),
                    ROAM_MATCH_MAX_VOLUME);
    }
    return true;
}

// the concatenated clouds of a match: offsets ascending from 0 with at most ROAM_ICP_MAX_POINTS rows each, every coordinate within the limit
static inline bool map_match_check_clouds(char *err, size_t cap, int32_t n_query, const double *xy, const int64_t *offsets)
{
    if (!offsets) MM_FAIL(err, cap, "map match: offsets is null");
    if (offsets[0] != 0) MM_FAIL(err, cap, "map match: offsets[0] = %lld, not 0", (long long)offsets[0]);
    for (int64_t q = 0; q < n_query; ++q) {
        const int64_t n = offsets[q + 1] - offsets[q];
        if (n < 0 || n > ROAM_ICP_MAX_POINTS)
            MM_FAIL(err, cap, "map match: offsets of query %lld: %lld points, not in [0, %d]", (long long)q, (long long)n, ROAM_ICP_MAX_POINTS);
    }
    const int64_t total = offsets[n_query];
    if (total && !xy) MM_FAIL(err, cap, "map match: xy is null");
    for (int64_t k = 0; k < 2 * total; ++k)
        if (!(fabs(xy[k]) <= ROAM_ICP_MAX_COORD))
            MM_FAIL(err, cap, "map match: xy of point %lld: a coordinate that is not finite or beyond %g m", (long long)(k / 2), ROAM_ICP_MAX_COORD);
    return true;
}

#define MM_THREADS 256                           // mm_match_kernel's workgroup
#define MM_ACC 8                                 // accumulators per thread
#define MM_CAND (MM_THREADS * MM_ACC)            // candidates per workgroup
#define MM_ROWS_ENV "ROAM_MATCH_ROWS"            // the tests' rows per workgroup (map_match_rows_env): how the window is cut, nothing else

// How a match cuts the 2 ky + 1 shift rows of its window into blocks, one workgroup per (query, angle, block): as many rows as the
// workgroup's MM_CAND candidates hold (most); fewer while that leaves compute units without a workgroup (about four per unit are
// wanted), but never so few that a wavefront of the workgroup has no candidate (least).  forced_rows > 0 takes the place of that
// choice and is clamped to [1, most] - the tests' way to every accumulator count on any device.  -> *rows (per workgroup), *n_blk
static inline void map_match_plan(int32_t cu_count, int32_t n_query, int32_t n_theta, int32_t kx, int32_t ky, int32_t forced_rows, int32_t *rows,
                                  int32_t *n_blk)
{
    const int rowlen = 2 * kx + 1, nb = 2 * ky + 1;
    const int most = nb < MM_CAND / rowlen ? nb : MM_CAND / rowlen, least = (MM_THREADS + rowlen - 1) / rowlen;
    const int64_t pairs = (int64_t)n_query * n_theta;
    const int64_t want_blk = (4 * (int64_t)(cu_count > 0 ? cu_count : 256) + pairs - 1) / pairs;
    int64_t r = forced_rows > 0 ? forced_rows : (nb + want_blk - 1) / want_blk;
    if (forced_rows <= 0 && r < least) r = least;
    *rows = (int32_t)(r > most ? most : r);
    *n_blk = (nb + *rows - 1) / *rows;
}

// the value of MM_ROWS_ENV (read per call): a positive integer forces the rows per workgroup, anything else is ignored
static inline int32_t map_match_rows_env()
{
    const char *e = getenv(MM_ROWS_ENV);
    const long v = e ? atol(e) : 0;
    return v > 0 && v <= 1024 ? (int32_t)v : 0;
}

// th_i = th0 + (double)(i - c) * step_rad, c = (n_theta - 1) / 2: two operations
static inline double map_match_theta(double th0, int32_t i, int32_t n_theta, double step_rad) { return th0 + (double)(i - (n_theta - 1) / 2) * step_rad; }

// cs (n_query, n_theta, 2) = (cos th_i, sin th_i).  The arguments have passed map_match_check_window
static inline void map_match_angle_table(int32_t n_query, const double *priors, int32_t n_theta, double step_rad, double *cs)
{
    for (int64_t q = 0; q < n_query; ++q)
        for (int32_t i = 0; i < n_theta; ++i) {
            const double th = map_match_theta(priors[3 * q + 2], i, n_theta, step_rad);
            cs[2 * (q * n_theta + i)] = cos(th);
            cs[2 * (q * n_theta + i) + 1] = sin(th);
        }
}
