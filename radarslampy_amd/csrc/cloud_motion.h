// cloud_motion.h - the host half of the peak clouds' motion compensation: the checks of a velocity list and the per-row table that
// cloud_gather_motion_kernel (loop_cloud.hip) multiplies with.  Plain C++ with the host's libm and nothing of HIP, so that
// profiles/asan_cloud_motion.cpp compiles it alone; internal.  The definition is tests/loop_cloud_motion_model.py.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#define CM_FAIL(err, cap, ...)                              \
    do {                                                    \
        if (err) snprintf(err, cap, __VA_ARGS__);           \
        return false;                                       \
    } while (0)

// scan i of a velocity list has none: NaN in its vx slot
static inline bool cloud_motion_none(const double *velocities, int64_t i) { return std::isnan(velocities[3 * i]); }

// what an add with velocities refuses, the text naming the argument: period not finite or <= 0, a component that is not finite
// (other than the marker), a scan that could leave max_coord: |v| period / 2, the furthest a point is shifted, plus the largest range
// cols res.  err may be null
static inline bool cloud_motion_check(char *err, size_t cap, int64_t n, const double *velocities, double period, int cols, double res,
                                      double max_coord)
{
    if (!(std::isfinite(period) && period > 0.0)) CM_FAIL(err, cap, "loop db: period finite and > 0, not %g", period);
    for (int64_t i = 0; i < n; ++i) {
        const double *v = velocities + 3 * i;
        if (cloud_motion_none(velocities, i)) continue;
        if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2])))
            CM_FAIL(err, cap, "loop db: velocities of scan %lld: (%g, %g, %g) is not finite", (long long)i, v[0], v[1], v[2]);
        const double reach = std::hypot(v[0], v[1]) * period / 2.0 + (double)cols * res;
        if (!(reach <= max_coord))
            CM_FAIL(err, cap, "loop db: velocities of scan %lld: (%g, %g) m/s over %g s moves a point at %g m beyond %g m", (long long)i, v[0],
                    v[1], period, (double)cols * res, max_coord);
    }
    return true;
}

// out (n, rows, 4): C S DX DY of every row of every scan, every operation rounded once; all NaN for a scan without a velocity.
// The arguments have passed cloud_motion_check
static inline void cloud_motion_fill(int rows, double period, int64_t n, const double *velocities, double *out)
{
    for (int64_t i = 0; i < n; ++i) {
        const double *v = velocities + 3 * i;
        double *o = out + 4 * i * rows;
        for (int t = 0; t < rows; ++t, o += 4) {
            if (cloud_motion_none(velocities, i)) {
                o[0] = o[1] = o[2] = o[3] = NAN;
                continue;
            }
            const double tau = period * ((double)(2 * t - rows) / (double)(2 * rows));
            const double a = v[2] * tau;
            o[0] = cos(a);
            o[1] = sin(a);
            o[2] = v[0] * tau;
            o[3] = v[1] * tau;
        }
    }
}
