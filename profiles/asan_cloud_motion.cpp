// Stand-alone sanitizer program for the host half of the peak clouds' motion compensation: the velocity checks and the motion table
// of csrc/cloud_motion.h, compiled alone as plain C++ with -fsanitize=address,undefined (profiles/asan_cloud_motion.sh).  Every
// refusal the ABI lists, the marker, the row times at the ends and the middle of a scan, the table's symmetry, and the table written
// into buffers of exactly n x rows x 4 doubles so that a write past the end is a report.  Exit code 0: no report, every check passed.
#include "../radarslampy_amd/csrc/cloud_motion.h"
#include <cstring>
#include <vector>

static int bad = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); bad++; } \
    } while (0)

int main()
{
    char err[64];                                      // shorter than the longest text: snprintf must cut it
    const double max_coord = 1e6, res = 0.0432;
    const double ok[6] = {15.0, 3.0, 0.5, NAN, INFINITY, -INFINITY};              // a velocity, then the marker with anything behind it
    CHECK(cloud_motion_check(err, sizeof(err), 2, ok, 0.25, 3768, res, max_coord));
    CHECK(cloud_motion_check(nullptr, 0, 2, ok, 0.25, 3768, res, max_coord));
    CHECK(cloud_motion_check(err, sizeof(err), 0, nullptr, 0.25, 3768, res, max_coord));      // no scan: nothing is read
    for (double period : {0.0, -0.25, (double)NAN, (double)INFINITY}) {
        err[0] = 0;
        CHECK(!cloud_motion_check(err, sizeof(err), 2, ok, period, 3768, res, max_coord) && strstr(err, "period"));
        CHECK(!cloud_motion_check(nullptr, 0, 2, ok, period, 3768, res, max_coord));
    }
    const double not_finite[][3] = {{1.0, NAN, 0.0}, {INFINITY, 0.0, 0.0}, {0.0, 0.0, -INFINITY}, {1.0, 2.0, NAN}};
    for (const auto &v : not_finite) {
        double two[6] = {1.0, 2.0, 3.0, v[0], v[1], v[2]};
        err[0] = 0;
        CHECK(!cloud_motion_check(err, sizeof(err), 2, two, 0.25, 3768, res, max_coord) && strstr(err, "velocities of scan 1"));
        CHECK(strlen(err) < sizeof(err));
    }
    const double edge = (max_coord - 3768 * res) * 8.0;                            // |v| period / 2 + the largest range = max_coord
    const double fits[3] = {edge * (1.0 - 1e-12), 0.0, 100.0}, far[3] = {edge * (1.0 + 1e-9), 0.0, 0.0}, diag[3] = {6e6, -6e6, 0.0};
    CHECK(cloud_motion_check(err, sizeof(err), 1, fits, 0.25, 3768, res, max_coord));
    CHECK(!cloud_motion_check(err, sizeof(err), 1, far, 0.25, 3768, res, max_coord) && strstr(err, "velocities"));
    CHECK(!cloud_motion_check(err, sizeof(err), 1, diag, 0.25, 3768, res, max_coord));
    CHECK(cloud_motion_check(err, sizeof(err), 1, far, 0.125, 3768, res, max_coord));
    const double huge[3] = {1e308, 1e308, 0.0};                                    // hypot overflows: refused against a finite limit
    CHECK(!cloud_motion_check(err, sizeof(err), 1, huge, 0.25, 0, 0.0, max_coord));
    CHECK(cloud_motion_check(err, sizeof(err), 1, huge, 0.25, 0, 0.0, INFINITY)); // the table function's own call: no limit

    for (int rows : {1, 2, 64, 399, 400, 1020, 65536}) {
        const double v[9] = {15.0, 3.0, 0.5, NAN, 7.0, 7.0, -30.0, 10.0, -1.5};
        std::vector<double> out((size_t)3 * rows * 4);                            // exactly the table: a write past it is a report
        cloud_motion_fill(rows, 0.25, 3, v, out.data());
        const double *a = out.data(), *none = a + (size_t)4 * rows, *c = none + (size_t)4 * rows;
        for (int t = 0; t < rows; ++t)
            for (int k = 0; k < 4; ++k) CHECK(std::isnan(none[4 * t + k]) && std::isfinite(a[4 * t + k]) && std::isfinite(c[4 * t + k]));
        CHECK(a[2] == 15.0 * -0.125 && a[3] == 3.0 * -0.125 && a[0] == cos(0.5 * -0.125) && a[1] == sin(0.5 * -0.125));      // row 0: -period / 2
        if (rows % 2 == 0) {
            const double *mid = a + (size_t)4 * (rows / 2);
            CHECK(mid[0] == 1.0 && mid[1] == 0.0 && mid[2] == 0.0 && mid[3] == 0.0);
            for (int t = 1; t < rows; ++t) {                                       // t <-> rows - t
                const double *p = c + (size_t)4 * t, *q = c + (size_t)4 * (rows - t);
                CHECK(p[0] == q[0] && p[1] == -q[1] && p[2] == -q[2] && p[3] == -q[3]);
            }
        } else {
            for (int t = 0; t < rows; ++t) CHECK(a[4 * t + 2] != 0.0);            // no row at mid-scan
        }
    }
    printf("%d checks failed\n", bad);
    return bad ? 1 : 0;
}
