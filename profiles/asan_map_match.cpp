// Stand-alone sanitizer program for the host half of the map matching: the smear table, the angle table and the argument checks of
// csrc/map_match.h, compiled alone as plain C++ with -fsanitize=address,undefined (profiles/asan_map_match.sh).  Every refusal the ABI
// lists, the tables written into buffers of exactly their size so that a write past the end is a report, the clouds read to exactly
// their last coordinate, and an error buffer shorter than the longest text.  Exit code 0: no report, every check passed.
#include "../radarslampy_amd/csrc/map_match.h"
#include <cstring>
#include <vector>

static int bad = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); bad++; } \
    } while (0)

int main()
{
    char err[48];                                      // shorter than the longest text: snprintf must cut it
    // ---- the smear table
    for (int r = 0; r <= ROAM_MATCH_MAX_RADIUS; ++r)
        for (double sigma : {0.05, 0.5, 1.0, 3.0, 1e300}) {
            const int side = 2 * r + 1;
            std::vector<uint8_t> t((size_t)side * side, 7);                       // exactly the table
            CHECK(map_field_table(sigma, r, t.data()));
            CHECK(t[(size_t)r * side + r] == 255);
            for (int a = 0; a < side; ++a)
                for (int b = 0; b < side; ++b) {
                    CHECK(t[a * side + b] == t[b * side + a] && t[a * side + b] == t[(side - 1 - a) * side + b]);
                    if (a < r) CHECK(t[a * side + b] <= t[(a + 1) * side + b]);  // falling off from the centre
                }
        }
    uint8_t one = 0;
    CHECK(!map_field_table(1e-200, 0, &one) && one == 0);                         // 2 sigma sigma underflows to 0: the centre would be 0 / 0
    CHECK(map_field_table(1e-150, 0, &one) && one == 255);
    for (double sigma : {0.0, -1.0, (double)NAN, (double)INFINITY}) CHECK(!map_field_table(sigma, 2, &one));
    CHECK(!map_field_table(1.0, -1, &one) && !map_field_table(1.0, ROAM_MATCH_MAX_RADIUS + 1, &one) && !map_field_table(1.0, 2, nullptr));
    // ---- the field's arguments
    CHECK(map_field_check(err, sizeof(err), -1.5, 2.5, 0.25, 8192, 8192, 1, 1, 8));
    CHECK(map_field_check(nullptr, 0, 0.0, 0.0, 1e-300, 1, 1, 2147483647, 2147483647, 0));
    struct { double ox, oy, res; int W, H, mh, mv, r; const char *text; } refused[] = {
        {0, 0, 0.0, 4, 4, 1, 1, 2, "res"}, {0, 0, -1.0, 4, 4, 1, 1, 2, "res"}, {0, 0, NAN, 4, 4, 1, 1, 2, "res"}, {0, 0, INFINITY, 4, 4, 1, 1, 2, "res"},
        {NAN, 0, 1.0, 4, 4, 1, 1, 2, "origin"}, {0, -INFINITY, 1.0, 4, 4, 1, 1, 2, "origin"}, {0, 0, 1.0, 0, 4, 1, 1, 2, "W and H"},
        {0, 0, 1.0, 4, -4, 1, 1, 2, "W and H"}, {0, 0, 1.0, 8193, 8192, 1, 1, 2, "W H"}, {0, 0, 1.0, 2147483647, 2147483647, 1, 1, 2, "W H"},
        {0, 0, 1.0, 4, 4, 0, 1, 2, "min_hits"}, {0, 0, 1.0, 4, 4, 1, 0, 2, "min_hits"}, {0, 0, 1.0, 4, 4, 1, 1, -1, "radius"}, {0, 0, 1.0, 4, 4, 1, 1, 9, "radius"}};
    for (const auto &c : refused) {
        err[0] = 0;
        CHECK(!map_field_check(err, sizeof(err), c.ox, c.oy, c.res, c.W, c.H, c.mh, c.mv, c.r) && strstr(err, c.text));
        CHECK(strlen(err) < sizeof(err));
        CHECK(!map_field_check(nullptr, 0, c.ox, c.oy, c.res, c.W, c.H, c.mh, c.mv, c.r));
    }
    // ---- the window and the priors
    const double pri[6] = {1.0, -2.0, 0.3, -1e6, 1e6, -3.0};
    CHECK(map_match_check_window(err, sizeof(err), 2, pri, 25, 0.01, 12, 12, true));
    CHECK(map_match_check_window(err, sizeof(err), 2, pri, ROAM_MATCH_MAX_ANGLES, 0.0, ROAM_MATCH_MAX_SHIFT, ROAM_MATCH_MAX_SHIFT, false));
    CHECK(!map_match_check_window(err, sizeof(err), 2, pri, ROAM_MATCH_MAX_ANGLES, 0.0, ROAM_MATCH_MAX_SHIFT, ROAM_MATCH_MAX_SHIFT, true) && strstr(err, "scores_out"));
    CHECK(map_match_check_window(err, sizeof(err), 1, pri, 1023, 0.0, 128, 127, true));                  // 1023 x 255 x 257 = 67 042 305 <= 2^26
    CHECK(!map_match_check_window(err, sizeof(err), 0, pri, 3, 0.01, 1, 1, false) && strstr(err, "n_query"));
    CHECK(!map_match_check_window(err, sizeof(err), 2, nullptr, 3, 0.01, 1, 1, false) && strstr(err, "priors"));
    for (int n_theta : {0, -1, 2, 1024, 1027}) CHECK(!map_match_check_window(err, sizeof(err), 2, pri, n_theta, 0.01, 1, 1, false) && strstr(err, "n_theta"));
    for (double step : {-0.01, (double)NAN, (double)INFINITY}) CHECK(!map_match_check_window(err, sizeof(err), 2, pri, 3, step, 1, 1, false) && strstr(err, "step_rad"));
    for (int k : {-1, ROAM_MATCH_MAX_SHIFT + 1}) {
        CHECK(!map_match_check_window(err, sizeof(err), 2, pri, 3, 0.01, k, 1, false) && strstr(err, "kx"));
        CHECK(!map_match_check_window(err, sizeof(err), 2, pri, 3, 0.01, 1, k, false) && strstr(err, "ky"));
    }
    const double bad_pri[][3] = {{NAN, 0, 0}, {0, INFINITY, 0}, {1.0000001e6, 0, 0}, {0, -1.0000001e6, 0}, {0, 0, NAN}, {0, 0, -INFINITY}, {0, 0, 1.7e308}};
    for (const auto &b : bad_pri) {
        const double two[6] = {1.0, 2.0, 3.0, b[0], b[1], b[2]};
        err[0] = 0;
        CHECK(!map_match_check_window(err, sizeof(err), 2, two, 1025, 1e305, 1, 1, false) && strstr(err, "priors of query 1"));
        CHECK(!map_match_check_window(nullptr, 0, 2, two, 1025, 1e305, 1, 1, false));
    }
    // ---- the clouds: xy holds exactly the points the offsets announce
    {
        const int64_t off[4] = {0, 3, 3, 8195};
        std::vector<double> xy((size_t)2 * 8195, 0.5);
        xy.front() = -1e6;
        xy.back() = 1e6;
        CHECK(map_match_check_clouds(err, sizeof(err), 3, xy.data(), off));
        CHECK(map_match_check_clouds(nullptr, 0, 2, xy.data(), off));
        xy.back() = 1.0000001e6;
        CHECK(!map_match_check_clouds(err, sizeof(err), 3, xy.data(), off) && strstr(err, "xy of point 8194"));
        xy.back() = NAN;
        CHECK(!map_match_check_clouds(err, sizeof(err), 3, xy.data(), off) && strstr(err, "xy of point 8194"));
        CHECK(map_match_check_clouds(err, sizeof(err), 2, xy.data(), off));      // the first two clouds end before it
        const int64_t none[2] = {0, 0}, from1[2] = {1, 2}, back[3] = {0, 5, 4}, many[2] = {0, 8193};
        CHECK(map_match_check_clouds(err, sizeof(err), 1, nullptr, none));       // no point: xy is not read
        CHECK(!map_match_check_clouds(err, sizeof(err), 1, xy.data(), from1) && strstr(err, "offsets[0]"));
        CHECK(!map_match_check_clouds(err, sizeof(err), 2, xy.data(), back) && strstr(err, "offsets of query 1"));
        CHECK(!map_match_check_clouds(err, sizeof(err), 1, xy.data(), many) && strstr(err, "offsets of query 0"));
        CHECK(!map_match_check_clouds(err, sizeof(err), 1, nullptr, many + 0) && strlen(err) < sizeof(err));
        CHECK(!map_match_check_clouds(err, sizeof(err), 1, xy.data(), nullptr) && strstr(err, "offsets"));
        const int64_t some[2] = {0, 4};
        CHECK(!map_match_check_clouds(err, sizeof(err), 1, nullptr, some) && strstr(err, "xy is null"));
    }
    // ---- the angle table, into exactly n_query x n_theta x 2 doubles
    for (int n_theta : {1, 3, 25, ROAM_MATCH_MAX_ANGLES}) {
        std::vector<double> cs((size_t)2 * n_theta * 2);
        map_match_angle_table(2, pri, n_theta, 0.01, cs.data());
        const int c = (n_theta - 1) / 2;
        CHECK(cs[2 * c] == cos(0.3) && cs[2 * c + 1] == sin(0.3));               // the middle angle is the prior's own
        CHECK(cs[2 * (n_theta + c)] == cos(-3.0) && cs[2 * (n_theta + c) + 1] == sin(-3.0));
        CHECK(cs[0] == cos(0.3 + (double)(-c) * 0.01) && cs[2 * (2 * n_theta - 1)] == cos(-3.0 + (double)c * 0.01));
        for (size_t k = 0; k < cs.size(); ++k) CHECK(std::isfinite(cs[k]) && fabs(cs[k]) <= 1.0);
        CHECK(map_match_theta(0.3, c, n_theta, 0.01) == 0.3 && map_match_theta(0.3, 0, n_theta, 0.01) == 0.3 + (double)(-c) * 0.01);
    }
    // ---- the cut of a window into workgroups: never more candidates than a workgroup holds, every row in exactly one block
    for (int cu : {0, 1, 256, 304, 100000})
        for (int nq : {1, 48, 65535})
            for (int n_theta : {1, 25, ROAM_MATCH_MAX_ANGLES})
                for (int kx : {0, 1, 12, 32, 127, ROAM_MATCH_MAX_SHIFT})
                    for (int ky : {0, 1, 12, 32, 127, ROAM_MATCH_MAX_SHIFT})
                        for (int forced : {0, -1, 1, 7, 31, 2147483647}) {
                            int32_t rows = -1, n_blk = -1;
                            map_match_plan(cu, nq, n_theta, kx, ky, forced, &rows, &n_blk);
                            const int rowlen = 2 * kx + 1, nb = 2 * ky + 1;
                            CHECK(rows >= 1 && rows <= nb && rows * rowlen <= MM_CAND && (n_blk - 1) * rows < nb && n_blk * (int64_t)rows >= nb);
                            if (forced > 0) CHECK(rows == (forced < nb && forced * (int64_t)rowlen <= MM_CAND ? forced : nb < MM_CAND / rowlen ? nb : MM_CAND / rowlen));
                        }
    printf("%d checks failed\n", bad);
    return bad ? 1 : 0;
}
