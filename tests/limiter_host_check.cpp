// limiter_host_check.cpp -- a program of its own around csrc/limiter_host.h (plain host code), built by
// tests/test_nupc_limiter_abi.py with the address and undefined-behaviour sanitizers: the argument checks,
// the release coefficient, and the envelope's two properties at the ends of every range.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../brutefir_amd/csrc/limiter_host.h"

using namespace bfhip;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main() {
    std::string why;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    EXPECT(limiter_check(1, 0.0, &why) && limiter_check(kLimLookaheadMax, 1e7, &why) && limiter_check(64, 1.0, &why));
    EXPECT(!limiter_check(0, 1.0, &why) && !limiter_check(kLimLookaheadMax + 1, 1.0, &why) && !limiter_check(-3, 1.0, &why));
    EXPECT(!limiter_check(8, 0.5, &why) && !limiter_check(8, -1.0, &why) && !limiter_check(8, 1.0000001e7, &why));
    EXPECT(!limiter_check(8, inf, &why) && !limiter_check(8, nan, &why));
    EXPECT(limiter_release_coef(0.0) == 0.0 && limiter_release_coef(1.0) == std::exp(-1.0));
    EXPECT(limiter_threshold_ok(inf) && limiter_threshold_ok(1e-300) && !limiter_threshold_ok(0.0));
    EXPECT(!limiter_threshold_ok(-1.0) && !limiter_threshold_ok(nan) && !limiter_threshold_ok(-inf));

    std::vector<int> group_of(9, -1);
    const int all[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8}, twice[2] = {3, 3}, far[1] = {9}, neg[1] = {-1};
    EXPECT(limiter_check_group(group_of, 0, all, 8, 0.5, &why));
    EXPECT(!limiter_check_group(group_of, 0, all, 9, 0.5, &why));
    EXPECT(!limiter_check_group(group_of, 0, all, 0, 0.5, &why) && !limiter_check_group(group_of, 0, nullptr, 1, 0.5, &why));
    EXPECT(!limiter_check_group(group_of, 0, twice, 2, 0.5, &why) && why.find("3") != std::string::npos);
    EXPECT(!limiter_check_group(group_of, 0, far, 1, 0.5, &why) && why.find("9") != std::string::npos);
    EXPECT(!limiter_check_group(group_of, 0, neg, 1, 0.5, &why));
    EXPECT(!limiter_check_group(group_of, 0, all, 2, 0.0, &why) && !limiter_check_group(group_of, 0, all, 2, nan, &why));
    EXPECT(!limiter_check_group(group_of, kLimGroupsMax, all, 2, 0.5, &why));
    group_of[1] = 4;
    EXPECT(!limiter_check_group(group_of, 5, all, 2, 0.5, &why) && why.find("group 4") != std::string::npos);

    // the envelope: idle input gives exactly 1.0; a burst is held under its ceiling D frames later
    for (int D : {1, 16, 96, kLimLookaheadMax})
        for (double rel : {0.0, 50.0, 1e7}) {
            const long n = 3 * (long)D + 700;
            std::vector<double> p((size_t)n, 0.9), s((size_t)n, -1.0);
            p[0] = 1.0;
            EXPECT(limiter_envelope(D, rel, n, p.data(), s.data()));
            for (long t = 0; t < n; t++) EXPECT(s[(size_t)t] == 1.0);
            p[0] = 7.0; p[(size_t)(n / 2)] = 12.5; p[(size_t)(n / 2 + 1)] = nan; p[(size_t)(n - 1)] = inf;
            EXPECT(limiter_envelope(D, rel, n, p.data(), s.data()));
            for (long t = D; t < n; t++) {
                const double pd = p[(size_t)(t - D)], r = pd > 1.0 ? 1.0 / pd : 1.0;
                EXPECT(s[(size_t)t] <= r + (D + 2) * std::ldexp(1.0, -52));
                EXPECT(s[(size_t)t] > 0.0 && s[(size_t)t] <= 1.0);
            }
        }
    std::vector<double> one(1, 2.0), out(1, 0.0);
    EXPECT(limiter_envelope(1, 0.0, 0, nullptr, nullptr));
    EXPECT(!limiter_envelope(1, 0.0, 1, nullptr, out.data()) && !limiter_envelope(1, 0.0, 1, one.data(), nullptr));
    EXPECT(!limiter_envelope(0, 0.0, 1, one.data(), out.data()) && !limiter_envelope(1, 0.5, 1, one.data(), out.data()));
    EXPECT(!limiter_envelope(1, 0.0, -1, one.data(), out.data()));
    EXPECT(limiter_envelope(1, 0.0, 1, one.data(), out.data()) && out[0] == 0.75);      // (1/2 + 1) / 2
    if (fails == 0) printf("ok\n");
    return fails ? 1 : 0;
}
