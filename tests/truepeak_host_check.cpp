// truepeak_host_check.cpp -- a program of its own around csrc/truepeak_host.h (plain host code), built by
// tests/test_nupc_truepeak_abi.py with the address and undefined-behaviour sanitizers: the taps, the detector
// check at both sides of its limit, and the frame-by-frame detector at the ends of its input.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../brutefir_amd/csrc/truepeak_host.h"

using namespace bfhip;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main() {
    std::string why;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    EXPECT(kTpTaps == 24 && kTpHalf == 12);
    EXPECT(truepeak_check(kTpSamplePeak, 1, &why) && truepeak_check(kTpSamplePeak, 1024, &why));
    EXPECT(truepeak_check(kTpTruePeak, 24, &why) && truepeak_check(kTpTruePeak, 1024, &why));
    EXPECT(!truepeak_check(kTpTruePeak, 23, &why) && why.find("24") != std::string::npos);
    EXPECT(!truepeak_check(kTpTruePeak, 1, &why));
    EXPECT(!truepeak_check(2, 64, &why) && !truepeak_check(-1, 64, &why) && why.find("detector") != std::string::npos);
    EXPECT(truepeak_envelope_lookahead(kTpSamplePeak, 64) == 64 && truepeak_envelope_lookahead(kTpTruePeak, 24) == 12);

    EXPECT(truepeak_i0(0.0) == 1.0 && std::fabs(truepeak_i0(8.0) - 427.56411572180474) < 1e-10);
    TruepeakTaps taps;
    truepeak_filter(&taps);
    for (int q = 0; q < kTpPhases; q++) {
        double sum = 0.0;
        for (int k = 0; k < kTpTaps; k++) {
            EXPECT(std::isfinite(taps.g[q][k]) && std::fabs(taps.g[q][k]) < 1.0);
            EXPECT(std::fabs(taps.g[q][k] - taps.g[kTpPhases - 1 - q][kTpTaps - 1 - k]) < 1e-15);   // q and 4 - q mirror
            sum += taps.g[q][k];
        }
        EXPECT(std::fabs(sum - 1.0) < 1e-4);           // a constant comes through (the interpolation error at 0 Hz)
    }
    EXPECT(taps.g[1][kTpHalf] > 0.6 && taps.g[1][kTpHalf] < 0.64);

    // the detector: nothing before frame 0, phase 0 is the sample H frames late, non-finite samples count as 0
    const long n = 200;
    std::vector<double> x((size_t)n, 0.0), tp((size_t)n, -1.0);
    x[0] = 1.0; x[(size_t)(n - 1)] = 5.0;
    EXPECT(truepeak_detect(n, x.data(), tp.data()));
    auto widest = [&](long k) { return std::fmax(std::fmax(std::fabs(taps.g[0][k]), std::fabs(taps.g[1][k])), std::fabs(taps.g[2][k])); };
    for (long t = 0; t < n - 1; t++) EXPECT(tp[(size_t)t] == (t == kTpHalf ? 1.0 : t < kTpTaps ? widest(t) : 0.0));
    EXPECT(tp[(size_t)(n - 1)] == 5.0 * widest(0));
    std::vector<double> bad = x, tp2((size_t)n, -1.0);
    bad[50] = nan; bad[60] = inf; bad[61] = -inf;
    EXPECT(truepeak_detect(n, bad.data(), tp2.data()));
    for (long t = 0; t < n; t++) EXPECT(tp2[(size_t)t] == tp[(size_t)t]);
    // the fs/4 sine 45 degrees off the sampling instants: samples at 0.7071, true peak at 1 in every other frame
    for (long t = 0; t < n; t++) x[(size_t)t] = std::sin(1.5707963267948966 * (double)t + 0.7853981633974483);
    EXPECT(truepeak_detect(n, x.data(), tp.data()));
    for (long t = 2 * kTpTaps; t + 1 < n; t++) {
        EXPECT(std::fabs(std::fmax(tp[(size_t)t], tp[(size_t)(t + 1)]) - 1.0) < 2e-4);
        EXPECT(tp[(size_t)t] > 0.7071);
    }

    std::vector<double> one(1, 2.0), out(1, -1.0);
    EXPECT(truepeak_detect(0, nullptr, nullptr));
    EXPECT(!truepeak_detect(1, nullptr, out.data()) && !truepeak_detect(1, one.data(), nullptr) && !truepeak_detect(-1, one.data(), out.data()));
    EXPECT(truepeak_detect(1, one.data(), out.data()) && out[0] == 2.0 * widest(0));
    if (fails == 0) printf("ok\n");
    return fails ? 1 : 0;
}
