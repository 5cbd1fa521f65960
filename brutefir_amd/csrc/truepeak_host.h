// truepeak_host.h -- the host half of the limiter's true-peak detector (bfhip_nupc_set_limiter_detector and
// the calls behind it, include/bfhip_nupc.h): the taps of the four-phase interpolator, the argument checks,
// and the detector of the definition evaluated frame by frame (bfhip_selftest_truepeak).  Plain C++: no HIP
// call and no HIP header, so that it compiles into a stand-alone host program (tests/truepeak_host_check.cpp)
// as well as into the library.
#pragma once
#include <cmath>
#include <string>

namespace bfhip {

constexpr int kTpSamplePeak = 0;                       // BFHIP_NUPC_LIMIT_SAMPLE_PEAK
constexpr int kTpTruePeak = 1;                         // BFHIP_NUPC_LIMIT_TRUE_PEAK
constexpr int kTpHalf = 12;                            // BFHIP_NUPC_LIMIT_TP_HALF: H
constexpr int kTpTaps = 2 * kTpHalf;                   // taps per phase
constexpr int kTpPhases = 3;                           // q = 1, 2, 3 (phase 0 is the sample itself)
constexpr double kTpBeta = 8.0;                        // of the Kaiser window

// g[q - 1][k], q = 1 .. 3, k = 0 .. 2 H - 1: a kernel argument of the true-peak limit kernel as it stands
struct TruepeakTaps { double g[kTpPhases][kTpTaps]; };

// the modified Bessel function I0 by its power series sum of ((x / 2)^k / k!)^2: every term is positive, so
// nothing cancels, and at x <= 8 the terms fall below 2^-53 of the sum within 40 of them
inline double truepeak_i0(double x) {
    const double h = 0.5 * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; k++) {
        term *= (h / k) * (h / k);
        sum += term;
        if (term < sum * 1e-17) break;
    }
    return sum;
}

// g_q[k] = sinc(v) I0(beta sqrt(1 - (v / H)^2)) / I0(beta), v = k - H + q / 4.  |v| <= H - 1/4 and v is never
// an integer, so neither the root nor the division meets a zero.
inline void truepeak_filter(TruepeakTaps *taps) {
    const double pi = 3.14159265358979323846, i0b = truepeak_i0(kTpBeta);
    for (int q = 1; q <= kTpPhases; q++)
        for (int k = 0; k < kTpTaps; k++) {
            const double v = (double)(k - kTpHalf) + 0.25 * q, w = v / kTpHalf;
            taps->g[q - 1][k] = std::sin(pi * v) / (pi * v) * truepeak_i0(kTpBeta * std::sqrt(1.0 - w * w)) / i0b;
        }
}

// a detector value the contract knows; true peak needs the interpolator's 2 H frames inside the look-ahead
inline bool truepeak_check(int detector, int lookahead_frames, std::string *why) {
    if (detector != kTpSamplePeak && detector != kTpTruePeak) {
        *why = "the detector must be BFHIP_NUPC_LIMIT_SAMPLE_PEAK or BFHIP_NUPC_LIMIT_TRUE_PEAK";
        return false;
    }
    if (detector == kTpTruePeak && lookahead_frames < kTpTaps) {
        *why = "true-peak detection needs lookahead_frames >= " + std::to_string(kTpTaps);
        return false;
    }
    return true;
}

// the envelope's look-ahead under a detector: the interpolator's H frames come out of the limiter's D
inline int truepeak_envelope_lookahead(int detector, int lookahead_frames) {
    return detector == kTpTruePeak ? lookahead_frames - kTpHalf : lookahead_frames;
}

// tp_out[t] = max over q = 0 .. 3 of |u_q[t]| of the definition for one channel, fresh history (x[t < 0] = 0),
// frame by frame: u_0[t] = x~[t - H], u_q[t] = sum over k ascending of g_q[k] x~[t - k], x~ = x if finite, else 0
inline bool truepeak_detect(long n, const double x[], double tp_out[]) {
    if (n < 0 || (n > 0 && (!x || !tp_out))) return false;
    TruepeakTaps taps;
    truepeak_filter(&taps);
    auto at = [&](long t) { return t >= 0 && std::isfinite(x[t]) ? x[t] : 0.0; };
    for (long t = 0; t < n; t++) {
        double peak = std::fabs(at(t - kTpHalf));
        for (int q = 0; q < kTpPhases; q++) {
            double u = 0.0;
            for (int k = 0; k < kTpTaps; k++) u += taps.g[q][k] * at(t - k);
            peak = std::fmax(peak, std::fabs(u));
        }
        tp_out[t] = peak;
    }
    return true;
}

}  // namespace bfhip
