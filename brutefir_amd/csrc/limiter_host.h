// limiter_host.h -- the host half of the look-ahead peak limiter (bfhip_nupc_enable_limiter and the calls
// behind it, include/bfhip_nupc.h): the argument checks, the release coefficient and the envelope of the
// definition, evaluated frame by frame (bfhip_selftest_limiter_envelope).  Plain C++: no HIP call and no HIP
// header, so that it compiles into a stand-alone host program (tests/limiter_host_check.cpp) as well as
// into the library.
#pragma once
#include <cmath>
#include <string>
#include <vector>

namespace bfhip {

constexpr int kLimLookaheadMax = 1024;                 // BFHIP_NUPC_LIMIT_LOOKAHEAD_MAX
constexpr int kLimGroupsMax = 32;                      // BFHIP_NUPC_LIMIT_GROUPS_MAX
constexpr int kLimGroupMax = 8;                        // BFHIP_NUPC_LIMIT_GROUP_MAX

// 1 <= lookahead <= kLimLookaheadMax; release finite, 0 or in [1, 1e7]
inline bool limiter_check(int lookahead_frames, double release_frames, std::string *why) {
    if (lookahead_frames < 1 || lookahead_frames > kLimLookaheadMax) {
        *why = "lookahead_frames must be 1 .. " + std::to_string(kLimLookaheadMax);
        return false;
    }
    if (!std::isfinite(release_frames) || !(release_frames == 0.0 || (release_frames >= 1.0 && release_frames <= 1e7))) {
        *why = "release_frames must be 0 or 1 .. 1e7";
        return false;
    }
    return true;
}

// a of e[t] = min(m[t], 1 - a (1 - e[t - 1]))
inline double limiter_release_coef(double release_frames) {
    return release_frames == 0.0 ? 0.0 : std::exp(-1.0 / release_frames);
}

// > 0, finite or +INFINITY (NaN fails the comparison)
inline bool limiter_threshold_ok(double threshold) { return threshold > 0.0; }

// a new group's channels: 1 .. kLimGroupMax of them, in range, pairwise distinct, in no other group
// (group_of[ch] < 0)
inline bool limiter_check_group(const std::vector<int> &group_of, int n_groups, const int ch[], int n_ch,
                                double threshold, std::string *why) {
    if (n_groups >= kLimGroupsMax) { *why = "at most " + std::to_string(kLimGroupsMax) + " groups"; return false; }
    if (!ch || n_ch < 1 || n_ch > kLimGroupMax) {
        *why = "a group has 1 .. " + std::to_string(kLimGroupMax) + " channels";
        return false;
    }
    for (int i = 0; i < n_ch; i++) {
        if (ch[i] < 0 || ch[i] >= (int)group_of.size()) { *why = "output channel " + std::to_string(ch[i]) + " is out of range"; return false; }
        if (group_of[ch[i]] >= 0) {
            *why = "output channel " + std::to_string(ch[i]) + " is in group " + std::to_string(group_of[ch[i]]) + " already";
            return false;
        }
        for (int j = 0; j < i; j++)
            if (ch[j] == ch[i]) { *why = "output channel " + std::to_string(ch[i]) + " is listed twice"; return false; }
    }
    if (!limiter_threshold_ok(threshold)) { *why = "the threshold must be > 0 (finite or +INFINITY)"; return false; }
    return true;
}

// s[0..n) of the definition from p[0..n), fresh state (r = e = 1 before frame 0), frame by frame and term by
// term: the window minimum and the box sum both walk j = 0 .. D, newest frame first
inline bool limiter_envelope(int lookahead_frames, double release_frames, long n, const double p[], double s_out[]) {
    std::string why;
    if (!limiter_check(lookahead_frames, release_frames, &why) || n < 0 || (n > 0 && (!p || !s_out))) return false;
    const int D = lookahead_frames, W = D + 1;
    const double a = limiter_release_coef(release_frames);
    std::vector<double> r((size_t)W, 1.0), e((size_t)W, 1.0);      // frame t lives in cell t mod W
    double e_prev = 1.0;
    for (long t = 0; t < n; t++) {
        r[(size_t)(t % W)] = p[t] > 1.0 ? 1.0 / p[t] : 1.0;
        double m = 1.0;
        for (int j = 0; j <= D; j++) { const double v = r[(size_t)(((t - j) % W + W) % W)]; m = v < m ? v : m; }
        const double rel = 1.0 - a * (1.0 - e_prev);
        e_prev = m < rel ? m : rel;
        e[(size_t)(t % W)] = e_prev;
        double sum = 0.0;
        for (int j = 0; j <= D; j++) sum += e[(size_t)(((t - j) % W + W) % W)];
        s_out[t] = sum / (double)W;
    }
    return true;
}

}  // namespace bfhip
