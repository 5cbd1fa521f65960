// loudness_host.h -- the host half of the BS.1770 loudness meter (bfhip_nupc_enable_loudness and the calls
// behind it, include/bfhip_nupc.h): the argument checks, the K-weighting design for any rate, the sub-block
// energies of the definition, evaluated frame by frame (bfhip_selftest_loudness_energy), and the read-outs
// with the gate (bfhip_nupc_get_loudness, bfhip_selftest_loudness_gate).  Plain C++: no HIP call and no HIP
// header, so that it compiles into a stand-alone host program (tests/loudness_host_check.cpp) as well as
// into the library.  The one step of the two sections is shared with the kernel (BFHIP_LOUD_HD).
#pragma once
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define BFHIP_LOUD_HD __host__ __device__
#else
#define BFHIP_LOUD_HD
#endif

namespace bfhip {

constexpr int kLoudGroupsMax = 32;                     // BFHIP_NUPC_LOUD_GROUPS_MAX
constexpr int kLoudGroupMax = 16;                      // BFHIP_NUPC_LOUD_GROUP_MAX
constexpr int kLoudRateMin = 8000, kLoudRateMax = 768000;
constexpr int kLoudHistoryMin = 30, kLoudHistoryMax = 1 << 22;

// what bfhip_loudness holds (include/bfhip_nupc.h), under a name of its own: this header includes nothing of include/
struct LoudnessReadout {
    double momentary, short_term, integrated;
    long long subblocks, first;
    int wrapped;
};

// a multiple of 10 in 8000 .. 768000: S = rate / 10 frames are 100 ms, and the shelf needs fs well above 2 x 1682 Hz
inline bool loudness_rate_ok(int sample_rate, std::string *why) {
    if (sample_rate < kLoudRateMin || sample_rate > kLoudRateMax || sample_rate % 10 != 0) {
        *why = "sample_rate must be a multiple of 10 in " + std::to_string(kLoudRateMin) + " .. " + std::to_string(kLoudRateMax);
        return false;
    }
    return true;
}

inline bool loudness_check(int sample_rate, int history_subblocks, std::string *why) {
    if (!loudness_rate_ok(sample_rate, why)) return false;
    if (history_subblocks < kLoudHistoryMin || history_subblocks > kLoudHistoryMax) {
        *why = "history_subblocks must be " + std::to_string(kLoudHistoryMin) + " .. " + std::to_string(kLoudHistoryMax);
        return false;
    }
    return true;
}

// a new group's members: 1 .. kLoudGroupMax of them, in range, pairwise distinct; weights finite and >= 0
// (weight == nullptr: all 1)
inline bool loudness_check_group(int n_out, int n_groups, const int ch[], const double weight[], int n_ch, std::string *why) {
    if (n_groups >= kLoudGroupsMax) { *why = "at most " + std::to_string(kLoudGroupsMax) + " groups"; return false; }
    if (!ch || n_ch < 1 || n_ch > kLoudGroupMax) {
        *why = "a group has 1 .. " + std::to_string(kLoudGroupMax) + " channels";
        return false;
    }
    for (int i = 0; i < n_ch; i++) {
        if (ch[i] < 0 || ch[i] >= n_out) { *why = "output channel " + std::to_string(ch[i]) + " is out of range"; return false; }
        for (int j = 0; j < i; j++)
            if (ch[j] == ch[i]) { *why = "output channel " + std::to_string(ch[i]) + " is listed twice"; return false; }
        if (weight && !(std::isfinite(weight[i]) && weight[i] >= 0.0)) {
            *why = "the weight of output channel " + std::to_string(ch[i]) + " must be finite and >= 0";
            return false;
        }
    }
    return true;
}

// the two sections for any rate, by the bilinear redesign of the BS.1770 prototype:
// c = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
inline void kweighting_design(int sample_rate, double c[10]) {
    const double pi = 3.14159265358979323846, fs = (double)sample_rate;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0; c[6] = -2.0; c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
}

// one frame through the shelf and then the high-pass, each in transposed direct form II:
// o = b0 v + s1;  s1 = b1 v - a1 o + s2;  s2 = b2 v - a2 o.   s = shelf s1 s2, high-pass s1 s2
BFHIP_LOUD_HD inline double kweighting_step(const double c[10], double s[4], double v) {
    const double o = c[0] * v + s[0];
    s[0] = c[1] * v - c[3] * o + s[1];
    s[1] = c[2] * v - c[4] * o;
    const double z = c[5] * o + s[2];
    s[2] = c[6] * o - c[8] * z + s[3];
    s[3] = c[7] * o - c[9] * z;
    return z;
}

// the 4 x 4 matrix that takes the four state values over `frames` frames of zero input (row-major), by walking
// the sections from each unit state: what the kernel's chunked scan carries a chunk's start state forward with
inline void kweighting_transition(const double c[10], int frames, double m[16]) {
    for (int col = 0; col < 4; col++) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[col] = 1.0;
        for (int t = 0; t < frames; t++) (void)kweighting_step(c, s, 0.0);
        for (int row = 0; row < 4; row++) m[row * 4 + col] = s[row];
    }
}

inline void loudness_mat_mul(const double a[16], const double b[16], double out[16]) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc += a[i * 4 + k] * b[k * 4 + j];
            out[i * 4 + j] = acc;
        }
}

// E[j] of the definition for one channel with weight 1, fresh state: v[0..n) as fractions of full scale (a value
// that is not finite counts as 0), frame by frame; E_out takes the n / S complete sub-blocks -> their number
inline long loudness_energy(int sample_rate, long n, const double v[], double E_out[]) {
    std::string why;
    if (!loudness_rate_ok(sample_rate, &why) || n < 0 || (n > 0 && (!v || !E_out))) return -1;
    double c[10], s[4] = {0.0, 0.0, 0.0, 0.0}, sum = 0.0;
    kweighting_design(sample_rate, c);
    const long S = sample_rate / 10;
    long j = 0, in_block = 0;
    for (long t = 0; t < n; t++) {
        const double z = kweighting_step(c, s, std::isfinite(v[t]) ? v[t] : 0.0);
        sum += z * z;
        if (++in_block == S) { E_out[j++] = sum; sum = 0.0; in_block = 0; }
    }
    return j;
}

// l(m) = -0.691 + 10 log10(m), l(0) = -INFINITY
inline double loudness_lufs(double m) {
    return m > 0.0 ? -0.691 + 10.0 * std::log10(m) : -std::numeric_limits<double>::infinity();
}

// The read-outs from the history.  `subblocks` sub-blocks are complete (J = subblocks - 1); E(j) gives the energy of
// sub-block j for max(0, subblocks - history) <= j < subblocks; `reset` is the first sub-block the integrated value
// may cover.  Windows sum oldest sub-block first.
template <typename Get>
inline void loudness_readout(int sample_rate, long long subblocks, long long history, long long reset, Get E, LoudnessReadout *out) {
    const double S = (double)(sample_rate / 10), ninf = -std::numeric_limits<double>::infinity();
    const long long J = subblocks - 1, oldest = subblocks > history ? subblocks - history : 0;
    auto window = [&](long long last, int len) {
        double sum = 0.0;
        for (long long j = last - len + 1; j <= last; j++) sum += E(j);
        return sum / ((double)len * S);
    };
    out->subblocks = subblocks;
    out->first = reset > oldest ? reset : oldest;
    out->wrapped = oldest > reset ? 1 : 0;
    out->momentary = subblocks >= 4 ? loudness_lufs(window(J, 4)) : ninf;
    out->short_term = subblocks >= 30 ? loudness_lufs(window(J, 30)) : ninf;
    // 400 ms gating blocks with 75 % overlap: absolute gate at -70 LUFS, relative gate 10 LU under the mean of the
    // blocks that pass it
    std::vector<double> B;
    for (long long j = out->first + 3; j <= J; j++) {
        const double b = window(j, 4);
        if (loudness_lufs(b) > -70.0) B.push_back(b);
    }
    out->integrated = ninf;
    if (B.empty()) return;
    double sum = 0.0;
    for (double b : B) sum += b;
    const double rel = loudness_lufs(sum / (double)B.size()) - 10.0;
    double sum2 = 0.0;
    long cnt = 0;
    for (double b : B)
        if (loudness_lufs(b) > rel) { sum2 += b; cnt++; }
    if (cnt) out->integrated = loudness_lufs(sum2 / (double)cnt);
}

// the read-outs of E[0 .. n_sub): sub-blocks 0 on, none dropped, no reset
inline bool loudness_gate(int sample_rate, long n_sub, const double E[], LoudnessReadout *out) {
    std::string why;
    if (!loudness_rate_ok(sample_rate, &why) || n_sub < 0 || (n_sub > 0 && !E) || !out) return false;
    loudness_readout(sample_rate, n_sub, n_sub > 0 ? n_sub : 1, 0, [&](long long j) { return E[j]; }, out);
    return true;
}

}  // namespace bfhip
