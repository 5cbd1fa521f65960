// loudness_host_check.cpp -- a program of its own around csrc/loudness_host.h (plain host code), built by
// tests/test_nupc_loudness_abi.py with the address and undefined-behaviour sanitizers: the argument checks at the
// ends of every range, the design at 48 kHz against the standard's table, the energies' sub-block bookkeeping,
// the transition matrix against a walk, and the read-outs over a ring that has wrapped.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../brutefir_amd/csrc/loudness_host.h"

using namespace bfhip;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main() {
    std::string why;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    EXPECT(loudness_check(8000, 30, &why) && loudness_check(768000, 1 << 22, &why) && loudness_check(44100, 36000, &why));
    EXPECT(!loudness_check(8001, 30, &why) && !loudness_check(7990, 30, &why) && !loudness_check(768010, 30, &why));
    EXPECT(!loudness_check(0, 30, &why) && !loudness_check(-48000, 30, &why));
    EXPECT(!loudness_check(48000, 29, &why) && why.find("30") != std::string::npos);
    EXPECT(!loudness_check(48000, (1 << 22) + 1, &why) && !loudness_check(48000, -1, &why));

    const int all[17] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, twice[2] = {3, 3}, far[1] = {17}, neg[1] = {-1};
    const double w5[5] = {1, 1, 1, 1.41, 1.41}, wneg[2] = {1.0, -0.5}, wnan[2] = {nan, 1.0}, winf[2] = {1.0, inf}, w0[2] = {0.0, 1.0};
    EXPECT(loudness_check_group(17, 0, all, nullptr, 16, &why) && loudness_check_group(17, 31, all, w5, 5, &why));
    EXPECT(loudness_check_group(17, 0, all, w0, 2, &why));
    EXPECT(!loudness_check_group(17, 0, all, nullptr, 17, &why) && !loudness_check_group(17, 0, all, nullptr, 0, &why));
    EXPECT(!loudness_check_group(17, 0, nullptr, nullptr, 1, &why) && !loudness_check_group(17, kLoudGroupsMax, all, nullptr, 2, &why));
    EXPECT(!loudness_check_group(17, 0, twice, nullptr, 2, &why) && why.find("3") != std::string::npos);
    EXPECT(!loudness_check_group(17, 0, far, nullptr, 1, &why) && why.find("17") != std::string::npos);
    EXPECT(!loudness_check_group(17, 0, neg, nullptr, 1, &why));
    EXPECT(!loudness_check_group(17, 0, all, wneg, 2, &why) && why.find("channel 1") != std::string::npos);
    EXPECT(!loudness_check_group(17, 0, all, wnan, 2, &why) && !loudness_check_group(17, 0, all, winf, 2, &why));

    // BS.1770-4, tables 1 and 2
    double c[10];
    kweighting_design(48000, c);
    const double want[10] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};
    for (int i = 0; i < 10; i++) EXPECT(std::fabs(c[i] - want[i]) <= 1e-13);

    // energies: n / S complete sub-blocks, nothing written past them, a value that is not finite counts as 0
    for (int rate : {8000, 44100}) {
        const long S = rate / 10;
        for (long n : {0L, 1L, S - 1, S, S + 1, 3 * S + 7}) {
            std::vector<double> v((size_t)n + 1, 0.25), E((size_t)(n / S) + 1, -1.0), E2((size_t)(n / S) + 1, -1.0);
            for (long t = 0; t < n; t += 3) v[(size_t)t] = -0.5;
            EXPECT(loudness_energy(rate, n, v.data(), E.data()) == n / S);
            for (long j = 0; j < n / S; j++) EXPECT(E[(size_t)j] > 0.0);
            EXPECT(E[(size_t)(n / S)] == -1.0);
            if (n > 5) {
                std::vector<double> u = v;
                v[5] = 0.0; u[5] = nan;
                EXPECT(loudness_energy(rate, n, v.data(), E.data()) == n / S && loudness_energy(rate, n, u.data(), E2.data()) == n / S);
                u[5] = -inf;
                for (long j = 0; j < n / S; j++) EXPECT(E[(size_t)j] == E2[(size_t)j]);
                EXPECT(loudness_energy(rate, n, u.data(), E2.data()) == n / S);
                for (long j = 0; j < n / S; j++) EXPECT(E[(size_t)j] == E2[(size_t)j]);
            }
        }
    }
    std::vector<double> one(800, 0.5), e1(2, 0.0);
    EXPECT(loudness_energy(8000, 0, nullptr, nullptr) == 0);
    EXPECT(loudness_energy(8001, 800, one.data(), e1.data()) < 0 && loudness_energy(7990, 800, one.data(), e1.data()) < 0);
    EXPECT(loudness_energy(8000, -1, one.data(), e1.data()) < 0);
    EXPECT(loudness_energy(8000, 800, nullptr, e1.data()) < 0 && loudness_energy(8000, 800, one.data(), nullptr) < 0);

    // the transition matrix and its squares: a state carried over 32 and over 64 frames of zero input
    double m[16], m2[16];
    kweighting_design(8000, c);
    kweighting_transition(c, 32, m);
    loudness_mat_mul(m, m, m2);
    double s[4] = {0.3, -0.2, 0.7, 0.1}, walk[4] = {0.3, -0.2, 0.7, 0.1};
    for (int t = 0; t < 64; t++) (void)kweighting_step(c, walk, 0.0);
    for (int r = 0; r < 4; r++) {
        double acc = 0.0;
        for (int k = 0; k < 4; k++) acc += m2[r * 4 + k] * s[k];
        EXPECT(std::fabs(acc - walk[r]) <= 1e-12);
    }

    // read-outs: a constant programme of mean square 0.1 per frame reads l(0.1) everywhere
    const int rate = 8000;
    const double S = 800.0, level = -0.691 + 10.0 * std::log10(0.1);
    std::vector<double> E(45, 0.1 * S);
    LoudnessReadout r;
    EXPECT(loudness_gate(rate, 45, E.data(), &r));
    EXPECT(std::fabs(r.momentary - level) < 1e-12 && std::fabs(r.short_term - level) < 1e-12 && std::fabs(r.integrated - level) < 1e-12);
    EXPECT(r.subblocks == 45 && r.first == 0 && r.wrapped == 0);
    EXPECT(loudness_gate(rate, 3, E.data(), &r) && r.momentary == -inf && r.short_term == -inf && r.integrated == -inf);
    EXPECT(loudness_gate(rate, 29, E.data(), &r) && r.momentary > -inf && r.short_term == -inf);
    EXPECT(loudness_gate(rate, 0, nullptr, &r) && r.subblocks == 0 && r.integrated == -inf);
    EXPECT(!loudness_gate(rate, 4, nullptr, &r) && !loudness_gate(rate, -1, E.data(), &r) && !loudness_gate(rate, 4, E.data(), nullptr));
    EXPECT(!loudness_gate(8001, 4, E.data(), &r));
    std::vector<double> zero(45, 0.0);
    EXPECT(loudness_gate(rate, 45, zero.data(), &r) && r.momentary == -inf && r.short_term == -inf && r.integrated == -inf);
    // a ring of 30 after 45 sub-blocks: cell j mod 30, only sub-blocks 15 .. 44 are read; and a reset at 40
    std::vector<double> ring(30);
    long reads_outside = 0;
    for (int j = 15; j < 45; j++) ring[(size_t)(j % 30)] = (j < 40 ? 0.1 : 0.4) * S;
    auto get = [&](long long j) { if (j < 15 || j > 44) reads_outside++; return ring[(size_t)(j % 30)]; };
    loudness_readout(rate, 45, 30, 0, get, &r);
    EXPECT(r.first == 15 && r.wrapped == 1 && r.subblocks == 45 && reads_outside == 0);
    EXPECT(r.integrated > level && r.integrated < level + 10.0 * std::log10(4.0));
    loudness_readout(rate, 45, 30, 40, get, &r);
    EXPECT(r.first == 40 && r.wrapped == 0 && reads_outside == 0);
    EXPECT(std::fabs(r.integrated - (level + 10.0 * std::log10(4.0))) < 1e-12);
    loudness_readout(rate, 45, 30, 43, get, &r);           // fewer than four sub-blocks since the reset
    EXPECT(r.first == 43 && r.integrated == -inf && r.momentary > -inf);
    if (fails == 0) printf("ok\n");
    return fails ? 1 : 0;
}
