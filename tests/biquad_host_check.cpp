// The host half of the parametric-equaliser sections (brutefir_amd/csrc/biquad_host.h: the designer and the
// section check) as a stand-alone program, for a build with -fsanitize=address,undefined on the CPU
// (tests/test_nupc_biquads_abi.py compiles and runs it).  It feeds them the cases of the ABI test and of the
// GPU test's error list; exit status 0 and "ok" when every answer is the expected one.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../brutefir_amd/csrc/biquad_host.h"

using namespace bfhip;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double f0s[] = {15.0 / 48000.0, 0.01, 0.25, 0.49};
    std::string why;

    // the designer: every type at every frequency gives one stable section
    for (int type = 0; type < kBiquadTypes; type++)
        for (double f0 : f0s)
            for (double gain : {-12.0, 0.0, 6.0}) {
                // heap, exactly five doubles: a write past coef[4] is the sanitizer's to see
                std::vector<double> coef(5, nan);
                EXPECT(biquad_design(type, f0, gain, 0.707, coef.data()));
                EqBiquads q;
                EXPECT(biquad_check(1, coef.data(), &q, &why));
                EXPECT(q.n == 1 && q.c[0] == coef[0] && q.c[4] == coef[4]);
            }

    // the designer's errors leave coef untouched
    {
        std::vector<double> coef(5, 7.0);
        EXPECT(!biquad_design(-1, 0.1, 0.0, 1.0, coef.data()));
        EXPECT(!biquad_design(7, 0.1, 0.0, 1.0, coef.data()));
        EXPECT(!biquad_design(0, 0.0, 0.0, 1.0, coef.data()));
        EXPECT(!biquad_design(0, -0.1, 0.0, 1.0, coef.data()));
        EXPECT(!biquad_design(0, 0.5, 0.0, 1.0, coef.data()));
        EXPECT(!biquad_design(0, nan, 0.0, 1.0, coef.data()));
        EXPECT(!biquad_design(0, 0.1, 0.0, 0.0, coef.data()));
        EXPECT(!biquad_design(0, 0.1, 0.0, -1.0, coef.data()));
        EXPECT(!biquad_design(0, 0.1, 0.0, nan, coef.data()));
        EXPECT(!biquad_design(0, 0.1, 0.0, inf, coef.data()));
        EXPECT(!biquad_design(0, 0.1, nan, 1.0, coef.data()));
        EXPECT(!biquad_design(0, 0.1, inf, 1.0, coef.data()));
        EXPECT(!biquad_design(0, 0.1, 0.0, 1.0, nullptr));
        for (double v : coef) EXPECT(v == 7.0);
    }

    // the section check: counts, NULL, non-finite values, the two edges of the stability triangle
    {
        std::vector<double> good(5 * kBiquadMax);
        for (int k = 0; k < kBiquadMax; k++) EXPECT(biquad_design(k % kBiquadTypes, 0.001 + 0.014 * k, 3.0, 1.0 + k, &good[5 * k]));
        EqBiquads q;
        q.n = -1;
        EXPECT(!biquad_check(0, good.data(), &q, &why) && q.n == -1);
        EXPECT(!biquad_check(kBiquadMax + 1, good.data(), &q, &why) && q.n == -1);      // must not read section 32
        EXPECT(!biquad_check(-3, good.data(), &q, &why) && q.n == -1);
        EXPECT(!biquad_check(1, nullptr, &q, &why) && q.n == -1);
        for (int i = 0; i < 5; i++)
            for (double v : {nan, inf, -inf}) {
                std::vector<double> bad(good.begin(), good.begin() + 15);
                bad[5 + i] = v;
                EXPECT(!biquad_check(3, bad.data(), &q, &why) && q.n == -1);
                EXPECT(why.find("section 1") != std::string::npos);
            }
        const double edges[][2] = {{0.0, 1.0}, {0.0, -1.0}, {1.5, 0.5}, {-1.5, 0.5}, {2.0, 1.0}, {0.0, 1.5}, {3.0, 0.5}};
        for (const auto &e : edges) {
            std::vector<double> bad(good.begin(), good.begin() + 15);
            bad[13] = e[0]; bad[14] = e[1];
            EXPECT(!biquad_check(3, bad.data(), &q, &why) && q.n == -1);
            EXPECT(why.find("section 2") != std::string::npos);
        }
        EXPECT(biquad_check(kBiquadMax, good.data(), &q, &why) && q.n == kBiquadMax);
        for (int i = 0; i < 5 * kBiquadMax; i++) EXPECT(q.c[i] == good[i]);
        EXPECT(biquad_check(1, good.data(), &q, &why) && q.n == 1);
    }

    std::printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
