// subdelay_filter.h -- the taps of the sub-sample delay filters (delay.c:56-76, 476-483), shared
// by the uniform engine (bfhip.hip) and the non-uniform convolver (nupc.hip).  Host only.  One
// copy, so the two paths filter with the same numbers.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

namespace bfhip {

// Kaiser window exactly as the reference applies it to its sub-sample filters
// (firwindow.c:12-160 via delay.c:56-76; note the window is applied twice when offset != 0)
inline double sd_bessel_i0(double x) {
    double n = 1.0, a = 1.0, sum = 1.0;
    const double h = x / 2.0;
    do { a *= h; a /= n; sum += a * a; n += 1.0; } while (a != 0.0 && std::isfinite(sum));
    return sum;
}

template <typename T>
void sd_make_filter(std::vector<T> &f, int half, double offset, double beta) {
    const int len = 2 * half + 1;
    f.assign(len, (T)0);
    if (offset == 0.0) { f[half] = (T)1; return; }            // delay.c:476-483: a unit pulse
    for (int n = 0; n < len; n++) {
        const double x = M_PI * ((double)(n - half) - offset);
        f[n] = (T)(x == 0.0 ? 1.0 : sin(x) / x);
    }
    const double inv = 1.0 / sd_bessel_i0(beta);
    auto kaiser = [&](double x) {
        if (x < -1.0) x = -1.0;
        if (x > 1.0) x = 1.0;
        return sd_bessel_i0(beta * sqrt(1.0 - x * x)) * inv;
    };
    int max = half + (int)floor(offset);
    offset -= floor(offset);
    if (fabs(offset) < 1e-20) offset = 0.0;
    double step = 1.0 / ((double)max + offset);
    if (offset == 0.0) max -= 1;
    int n = 0;
    for (; n <= max; n++) { const double y = kaiser(-1.0 + (double)n * step); f[n] = (T)(f[n] * y); f[n] = (T)(f[n] * y); }
    if (offset == 0.0) max += 1;
    step = 1.0 / ((double)(len - max - 1) - offset);
    for (; n < len; n++) { const double y = kaiser(((double)(n - max) - offset) * step); f[n] = (T)(f[n] * y); f[n] = (T)(f[n] * y); }
}

// the bank of all 199 filters, index 99 + subdelay (hundredths of a sample in (-100, 100),
// BF_SAMPLE_SLOTS), `realsize` wide, [199][2 * half + 1]; always built with beta 9 (delay.c:73)
inline std::vector<unsigned char> sd_make_bank(int half, int realsize) {
    const int flen = 2 * half + 1;
    std::vector<unsigned char> bank((size_t)199 * flen * realsize);
    for (int sd = -99; sd <= 99; sd++) {
        if (realsize == 4) {
            std::vector<float> f;
            sd_make_filter(f, half, (double)sd / 100, 9.0);
            memcpy(bank.data() + (size_t)(99 + sd) * flen * 4, f.data(), f.size() * 4);
        } else {
            std::vector<double> f;
            sd_make_filter(f, half, (double)sd / 100, 9.0);
            memcpy(bank.data() + (size_t)(99 + sd) * flen * 8, f.data(), f.size() * 8);
        }
    }
    return bank;
}

}  // namespace bfhip
