// biquad_host.h -- the host half of the parametric-equaliser sections (bfhip_biquad_design and the section
// check of bfhip_nupc_render_biquads*, include/bfhip_nupc.h).  Plain C++: no HIP call and no HIP header, so
// that it compiles into a stand-alone host program (tests/biquad_host_check.cpp) as well as into the library.
//
// A section is five doubles b0, b1, b2, a1, a2 with a0 = 1:
//     H(z) = (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2)
#pragma once
#include <cmath>
#include <string>

namespace bfhip {

constexpr int kBiquadMax = 32;                         // BFHIP_BIQUAD_MAX
constexpr int kBiquadTypes = 7;                        // BFHIP_BIQUAD_PEAK .. BFHIP_BIQUAD_ALL_PASS

// the kernel-argument copy of a cascade (eq_biquad.h): 1280 bytes and a count
struct EqBiquads {
    double c[kBiquadMax * 5];
    int n;
};

// the audio-EQ-cookbook section of `type` at f0 (normalised, 0 < f0 < 0.5); false on a bad argument, and
// coef is then untouched.  1 - cos w0 = 2 sin^2(w0/2) and 1 + cos w0 = 2 cos^2(w0/2) are written that way.
inline bool biquad_design(int type, double f0, double gain_db, double q, double coef[5]) {
    if (!coef || type < 0 || type >= kBiquadTypes) return false;
    if (!(f0 > 0.0) || !(f0 < 0.5) || !(q > 0.0) || !std::isfinite(q) || !std::isfinite(gain_db)) return false;
    const double w0 = 2.0 * M_PI * f0;
    const double cw = std::cos(w0), alpha = std::sin(w0) / (2.0 * q);
    const double sh = std::sin(0.5 * w0), ch = std::cos(0.5 * w0);
    const double A = std::pow(10.0, gain_db / 40.0), sq = 2.0 * std::sqrt(A) * alpha;
    double b0, b1, b2, a0, a1, a2;
    switch (type) {
    case 0:                                            // peak
        b0 = 1.0 + alpha * A; b1 = -2.0 * cw; b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A; a1 = -2.0 * cw; a2 = 1.0 - alpha / A;
        break;
    case 1:                                            // low shelf
        b0 = A * ((A + 1.0) - (A - 1.0) * cw + sq); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cw);
        b2 = A * ((A + 1.0) - (A - 1.0) * cw - sq);
        a0 = (A + 1.0) + (A - 1.0) * cw + sq; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cw);
        a2 = (A + 1.0) + (A - 1.0) * cw - sq;
        break;
    case 2:                                            // high shelf
        b0 = A * ((A + 1.0) + (A - 1.0) * cw + sq); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cw);
        b2 = A * ((A + 1.0) + (A - 1.0) * cw - sq);
        a0 = (A + 1.0) - (A - 1.0) * cw + sq; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cw);
        a2 = (A + 1.0) - (A - 1.0) * cw - sq;
        break;
    case 3:                                            // low pass
        b0 = sh * sh; b1 = 2.0 * sh * sh; b2 = sh * sh;
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
        break;
    case 4:                                            // high pass
        b0 = ch * ch; b1 = -2.0 * ch * ch; b2 = ch * ch;
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
        break;
    case 5:                                            // notch
        b0 = 1.0; b1 = -2.0 * cw; b2 = 1.0;
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
        break;
    default:                                           // all pass
        b0 = 1.0 - alpha; b1 = -2.0 * cw; b2 = 1.0 + alpha;
        a0 = 1.0 + alpha; a1 = -2.0 * cw; a2 = 1.0 - alpha;
        break;
    }
    coef[0] = b0 / a0; coef[1] = b1 / a0; coef[2] = b2 / a0; coef[3] = a1 / a0; coef[4] = a2 / a0;
    return true;
}

// 1 .. kBiquadMax sections, every value finite, every section strictly stable (|a2| < 1 and |a1| < 1 + a2:
// the denominator then has no zero on the unit circle).  Fills *q and returns true, or leaves *q as it was
// and says in *why what is wrong, naming the section.
inline bool biquad_check(int n_sections, const double coef[], EqBiquads *q, std::string *why) {
    if (!coef || n_sections < 1 || n_sections > kBiquadMax) {
        *why = "1 .. " + std::to_string(kBiquadMax) + " sections of 5 doubles";
        return false;
    }
    for (int k = 0; k < n_sections; k++) {
        const double *c = coef + 5 * k;
        for (int i = 0; i < 5; i++)
            if (!std::isfinite(c[i])) { *why = "section " + std::to_string(k) + ": a coefficient is not finite"; return false; }
        if (!(std::fabs(c[4]) < 1.0) || !(std::fabs(c[3]) < 1.0 + c[4])) {
            *why = "section " + std::to_string(k) + ": not strictly stable (needs |a2| < 1 and |a1| < 1 + a2)";
            return false;
        }
    }
    for (int i = 0; i < 5 * n_sections; i++) q->c[i] = coef[i];
    q->n = n_sections;
    return true;
}

}  // namespace bfhip
