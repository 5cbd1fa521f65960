// dither_init.h -- the host half of HP-TPDF dither (dither.c:75-139), shared by the uniform
// engine (bfhip.hip) and the non-uniform convolver (nupc.hip): the Tausworthe table and its
// spacing, the randmap, the per-slot start states, and their upload.  One copy, so the two
// paths walk the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "alloc.h"
#include "kernels.h"

namespace bfhip {

// dither_init for n channels, max_samples_per_loop = L: table spacing and n * spacing + 1
// Tausworthe bytes.  Returns "" or the reference's error message (max_size too small).
inline std::string dither_make_table(int n, int sample_rate, int max_size, int L, int *spacing_out,
                                     std::vector<int8_t> *table) {
    int spacing = 10 * sample_rate;
    const int minspacing = sample_rate > L ? sample_rate : L;
    if (spacing < minspacing) spacing = minspacing;
    if (max_size > 0 && n * spacing > max_size) spacing = max_size / n;
    if (spacing < minspacing) {
        char buf[160];
        snprintf(buf, sizeof(buf), "Maximum dither table size %d bytes is too small, must at least be %d bytes.",
                 max_size, n * sample_rate * minspacing);
        return buf;
    }
    *spacing_out = spacing;
    table->resize((size_t)n * spacing + 1);
    uint32_t st[3];
    auto lcg = [](uint32_t v) { return (uint32_t)(69069u * v); };
    st[0] = lcg(1); st[1] = lcg(st[0]); st[2] = lcg(st[1]);
    auto taus = [&]() {
        st[0] = ((st[0] & 4294967294u) << 12) ^ (((st[0] << 13) ^ st[0]) >> 19);
        st[1] = ((st[1] & 4294967288u) << 4) ^ (((st[1] << 2) ^ st[1]) >> 25);
        st[2] = ((st[2] & 4294967280u) << 17) ^ (((st[2] << 3) ^ st[2]) >> 11);
        return st[0] ^ st[1] ^ st[2];
    };
    for (int i = 0; i < 6; i++) taus();
    for (auto &b : *table) b = (int8_t)(taus() & 0xFF);
    return "";
}

// device copies of the table, the randmap (512 reals, index -256..255 at +256) and the slot
// states (slot i starts at rank[i] * spacing + 1 with zero error feedback, dither.c:133-137)
inline hipError_t dither_upload_tables(const std::vector<int8_t> &table, int spacing, const std::vector<int> &rank,
                                       int rs, int8_t **d_table, void **d_randmap, void **d_state) {
    hipError_t e;
    if ((e = bfhip_internal_dev_alloc((void **)d_table, table.size())) != hipSuccess) return e;
    if ((e = hipMemcpy(*d_table, table.data(), table.size(), hipMemcpyHostToDevice)) != hipSuccess) return e;
    // randmap[d] = 0.5 + (d + 1)/255 for d in -255..253, [-256] = -0.5, [254] = 1.5
    // (dither.c:115-131).  The reference indexes it with int8 - int8, which can be +255: one
    // element past its table (undefined there); defined here by continuing the formula.
    std::vector<unsigned char> map(512 * rs);
    for (int d = -256; d < 256; d++) {
        if (rs == 4) {
            float v = d == -256 ? -0.5f : (d == 254 ? 1.5f : (float)(0.5 + 1.0 / 255.0 + 1.0 / 255.0 * (float)d));
            ((float *)map.data())[d + 256] = v;
        } else {
            double v = d == -256 ? -0.5 : (d == 254 ? 1.5 : 0.5 + 1.0 / 255.0 + 1.0 / 255.0 * (double)d);
            ((double *)map.data())[d + 256] = v;
        }
    }
    if ((e = bfhip_internal_dev_alloc(d_randmap, map.size())) != hipSuccess) return e;
    if ((e = hipMemcpy(*d_randmap, map.data(), map.size(), hipMemcpyHostToDevice)) != hipSuccess) return e;
    const size_t ssz = rs == 4 ? sizeof(DitherState<float>) : sizeof(DitherState<double>);
    std::vector<unsigned char> stv(ssz * rank.size(), 0);
    for (size_t i = 0; i < rank.size(); i++) *(int *)(stv.data() + ssz * i) = rank[i] * spacing + 1;
    if ((e = bfhip_internal_dev_alloc(d_state, stv.size())) != hipSuccess) return e;
    return hipMemcpy(*d_state, stv.data(), stv.size(), hipMemcpyHostToDevice);
}

}  // namespace bfhip
