// eq_render.h -- an equaliser curve rendered into R real taps on the device (the reference's
// render_equaliser, rendereq.h:20-62, for taps = R; bfhip_nupc_render_eq*, include/bfhip_nupc.h).
//
// The curve is n_bands knots (freq ascending from 0 to 0.5, linear magnitude, phase in radians);
// between two knots magnitude and phase follow a raised cosine:
//     ci(a1, a2, f1, f2, f) = (a1 - a2) 0.5 cos(pi (f - f1) / (f2 - f1)) + (a1 + a2) 0.5
// Bin n = 1 .. R/2 - 1 at f = n / R, i the first band with f <= freq[i + 1]:
//     X[n] = (-1)^n  ci(mag) / R  (cos phi + i sin phi),  phi = ci(phase)
// X[0] = mag[0] / R and X[R/2] = mag[last] / R are real, and the taps are the unnormalised HC2R of
// X.  (-1)^n is the reference's linear-phase term cos(-R pi f + phi) in exact arithmetic; the sign
// form is what is computed here.  Curve, sine and cosine are evaluated in
// float64 for both precisions and rounded to T once.
//
// The transform is the one K3 uses for its HC2R: the R/2 + 1 bins are folded into H = R/2 packed
// complex values (kernels.h: tangle), an inverse complex FFT of H points follows, and its output
// z[n] = (x[2n], x[2n + 1]) IS the array of taps.
//     H <= 8192   one kernel, one workgroup: bins -> fold -> lds_fft -> taps
//     H >= 16384  a spectrum-and-fold kernel over the bins into global scratch, then big_fft_run
//                 (bigfft.h) straight into the taps buffer: no unpack step is needed
// The bands travel in the kernel arguments, so a render in flight never reads caller memory.  No
// atomics: a render is a pure function of its arguments.
#pragma once
#include <vector>

#include "alloc.h"
#include "bigfft.h"

namespace bfhip {

constexpr int kEqMaxBands = 130;
constexpr int kEqMinLog2H = 2, kEqMaxLog2H = 19;       // 8 .. 1048576 taps

struct EqBands {
    double freq[kEqMaxBands], mag[kEqMaxBands], phase[kEqMaxBands];
    int n;
};

// the knots in LDS: [freq | mag | phase], kEqMaxBands doubles each (every thread calls)
__device__ __forceinline__ void eq_load_bands(double *lb, const EqBands &b, int tid, int nt) {
    for (int i = tid; i < b.n; i += nt) {
        lb[i] = b.freq[i];
        lb[kEqMaxBands + i] = b.mag[i];
        lb[2 * kEqMaxBands + i] = b.phase[i];
    }
}

__device__ __forceinline__ double eq_ci(double a1, double a2, double f1, double f2, double f) {
    return (a1 - a2) * 0.5 * cos(M_PI * (f - f1) / (f2 - f1)) + (a1 + a2) * 0.5;
}

// the first band i with f <= freq[i + 1], 0 < f < 0.5
__device__ __forceinline__ int eq_band(const double *lb, int n_bands, double f) {
    int lo = 0, hi = n_bands - 2;                          // f < 0.5 = freq[n_bands - 1]: there is one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (f <= lb[mid + 1]) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// X[n], 1 <= n < R/2
template <typename T>
__device__ __forceinline__ c2<T> eq_bin(const double *lb, int n_bands, int n, int R) {
    const double f = (double)n / (double)R;                // exact: R is a power of two
    const int lo = eq_band(lb, n_bands, f);
    const double f1 = lb[lo], f2 = lb[lo + 1];
    const double *mag = lb + kEqMaxBands, *phase = lb + 2 * kEqMaxBands;
    double m = eq_ci(mag[lo], mag[lo + 1], f1, f2, f) / (double)R;
    const double phi = eq_ci(phase[lo], phase[lo + 1], f1, f2, f);
    if (n & 1) m = -m;
    return mk<T>((T)(m * cos(phi)), (T)(m * sin(phi)));
}

// the packed, folded value(s) of bin pair (k, H - k), 0 <= k <= H/2, into s (LDS or global)
template <typename T, typename Arr>
__device__ __forceinline__ void eq_fold(Arr &s, const double *lb, int n_bands, int k, int H, const c2<T> *__restrict__ tw) {
    const int R = 2 * H;
    if (k == 0) {
        const T x0 = (T)(lb[kEqMaxBands] / (double)R), xh = (T)(lb[kEqMaxBands + n_bands - 1] / (double)R);
        s[0] = mk<T>(x0 + xh, x0 - xh);
        return;
    }
    const c2<T> a = eq_bin<T>(lb, n_bands, k, R);
    const c2<T> b = k == H - k ? a : eq_bin<T>(lb, n_bands, H - k, R);
    c2<T> zk, zlk;
    tangle(a, conj(b), tw[k], zk, zlk);
    s[k] = zk;
    if (k != H - k) s[H - k] = zlk;
}

template <typename T, int LOG2H>
__global__ __launch_bounds__(fft_threads<T>(LOG2H)) void
eq_render_lds_kernel(const EqBands b, const c2<T> *__restrict__ tw, c2<T> *__restrict__ taps) {
    constexpr int H = 1 << LOG2H, NT = fft_threads<T>(LOG2H);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsArr<T> s{reinterpret_cast<c2<T> *>(smem)};
    double *lb = reinterpret_cast<double *>(smem + (lds_fft_bytes(LOG2H, sizeof(c2<T>)) + 15) / 16 * 16);
    const int tid = threadIdx.x;
    TwRegs<T, LOG2H, NT> twr;
    twr.prefetch(tw);
    eq_load_bands(lb, b, tid, NT);
    __syncthreads();
    for (int k = tid; k <= H / 2; k += NT) eq_fold<T>(s, lb, b.n, k, H, tw);
    __syncthreads();
    lds_fft<T, LOG2H, NT, true>(s, twr);
    for (int n = tid; n < H; n += NT) taps[n] = s[n];
}
template <int LOG2H> constexpr size_t eq_lds_bytes(size_t elem) {
    return (lds_fft_bytes(LOG2H, elem) + 15) / 16 * 16 + 3 * kEqMaxBands * sizeof(double);
}

// H >= 16384: bins and fold into zin[H], one thread per pair
template <typename T>
__global__ __launch_bounds__(256) void
eq_spectrum_kernel(const EqBands b, c2<T> *__restrict__ zin, const c2<T> *__restrict__ twL, int H) {
    __shared__ double lb[3 * kEqMaxBands];
    eq_load_bands(lb, b, threadIdx.x, 256);
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k <= H / 2) eq_fold<T>(zin, lb, b.n, k, H, twL);
}

// ---- host

// what a convolver with an equaliser reservation owns: the twiddle table of every render length
// up to max_taps, the big-FFT scratch and the buffer the taps are rendered into
struct EqRender {
    int rs = 0;
    long max_taps = 0;
    void *tw[kEqMaxLog2H + 1] = {};    // [log2 H]
    void *zin = nullptr, *zmid = nullptr;
    void *taps = nullptr;              // max_taps reals
};

inline int eq_log2(long v) { int l = 0; while ((1L << l) < v) l++; return l; }

inline hipError_t eq_render_alloc(EqRender &e, int rs, long max_taps) {
    e.rs = rs; e.max_taps = max_taps;
    const int top = eq_log2(max_taps) - 1;
    hipError_t err;
    for (int l = kEqMinLog2H; l <= top; l++) {
        const int nt = l > BIG_LOG2M ? 0 : (rs == 4 ? fft_threads<float>(l) : fft_threads<double>(l));
        const std::vector<unsigned char> t = make_twiddle_table(l, rs, nt);
        if ((err = bfhip_internal_dev_alloc(&e.tw[l], t.size())) != hipSuccess) return err;
        if ((err = hipMemcpy(e.tw[l], t.data(), t.size(), hipMemcpyHostToDevice)) != hipSuccess) return err;
    }
    const size_t bytes = (size_t)max_taps * rs;           // H complex values = R reals
    if (top > BIG_LOG2M) {
        if ((err = bfhip_internal_dev_alloc(&e.zin, bytes)) != hipSuccess) return err;
        if ((err = bfhip_internal_dev_alloc(&e.zmid, bytes)) != hipSuccess) return err;
    }
    if ((err = bfhip_internal_dev_alloc(&e.taps, bytes)) != hipSuccess) return err;
    return hipMemset(e.taps, 0, bytes);
}

inline void eq_render_free(EqRender &e) {
    for (void *&t : e.tw) if (t) { (void)hipFree(t); t = nullptr; }
    void **p[] = {&e.zin, &e.zmid, &e.taps};
    for (void **q : p) if (*q) { (void)hipFree(*q); *q = nullptr; }
}

template <typename T, int LOG2H>
inline hipError_t eq_launch_lds(const EqRender &e, const EqBands &b, hipStream_t st) {
    auto kern = eq_render_lds_kernel<T, LOG2H>;
    const size_t lds = eq_lds_bytes<LOG2H>(sizeof(c2<T>));
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kern, dim3(1), dim3(fft_threads<T>(LOG2H)), lds, st, b, (const c2<T> *)e.tw[LOG2H], (c2<T> *)e.taps);
    return hipGetLastError();
}

// enqueue the render of `taps` reals (a power of two, 8 .. max_taps) into e.taps
template <typename T>
inline hipError_t eq_render_launch(const EqRender &e, const EqBands &b, long taps, hipStream_t st) {
    const int l = eq_log2(taps) - 1;
    switch (l) {
    case 2: return eq_launch_lds<T, 2>(e, b, st);
    case 3: return eq_launch_lds<T, 3>(e, b, st);
    case 4: return eq_launch_lds<T, 4>(e, b, st);
    case 5: return eq_launch_lds<T, 5>(e, b, st);
    case 6: return eq_launch_lds<T, 6>(e, b, st);
    case 7: return eq_launch_lds<T, 7>(e, b, st);
    case 8: return eq_launch_lds<T, 8>(e, b, st);
    case 9: return eq_launch_lds<T, 9>(e, b, st);
    case 10: return eq_launch_lds<T, 10>(e, b, st);
    case 11: return eq_launch_lds<T, 11>(e, b, st);
    case 12: return eq_launch_lds<T, 12>(e, b, st);
    case 13: return eq_launch_lds<T, 13>(e, b, st);
    default: break;
    }
    const int H = 1 << l;
    hipLaunchKernelGGL(eq_spectrum_kernel<T>, dim3((unsigned)(H / 2 / 256 + 1)), dim3(256), 0, st, b, (c2<T> *)e.zin,
                       (const c2<T> *)e.tw[l], H);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    return big_fft_run<T, true>((const c2<T> *)e.zin, (c2<T> *)e.zmid, (c2<T> *)e.taps, l, 1, (const c2<T> *)e.tw[BIG_LOG2M],
                                (const c2<T> *)e.tw[l], st);
}

}  // namespace bfhip
