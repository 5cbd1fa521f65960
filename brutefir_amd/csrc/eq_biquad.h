// eq_biquad.h -- a cascade of second-order sections rendered into R real taps on the device
// (bfhip_nupc_render_biquads*, include/bfhip_nupc.h): the second curve producer in front of the
// transform of eq_render.h.
//
// Section k is b0, b1, b2, a1, a2 (a0 = 1).  Bin n = 0 .. R/2, s = sin^2(pi n / R), u = sin(2 pi n / R):
//     N_k  = ((b0 + b1) + b2) - 2 (b0 + b2) s + i (b0 - b2) u
//     D_k  = ((1  + a1) + a2) - 2 (1  + a2) s + i (1  - a2) u
//     G[n] = prod_k N_k / D_k                    (k ascending, float64 complex for both precisions)
// which is prod_k H_k(e^{i 2 pi n / R}) with the common factor e^{-i w} cancelled.  The direct
// polynomial b0 + b1 z + b2 z^2 is NOT used: at low frequencies 1 + a1 + a2 is of the order w0^2 and
// the polynomial loses that many digits at every bin; here the small sum is formed once, from the
// coefficients alone.  The host's stability check keeps D_k off zero on the unit circle.
//     phase OWN     X[n] = G[n] / R,             X[0] = Re G[0] / R,  X[R/2] = Re G[R/2] / R
//     phase LINEAR  X[n] = (-1)^n |G[n]| / R,    X[0] = |G[0]| / R,   X[R/2] = |G[R/2]| / R
// X is rounded to T once.  Fold (tangle, the packed DC / Nyquist slot), twiddle tables, lds_fft and
// big_fft_run are the band render's, and the taps land in EqRender::taps, where eq_apply.h and the group
// path read them.  The sections take the LDS region the knots take in eq_render.h (160 doubles against
// 390).  No atomics: a render is a pure function of its arguments.
#pragma once
#include "biquad_host.h"
#include "eq_render.h"

namespace bfhip {

constexpr int kBiquadOwn = 0, kBiquadLinear = 1;       // BFHIP_BIQUAD_OWN, BFHIP_BIQUAD_LINEAR

// the sections in LDS, 5 doubles each (every thread calls)
__device__ __forceinline__ void bq_load(double *lc, const EqBiquads &q, int tid, int nt) {
    for (int i = tid; i < 5 * q.n; i += nt) lc[i] = q.c[i];
}

// G[n], 0 <= n <= R/2
__device__ __forceinline__ double2 bq_response(const double *lc, int n_sections, int n, int R) {
    const double f = (double)n / (double)R;                // exact: R is a power of two
    const double sh = sinpi(f), s = sh * sh, u = sinpi(2.0 * f);
    double gr = 1.0, gi = 0.0;
    for (int k = 0; k < n_sections; k++) {
        const double b0 = lc[5 * k], b1 = lc[5 * k + 1], b2 = lc[5 * k + 2], a1 = lc[5 * k + 3], a2 = lc[5 * k + 4];
        const double nr = ((b0 + b1) + b2) - 2.0 * (b0 + b2) * s, ni = (b0 - b2) * u;
        const double dr = ((1.0 + a1) + a2) - 2.0 * (1.0 + a2) * s, di = (1.0 - a2) * u;
        const double d2 = dr * dr + di * di;
        const double hr = (nr * dr + ni * di) / d2, hi = (ni * dr - nr * di) / d2;
        const double tr = gr * hr - gi * hi;
        gi = gr * hi + gi * hr;
        gr = tr;
    }
    return make_double2(gr, gi);
}

// X[n], 0 <= n <= R/2 (the caller takes the real part at 0 and R/2)
template <typename T>
__device__ __forceinline__ c2<T> bq_bin(const double *lc, int n_sections, int phase, int n, int R) {
    const double2 g = bq_response(lc, n_sections, n, R);
    if (phase == kBiquadOwn) return mk<T>((T)(g.x / (double)R), (T)(g.y / (double)R));
    const double m = hypot(g.x, g.y) / (double)R;
    return mk<T>((T)((n & 1) ? -m : m), (T)0);
}

// the packed, folded value(s) of bin pair (k, H - k), 0 <= k <= H/2, into s (LDS or global): eq_fold's
// layout with this header's bins
template <typename T, typename Arr>
__device__ __forceinline__ void bq_fold(Arr &s, const double *lc, int n_sections, int phase, int k, int H,
                                        const c2<T> *__restrict__ tw) {
    const int R = 2 * H;
    if (k == 0) {
        const T x0 = bq_bin<T>(lc, n_sections, phase, 0, R).x, xh = bq_bin<T>(lc, n_sections, phase, H, R).x;   // H is even
        s[0] = mk<T>(x0 + xh, x0 - xh);
        return;
    }
    const c2<T> a = bq_bin<T>(lc, n_sections, phase, k, R);
    const c2<T> b = k == H - k ? a : bq_bin<T>(lc, n_sections, phase, H - k, R);
    c2<T> zk, zlk;
    tangle(a, conj(b), tw[k], zk, zlk);
    s[k] = zk;
    if (k != H - k) s[H - k] = zlk;
}

template <int LOG2H> constexpr size_t bq_lds_bytes(size_t elem) {
    return (lds_fft_bytes(LOG2H, elem) + 15) / 16 * 16 + 5 * kBiquadMax * sizeof(double);
}

// H <= 8192: one workgroup, sections -> bins -> fold -> lds_fft -> taps
template <typename T, int LOG2H>
__global__ __launch_bounds__(fft_threads<T>(LOG2H)) void
bq_render_lds_kernel(const EqBiquads q, int phase, const c2<T> *__restrict__ tw, c2<T> *__restrict__ taps) {
    constexpr int H = 1 << LOG2H, NT = fft_threads<T>(LOG2H);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsArr<T> s{reinterpret_cast<c2<T> *>(smem)};
    double *lc = reinterpret_cast<double *>(smem + (lds_fft_bytes(LOG2H, sizeof(c2<T>)) + 15) / 16 * 16);
    const int tid = threadIdx.x;
    TwRegs<T, LOG2H, NT> twr;
    twr.prefetch(tw);
    bq_load(lc, q, tid, NT);
    __syncthreads();
    for (int k = tid; k <= H / 2; k += NT) bq_fold<T>(s, lc, q.n, phase, k, H, tw);
    __syncthreads();
    lds_fft<T, LOG2H, NT, true>(s, twr);
    for (int n = tid; n < H; n += NT) taps[n] = s[n];
}

// H >= 16384: bins and fold into zin[H], one thread per pair (k <= H/2 < H: inside zin)
template <typename T>
__global__ __launch_bounds__(256) void
bq_spectrum_kernel(const EqBiquads q, int phase, c2<T> *__restrict__ zin, const c2<T> *__restrict__ twL, int H) {
    __shared__ double lc[5 * kBiquadMax];
    bq_load(lc, q, threadIdx.x, 256);
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k <= H / 2) bq_fold<T>(zin, lc, q.n, phase, k, H, twL);
}

// ---- host

template <typename T, int LOG2H>
inline hipError_t bq_launch_lds(const EqRender &e, const EqBiquads &q, int phase, hipStream_t st) {
    auto kern = bq_render_lds_kernel<T, LOG2H>;
    const size_t lds = bq_lds_bytes<LOG2H>(sizeof(c2<T>));
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kern, dim3(1), dim3(fft_threads<T>(LOG2H)), lds, st, q, phase, (const c2<T> *)e.tw[LOG2H], (c2<T> *)e.taps);
    return hipGetLastError();
}

// enqueue the render of `taps` reals (a power of two, 8 .. max_taps) into e.taps
template <typename T>
inline hipError_t eq_biquad_launch(const EqRender &e, const EqBiquads &q, int phase, long taps, hipStream_t st) {
    const int l = eq_log2(taps) - 1;
    switch (l) {
    case 2: return bq_launch_lds<T, 2>(e, q, phase, st);
    case 3: return bq_launch_lds<T, 3>(e, q, phase, st);
    case 4: return bq_launch_lds<T, 4>(e, q, phase, st);
    case 5: return bq_launch_lds<T, 5>(e, q, phase, st);
    case 6: return bq_launch_lds<T, 6>(e, q, phase, st);
    case 7: return bq_launch_lds<T, 7>(e, q, phase, st);
    case 8: return bq_launch_lds<T, 8>(e, q, phase, st);
    case 9: return bq_launch_lds<T, 9>(e, q, phase, st);
    case 10: return bq_launch_lds<T, 10>(e, q, phase, st);
    case 11: return bq_launch_lds<T, 11>(e, q, phase, st);
    case 12: return bq_launch_lds<T, 12>(e, q, phase, st);
    case 13: return bq_launch_lds<T, 13>(e, q, phase, st);
    default: break;
    }
    const int H = 1 << l;
    hipLaunchKernelGGL(bq_spectrum_kernel<T>, dim3((unsigned)(H / 2 / 256 + 1)), dim3(256), 0, st, q, phase, (c2<T> *)e.zin,
                       (const c2<T> *)e.tw[l], H);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    return big_fft_run<T, true>((const c2<T> *)e.zin, (c2<T> *)e.zmid, (c2<T> *)e.taps, l, 1, (const c2<T> *)e.tw[BIG_LOG2M],
                                (const c2<T> *)e.tw[l], st);
}

}  // namespace bfhip
