// eq_apply.h -- the rendered equaliser taps of eq_render.h / eq_minphase.h convolved onto a base
// impulse response on the device (bfhip_nupc_render_eq_base*, include/bfhip_nupc.h): the idle set
// receives base (*) eq instead of eq.  An extension: the reference cascades two filters instead.
//
// e[0 .. R) are the rendered taps, b[0 .. T) the base, and the result is the convolution truncated at T:
//     y[t] = sum_{j = 0}^{min(t, R - 1)} e[j] b[t - j],   0 <= t < T
// by FFT overlap-save with blocks of B reals, R <= B <= 8192, both powers of two (B = R beyond 8192,
// through bigfft.h: the second half of this file).  Window j of
// ceil(T / B) is the 2B reals b[(j - 1) B, (j + 1) B), zeros in front of tap 0 and behind T; its circular
// convolution with e, zero-padded to 2B, is exact in its last B values, which are y[j B, (j + 1) B).
//
// Both real transforms are the packed complex ones K1 and K3 use (kernels.h: untangle / tangle) with
// H = B points in LDS:
//     eq_apply_spectrum_kernel   one workgroup, once per render: e -> E[0 .. H], scaled by 1 / (2B) (a
//                                power of two: exact); E[0] and E[H] are real and share slot 0
//     eq_apply_kernel            one workgroup per window: load -> lds_fft -> untangle, times E, tangle
//                                -> lds_fft inverse -> the last B reals to y
//     eq_apply_group_kernel      the same window for up to 16 bases under one E, grid (windows, members):
//                                bfhip_nupc_render_eq_group_async
// No atomics and no scratch: y is a pure function of e, b, B and T.  LDS is the padded array alone,
// 139 280 bytes at float64 and B = 8192.
#pragma once
#include <algorithm>

#include "eq_render.h"

namespace bfhip {

constexpr int kEqApplyMaxLog2B = 13;                  // what one workgroup transforms in LDS at float64
constexpr int kEqApplyLog2B = 11;                     // the block length where R leaves the choice open

// B for R taps onto T: max(R, 2048), but no longer than the power of two that holds T in one window.
// A short curve then does not mean hundreds of thousands of 8-point windows, a long schedule has
// hundreds of workgroups to spread over the CUs, and a short schedule is one window.
inline int eq_apply_log2b(long R, long T) { return std::max(eq_log2(R), std::min(kEqApplyLog2B, eq_log2(T))); }

template <typename T, int LOG2H>
__global__ __launch_bounds__(fft_threads<T>(LOG2H)) void
eq_apply_spectrum_kernel(const c2<T> *__restrict__ e, int pairs /* R / 2 <= H / 2 */, const c2<T> *__restrict__ tw,
                         c2<T> *__restrict__ E) {
    constexpr int H = 1 << LOG2H, NT = fft_threads<T>(LOG2H);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsArr<T> s{reinterpret_cast<c2<T> *>(smem)};
    const int tid = threadIdx.x;
    TwRegs<T, LOG2H, NT> twr;
    twr.prefetch(tw);
    for (int n = tid; n < H; n += NT) s[n] = n < pairs ? e[n] : mk<T>((T)0, (T)0);
    __syncthreads();
    lds_fft<T, LOG2H, NT, false>(s, twr);
    const T sc = (T)1 / (T)(2 * H);
    for (int k = tid; k <= H / 2; k += NT) {
        if (k == 0) {
            const c2<T> z = s[0];
            E[0] = mk<T>((z.x + z.y) * sc, (z.x - z.y) * sc);
            continue;
        }
        c2<T> xk, xlk;
        untangle(s[k], conj(s[H - k]), tw[k], xk, xlk);
        E[k] = mk<T>(xk.x * sc, xk.y * sc);
        if (k != H - k) E[H - k] = mk<T>(xlk.x * sc, xlk.y * sc);
    }
}

// B reals b[from, from + B) as packed pairs into s[n0, n0 + B / 2): zeros outside [0, T), 16-byte loads
// where the range is whole (from is a multiple of B >= 8 reals, so it is 16-byte aligned)
template <typename T, int B, int NT>
__device__ __forceinline__ void eq_apply_load(LdsArr<T> s, int n0, const T *__restrict__ b, long from, long Tn, int tid) {
    if (from < 0 || from >= Tn) {
        for (int n = tid; n < B / 2; n += NT) s[n0 + n] = mk<T>((T)0, (T)0);
    } else if (from + B <= Tn) {
        if constexpr (sizeof(T) == 8) {
            const c2<T> *p = reinterpret_cast<const c2<T> *>(b + from);
            for (int n = tid; n < B / 2; n += NT) s[n0 + n] = p[n];
        } else {
            const float4 *p = reinterpret_cast<const float4 *>(b + from);
            for (int m = tid; m < B / 4; m += NT) {
                const float4 v = p[m];
                s[n0 + 2 * m] = mk<T>(v.x, v.y);
                s[n0 + 2 * m + 1] = mk<T>(v.z, v.w);
            }
        }
    } else {
        for (int n = tid; n < B / 2; n += NT) {
            const long i = from + 2 * n;
            s[n0 + n] = mk<T>(i < Tn ? b[i] : (T)0, i + 1 < Tn ? b[i + 1] : (T)0);
        }
    }
}

// one window of one base: y[at, at + B), at = blockIdx.x * B.  The body of both window kernels below, so
// that a member of a group gets the single render's arithmetic operation for operation
template <typename T, int LOG2H>
__device__ __forceinline__ void
eq_apply_window(const T *__restrict__ b, const c2<T> *__restrict__ E, const c2<T> *__restrict__ tw, T *__restrict__ y, long Tn) {
    constexpr int H = 1 << LOG2H, B = H, NT = fft_threads<T>(LOG2H);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsArr<T> s{reinterpret_cast<c2<T> *>(smem)};
    const int tid = threadIdx.x;
    const long at = (long)blockIdx.x * B;                 // y[at, at + B) is this window's
    TwRegs<T, LOG2H, NT> twr;
    twr.prefetch(tw);
    eq_apply_load<T, B, NT>(s, 0, b, at - B, Tn, tid);
    eq_apply_load<T, B, NT>(s, H / 2, b, at, Tn, tid);
    __syncthreads();
    lds_fft<T, LOG2H, NT, false>(s, twr);
    for (int k = tid; k <= H / 2; k += NT) {
        if (k == 0) {                                     // X[0] and X[H] are real, and so are E's
            const c2<T> z = s[0], e0 = E[0];
            const T y0 = (z.x + z.y) * e0.x, yh = (z.x - z.y) * e0.y;
            s[0] = mk<T>(y0 + yh, y0 - yh);
            continue;
        }
        c2<T> xk, xlk, zk, zlk;
        untangle(s[k], conj(s[H - k]), tw[k], xk, xlk);
        const c2<T> pk = cmul(xk, E[k]);
        const c2<T> pl = k == H - k ? pk : cmul(xlk, E[H - k]);
        tangle(pk, conj(pl), tw[k], zk, zlk);
        s[k] = zk;
        if (k != H - k) s[H - k] = zlk;
    }
    __syncthreads();
    lds_fft<T, LOG2H, NT, true>(s, twr);
    // s[n] = (window[2n], window[2n + 1]): the last B reals are pairs H/2 .. H - 1
    if (at + B <= Tn) {
        if constexpr (sizeof(T) == 8) {
            c2<T> *p = reinterpret_cast<c2<T> *>(y + at);
            for (int n = tid; n < B / 2; n += NT) p[n] = s[H / 2 + n];
        } else {
            float4 *p = reinterpret_cast<float4 *>(y + at);
            for (int m = tid; m < B / 4; m += NT) {
                const c2<T> u = s[H / 2 + 2 * m], v = s[H / 2 + 2 * m + 1];
                p[m] = make_float4(u.x, u.y, v.x, v.y);
            }
        }
    } else {
        for (int n = tid; n < B / 2; n += NT) {
            const long i = at + 2 * n;
            const c2<T> v = s[H / 2 + n];
            if (i < Tn) y[i] = v.x;
            if (i + 1 < Tn) y[i + 1] = v.y;
        }
    }
}

template <typename T, int LOG2H>
__global__ __launch_bounds__(fft_threads<T>(LOG2H)) void
eq_apply_kernel(const T *__restrict__ b, const c2<T> *__restrict__ E, const c2<T> *__restrict__ tw, T *__restrict__ y, long Tn) {
    eq_apply_window<T, LOG2H>(b, E, tw, y, Tn);
}

// ---- a group of bases under one curve (bfhip_nupc_render_eq_group_async): grid (ceil(T / B), members),
// member blockIdx.y takes its base and its result from the by-value table (256 bytes of kernel arguments:
// no upload), E is the one spectrum of the call.  LDS is the padded array alone here too.
constexpr int kEqGroupMax = 16;                       // BFHIP_NUPC_GROUP_MAX
struct EqApplyGroup {
    const void *b[kEqGroupMax];
    void *y[kEqGroupMax];
};

template <typename T, int LOG2H>
__global__ __launch_bounds__(fft_threads<T>(LOG2H)) void
eq_apply_group_kernel(const EqApplyGroup g, const c2<T> *__restrict__ E, const c2<T> *__restrict__ tw, long Tn) {
    const int m = blockIdx.y;                             // < members <= kEqGroupMax: the grid's height
    eq_apply_window<T, LOG2H>(static_cast<const T *>(g.b[m]), E, tw, static_cast<T *>(g.y[m]), Tn);
}

// ---- R > 8192 (bfhip_nupc_reserve_eq_base_long): B = R, and a window's H = B points do not fit a
// workgroup's LDS.  The same overlap-save with the transforms of bigfft.h over global scratch, all n_win =
// ceil(T / B) windows as one batch, and the curve as transform n_win of the forward batch:
//     eq_apply_gather_kernel     z[w][n] = (b[(w - 1) B + 2n], b[(w - 1) B + 2n + 1]), zeros outside [0, T);
//                                z[n_win][n] = (e[2n], e[2n + 1]), zeros from R / 2 on
//     big_fft_run forward        n_win + 1 transforms of H points
//     big_untangle               transform n_win -> E[0 .. H], scaled by 1 / (2B), E[0] and E[H] in slot 0
//     eq_apply_product_kernel    (w, k <= H / 2): eq_apply_kernel's untangle, times E, tangle
//     big_fft_run inverse        n_win transforms
//     eq_apply_store_kernel      the last B reals of window w to y[w B, (w + 1) B), clipped at T
// No atomics here either.  The three buffers that big_fft_run alternates between hold (n_win + 1) B complex
// values each: T + max_taps where B divides T, below T + 2 max_taps otherwise.

template <typename T>
__global__ __launch_bounds__(256) void
eq_apply_gather_kernel(const T *__restrict__ b, const c2<T> *__restrict__ e, int pairs /* R / 2 */, c2<T> *__restrict__ z,
                       int log2b, int n_win, long Tn) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;  // < B: the grid is B / 256 wide
    const int w = blockIdx.y;
    c2<T> v;
    if (w == n_win) {
        v = n < pairs ? e[n] : mk<T>((T)0, (T)0);
    } else {
        const long i = ((long)(w - 1) << log2b) + 2 * n;   // even: in front of tap 0 both of a pair lie, or neither
        if (i >= 0 && i + 1 < Tn) v = *reinterpret_cast<const c2<T> *>(b + i);
        else v = mk<T>(i >= 0 && i < Tn ? b[i] : (T)0, (T)0);
    }
    z[((size_t)w << log2b) + n] = v;
}

template <typename T>
__global__ __launch_bounds__(256) void
eq_apply_product_kernel(const c2<T> *__restrict__ x, const c2<T> *__restrict__ E, const c2<T> *__restrict__ tw,
                        c2<T> *__restrict__ z, int H) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > H / 2) return;
    const c2<T> *s = x + (size_t)blockIdx.y * H;
    c2<T> *d = z + (size_t)blockIdx.y * H;
    if (k == 0) {                                         // X[0] and X[H] are real, and so are E's
        const c2<T> z0 = s[0], e0 = E[0];
        const T y0 = (z0.x + z0.y) * e0.x, yh = (z0.x - z0.y) * e0.y;
        d[0] = mk<T>(y0 + yh, y0 - yh);
        return;
    }
    c2<T> xk, xlk, zk, zlk;
    untangle(s[k], conj(s[H - k]), tw[k], xk, xlk);
    const c2<T> pk = cmul(xk, E[k]);
    const c2<T> pl = k == H - k ? pk : cmul(xlk, E[H - k]);
    tangle(pk, conj(pl), tw[k], zk, zlk);
    d[k] = zk;
    if (k != H - k) d[H - k] = zlk;
}

template <typename T>
__global__ __launch_bounds__(256) void
eq_apply_store_kernel(const c2<T> *__restrict__ z, T *__restrict__ y, int log2b, long Tn) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;  // < B / 2: the grid is B / 512 wide
    const long B = 1L << log2b, at = (long)blockIdx.y << log2b;
    // z[w][n] = (window[2n], window[2n + 1]): the last B reals are pairs B/2 .. B - 1
    const c2<T> v = z[(size_t)at + B / 2 + n];
    const long i = at + 2 * n;
    if (i + 1 < Tn) *reinterpret_cast<c2<T> *>(y + i) = v;
    else if (i < Tn) y[i] = v.x;
}

// ---- host

// what bfhip_nupc_reserve_eq_base adds to an EqRender: a base per reserved filter, the result, the
// curve's spectrum and the twiddle tables of the block lengths the render's own lengths do not cover;
// and what bfhip_nupc_reserve_eq_base_long adds to that where max_taps > 8192
struct EqApply {
    bool reserved = false;
    bool reserved_long = false;                // bfhip_nupc_reserve_eq_base_long
    long T = 0;
    std::vector<void *> base;                  // [filter]: T reals, nullptr without a reservation
    void *y = nullptr;                         // T reals: the device source of the rewrite
    void *ys[kEqGroupMax] = {};                // [slot]: ys[0] = y; 1 .. max_members - 1 under bfhip_nupc_reserve_eq_group
    void *spec = nullptr;                      // B_max complex values, B_max <= 8192
    const void *tw[kEqMaxLog2H + 2] = {};      // [log2 B]: the render's table, or one of `own`
    void *own[kEqMaxLog2H + 2] = {};
    void *big[3] = {};                         // R > 8192: (n_win + 1) B complex values each, the largest over B
    void *big_spec = nullptr;                  // max_taps complex values
};

// R > 8192: the complex values each of the three buffers holds, the largest over the lengths B
inline size_t eq_apply_big_elems(long T, long max_taps) {
    size_t most = 0;
    for (long B = 2L << kEqApplyMaxLog2B; B <= max_taps; B *= 2) most = std::max(most, (size_t)((T + B - 1) / B + 1) * (size_t)B);
    return most;
}

inline hipError_t eq_apply_alloc(EqApply &a, const EqRender &e, long T, const std::vector<char> &want) {
    a.T = T;
    hipError_t err;
    const size_t bytes = (size_t)T * e.rs;
    a.base.assign(want.size(), nullptr);
    for (size_t f = 0; f < want.size(); f++) {
        if (!want[f]) continue;
        if ((err = bfhip_internal_dev_alloc(&a.base[f], bytes)) != hipSuccess) return err;
        if ((err = hipMemset(a.base[f], 0, bytes)) != hipSuccess) return err;
    }
    if ((err = bfhip_internal_dev_alloc(&a.y, bytes)) != hipSuccess) return err;
    if ((err = hipMemset(a.y, 0, bytes)) != hipSuccess) return err;
    a.ys[0] = a.y;
    const int lo = eq_apply_log2b(8, T), hi = eq_apply_log2b(std::min(e.max_taps, 1L << kEqApplyMaxLog2B), T);
    if ((err = bfhip_internal_dev_alloc(&a.spec, ((size_t)2 << hi) * e.rs)) != hipSuccess) return err;
    for (int l = lo; l <= hi; l++) {
        if (e.tw[l]) { a.tw[l] = e.tw[l]; continue; }
        const std::vector<unsigned char> t = make_twiddle_table(l, e.rs, e.rs == 4 ? fft_threads<float>(l) : fft_threads<double>(l));
        if ((err = bfhip_internal_dev_alloc(&a.own[l], t.size())) != hipSuccess) return err;
        if ((err = hipMemcpy(a.own[l], t.data(), t.size(), hipMemcpyHostToDevice)) != hipSuccess) return err;
        a.tw[l] = a.own[l];
    }
    if (!a.reserved_long || e.max_taps <= (1L << kEqApplyMaxLog2B)) return hipSuccess;
    // the tables of H = 16384 .. max_taps points: the render's own stop at max_taps / 2
    for (int l = kEqApplyMaxLog2B + 1; l <= eq_log2(e.max_taps); l++) {
        if (l <= kEqMaxLog2H && e.tw[l]) { a.tw[l] = e.tw[l]; continue; }   // e.tw stops at kEqMaxLog2H
        const std::vector<unsigned char> t = make_twiddle_table(l, e.rs, 0);
        if ((err = bfhip_internal_dev_alloc(&a.own[l], t.size())) != hipSuccess) return err;
        if ((err = hipMemcpy(a.own[l], t.data(), t.size(), hipMemcpyHostToDevice)) != hipSuccess) return err;
        a.tw[l] = a.own[l];
    }
    for (void *&p : a.big)
        if ((err = bfhip_internal_dev_alloc(&p, eq_apply_big_elems(T, e.max_taps) * 2 * e.rs)) != hipSuccess) return err;
    return bfhip_internal_dev_alloc(&a.big_spec, (size_t)e.max_taps * 2 * e.rs);
}

// what bfhip_nupc_reserve_eq_group adds: one more result of T reals per member beyond the first
inline hipError_t eq_apply_group_alloc(EqApply &a, const EqRender &e, int max_members) {
    hipError_t err;
    const size_t bytes = (size_t)a.T * e.rs;
    for (int m = 1; m < max_members; m++) {
        if ((err = bfhip_internal_dev_alloc(&a.ys[m], bytes)) != hipSuccess) return err;
        if ((err = hipMemset(a.ys[m], 0, bytes)) != hipSuccess) return err;
    }
    return hipSuccess;
}

inline void eq_apply_free(EqApply &a) {
    for (int m = 1; m < kEqGroupMax; m++) if (a.ys[m]) { (void)hipFree(a.ys[m]); a.ys[m] = nullptr; }
    a.ys[0] = nullptr;
    for (void *&p : a.base) if (p) { (void)hipFree(p); p = nullptr; }
    for (void *&p : a.own) if (p) { (void)hipFree(p); p = nullptr; }
    void **p[] = {&a.y, &a.spec, &a.big[0], &a.big[1], &a.big[2], &a.big_spec};
    for (void **q : p) if (*q) { (void)hipFree(*q); *q = nullptr; }
}

// n members: base[i] (*) e.taps[0 .. R) into y[i].  One member is the single render's two launches; more
// are the spectrum once and one batched launch
template <typename T, int LOG2H>
inline hipError_t eq_apply_launch_lds(const EqApply &a, const EqRender &e, int n, const void *const base[], void *const y[], long R,
                                      hipStream_t st) {
    auto spec = eq_apply_spectrum_kernel<T, LOG2H>;
    auto kern = eq_apply_kernel<T, LOG2H>;
    auto group = eq_apply_group_kernel<T, LOG2H>;
    const size_t lds = lds_fft_bytes(LOG2H, sizeof(c2<T>));
    hipError_t err;
    if ((err = hipFuncSetAttribute(reinterpret_cast<const void *>(spec), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return err;
    if (n == 1 && (err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return err;
    if (n > 1 && (err = hipFuncSetAttribute(reinterpret_cast<const void *>(group), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) return err;
    const dim3 nt(fft_threads<T>(LOG2H));
    const c2<T> *tw = (const c2<T> *)a.tw[LOG2H];
    hipLaunchKernelGGL(spec, dim3(1), nt, lds, st, (const c2<T> *)e.taps, (int)(R / 2), tw, (c2<T> *)a.spec);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    const long B = 1L << LOG2H;
    const unsigned n_win = (unsigned)((a.T + B - 1) / B);
    if (n == 1) {
        hipLaunchKernelGGL(kern, dim3(n_win), nt, lds, st, (const T *)base[0], (const c2<T> *)a.spec, tw, (T *)y[0], a.T);
        return hipGetLastError();
    }
    EqApplyGroup g = {};
    for (int i = 0; i < n; i++) { g.b[i] = base[i]; g.y[i] = y[i]; }
    hipLaunchKernelGGL(group, dim3(n_win, (unsigned)n), nt, lds, st, g, (const c2<T> *)a.spec, tw, a.T);
    return hipGetLastError();
}

// R > 8192: the windows through bigfft.h (needs what eq_apply_alloc adds under reserved_long)
template <typename T>
inline hipError_t eq_apply_launch_big(const EqApply &a, const EqRender &e, const void *base, void *y, long R, hipStream_t st) {
    const int l = eq_apply_log2b(R, a.T);
    const long B = 1L << l;
    const int H = (int)B, n_win = (int)((a.T + B - 1) / B);
    if (!a.big[0] || !a.tw[l] || (size_t)(n_win + 1) * (size_t)B > eq_apply_big_elems(a.T, e.max_taps)) return hipErrorInvalidValue;
    c2<T> *z0 = (c2<T> *)a.big[0], *z1 = (c2<T> *)a.big[1], *z2 = (c2<T> *)a.big[2], *E = (c2<T> *)a.big_spec;
    const c2<T> *tw13 = (const c2<T> *)e.tw[BIG_LOG2M], *twL = (const c2<T> *)a.tw[l];
    hipError_t err;
    hipLaunchKernelGGL(eq_apply_gather_kernel<T>, dim3((unsigned)(B / 256), (unsigned)(n_win + 1)), dim3(256), 0, st,
                       (const T *)base, (const c2<T> *)e.taps, (int)(R / 2), z0, l, n_win, a.T);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if ((err = big_fft_run<T, false>(z0, z1, z2, l, n_win + 1, tw13, twL, st)) != hipSuccess) return err;
    hipLaunchKernelGGL(big_untangle<T>, dim3((unsigned)(H / 2 / 256 + 1), 1), dim3(256), 0, st, z2 + (size_t)n_win * B, E, (size_t)0,
                       twL, H, (T)1 / (T)(2 * B));
    hipLaunchKernelGGL(eq_apply_product_kernel<T>, dim3((unsigned)(H / 2 / 256 + 1), (unsigned)n_win), dim3(256), 0, st,
                       (const c2<T> *)z2, (const c2<T> *)E, twL, z0, H);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if ((err = big_fft_run<T, true>(z0, z1, z2, l, n_win, tw13, twL, st)) != hipSuccess) return err;
    hipLaunchKernelGGL(eq_apply_store_kernel<T>, dim3((unsigned)(B / 512), (unsigned)n_win), dim3(256), 0, st, (const c2<T> *)z2,
                       (T *)y, l, a.T);
    return hipGetLastError();
}

// enqueue y[i] = base[i] (*) e.taps[0 .. R), truncated at T, for n members (R: a power of two, 8 .. max_taps,
// rendered into e.taps on the same stream before; above 8192 under reserved_long only, and there the members
// go through the three big buffers one after another, each with the single render's launches: the curve is
// member n_win of every member's forward batch again)
template <typename T>
inline hipError_t eq_apply_launch(const EqApply &a, const EqRender &e, int n, const void *const base[], void *const y[], long R,
                                  hipStream_t st) {
    if (n < 1 || n > kEqGroupMax) return hipErrorInvalidValue;
    if (R > (1L << kEqApplyMaxLog2B)) {
        for (int i = 0; i < n; i++) {
            const hipError_t err = eq_apply_launch_big<T>(a, e, base[i], y[i], R, st);
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    }
    switch (eq_apply_log2b(R, a.T)) {
    case 3: return eq_apply_launch_lds<T, 3>(a, e, n, base, y, R, st);
    case 4: return eq_apply_launch_lds<T, 4>(a, e, n, base, y, R, st);
    case 5: return eq_apply_launch_lds<T, 5>(a, e, n, base, y, R, st);
    case 6: return eq_apply_launch_lds<T, 6>(a, e, n, base, y, R, st);
    case 7: return eq_apply_launch_lds<T, 7>(a, e, n, base, y, R, st);
    case 8: return eq_apply_launch_lds<T, 8>(a, e, n, base, y, R, st);
    case 9: return eq_apply_launch_lds<T, 9>(a, e, n, base, y, R, st);
    case 10: return eq_apply_launch_lds<T, 10>(a, e, n, base, y, R, st);
    case 11: return eq_apply_launch_lds<T, 11>(a, e, n, base, y, R, st);
    case 12: return eq_apply_launch_lds<T, 12>(a, e, n, base, y, R, st);
    case 13: return eq_apply_launch_lds<T, 13>(a, e, n, base, y, R, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace bfhip
