// eq_minphase.h -- the equaliser curve of eq_render.h rendered with MINIMUM phase: the same
// magnitude, the energy at the first taps, no R/2 frames of delay (bfhip_nupc_render_eq_mode*,
// include/bfhip_nupc.h).  An extension: the reference's render has no such mode.
//
// The homomorphic method, R = taps, H = R/2, ci and the band search those of eq_render.h:
//     M[n]   = ci(mag),  phi[n] = ci(phase)              n = 1 .. H - 1;  M[0] = mag[0], M[H] = mag[last]
//     c      = irfft(log M, R)                           the real cepstrum (normalised inverse)
//     c^[t]  = c[0] | 2 c[t] (1 <= t < H) | c[H] | 0 (t > H)
//     S      = rfft(c^)                                  Re S = log M in exact arithmetic
//     X[k]   = M[k] / R  (cos(Im S[k] + phi[k]) + i sin(Im S[k] + phi[k])),  X[0], X[H] real
//     taps   = unnormalised HC2R of X
// The magnitude is taken from M[k], not from exp(Re S[k]): only Im S is read.  Curve, log, sine and
// cosine are float64 for both precisions; the three transforms run in T; one rounding to T per value
// handed to a transform.
//
// All three real transforms are the packed complex ones of eq_render.h (H points, tangle /
// untangle of kernels.h).  The cepstrum comes out of the first as z[n] = (c[2n], c[2n + 1]), which is
// also the packing the forward transform wants: the window is applied in place.  The forward
// transform is the inverse one on conjugated data (the window conjugates, the untangle step
// conjugates back), so the one-workgroup kernel holds ONE transform, run three times in a loop.
//     H <= 8192   one kernel, one workgroup, the three transforms in the same LDS array
//     H >= 16384  log-and-fold, window, untangle-and-fold kernels with big_fft_run between them; the
//                 one buffer this needs beyond the linear render's is EqMinphase::zc
// No atomics: a render is a pure function of its arguments.
#pragma once
#include "eq_render.h"

namespace bfhip {

// log M of bin pair (k, H - k), scaled by 1 / R for the normalised inverse, folded into s
template <typename T, typename Arr>
__device__ __forceinline__ void eqmin_log_fold(Arr &s, const double *lb, int n_bands, int k, int H, const c2<T> *__restrict__ tw) {
    const int R = 2 * H;
    const double *mag = lb + kEqMaxBands;
    if (k == 0) {
        const T x0 = (T)(log(mag[0]) / (double)R), xh = (T)(log(mag[n_bands - 1]) / (double)R);
        s[0] = mk<T>(x0 + xh, x0 - xh);
        return;
    }
    const double fa = (double)k / (double)R, fb = (double)(H - k) / (double)R;
    const int i = eq_band(lb, n_bands, fa), j = eq_band(lb, n_bands, fb);
    const T a = (T)(log(eq_ci(mag[i], mag[i + 1], lb[i], lb[i + 1], fa)) / (double)R);
    const T b = (T)(log(eq_ci(mag[j], mag[j + 1], lb[j], lb[j + 1], fb)) / (double)R);
    c2<T> zk, zlk;
    tangle(mk<T>(a, (T)0), mk<T>(b, (T)0), tw[k], zk, zlk);
    s[k] = zk;
    if (k != H - k) s[H - k] = zlk;
}

// the cepstral window on packed pair n = (c[2n], c[2n + 1]), 0 <= n < H, conjugated for the
// forward transform that follows
template <typename T>
__device__ __forceinline__ c2<T> eqmin_window(c2<T> c, int n, int H) {
    if (n == 0) return mk<T>(c.x, (T)-2 * c.y);
    if (n < H / 2) return mk<T>((T)2 * c.x, (T)-2 * c.y);
    if (n == H / 2) return mk<T>(c.x, (T)0);
    return mk<T>((T)0, (T)0);
}

// X[n], 1 <= n < R/2, from the minimum phase theta = Im S[n]
template <typename T>
__device__ __forceinline__ c2<T> eqmin_bin(const double *lb, int n_bands, int n, int R, T theta) {
    const double f = (double)n / (double)R;
    const int i = eq_band(lb, n_bands, f);
    const double f1 = lb[i], f2 = lb[i + 1];
    const double *mag = lb + kEqMaxBands, *phase = lb + 2 * kEqMaxBands;
    const double m = eq_ci(mag[i], mag[i + 1], f1, f2, f) / (double)R;
    const double a = (double)theta + eq_ci(phase[i], phase[i + 1], f1, f2, f);
    return mk<T>((T)(m * cos(a)), (T)(m * sin(a)));
}

// bin pair (k, H - k), 0 <= k <= H/2: z holds the conjugate of the forward transform of the windowed
// cepstrum; its untangled S gives the phases, and the folded X goes to s.  z and s may be the same
// array: a pair is read and written by one thread.
template <typename T, typename Src, typename Dst>
__device__ __forceinline__ void eqmin_spectrum_fold(const Src &z, Dst &s, const double *lb, int n_bands, int k, int H,
                                                    const c2<T> *__restrict__ tw) {
    if (k == 0) { eq_fold<T>(s, lb, n_bands, 0, H, tw); return; }     // S[0], S[H] are real: X[0], X[H] as in the linear render
    const c2<T> zk0 = z[k], zl0 = z[H - k];
    c2<T> sk, slk;
    untangle(conj(zk0), zl0, tw[k], sk, slk);
    const int R = 2 * H;
    const c2<T> a = eqmin_bin<T>(lb, n_bands, k, R, sk.y);
    const c2<T> b = k == H - k ? a : eqmin_bin<T>(lb, n_bands, H - k, R, slk.y);
    c2<T> zk, zlk;
    tangle(a, conj(b), tw[k], zk, zlk);
    s[k] = zk;
    if (k != H - k) s[H - k] = zlk;
}

// Registers of the one-workgroup kernel.  The compiler computes the LDS addresses and twiddle
// products of every pass once and keeps them, next to the constants of the float64 log / sine /
// cosine: three inlined transforms needed 196 VGPRs at H = 4096 and spilled at H = 8192.  Hence
//   * one transform in a loop, and eqmin_forget on its twiddles before each run, so that the products
//     (w^3, w^5 ... of every pass) are not hoisted out of the loop;
//   * at most 512 threads, so that a thread may have 256 registers: at 1024 threads (float32,
//     H = 8192: 128 registers) what is left still spilled 104 bytes per lane.  Float32 at H = 8192
//     therefore has a twiddle table of its own, in thread order for 512 threads (EqMinphase::tw512).
template <typename T> constexpr int eqmin_threads(int log2h) { return fft_threads<T>(log2h) > 512 ? 512 : fft_threads<T>(log2h); }

template <typename TW>
__device__ __forceinline__ void eqmin_forget(TW &t) {
    if constexpr (TW::LAZY) asm volatile("" : "+v"(t.g));
    else {
#pragma unroll
        for (int i = 0; i < TW::N; i++) asm volatile("" : "+v"(t.r[i].x), "+v"(t.r[i].y));
    }
}

// LDS as in eq_render_lds_kernel: the padded array of H values, then the bands
template <typename T, int LOG2H>
__global__ __launch_bounds__(eqmin_threads<T>(LOG2H)) void
eq_minphase_lds_kernel(const EqBands b, const c2<T> *__restrict__ tw, c2<T> *__restrict__ taps) {
    constexpr int H = 1 << LOG2H, NT = eqmin_threads<T>(LOG2H);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    LdsArr<T> s{reinterpret_cast<c2<T> *>(smem)};
    double *lb = reinterpret_cast<double *>(smem + (lds_fft_bytes(LOG2H, sizeof(c2<T>)) + 15) / 16 * 16);
    const int tid = threadIdx.x;
    TwRegs<T, LOG2H, NT, (NT < fft_threads<T>(LOG2H))> twr;    // two butterflies per thread: 52 VGPRs of twiddles stay in memory
    twr.prefetch(tw);
    eq_load_bands(lb, b, tid, NT);
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < 3; step++) {
        if (step == 0) {
            for (int k = tid; k <= H / 2; k += NT) eqmin_log_fold<T>(s, lb, b.n, k, H, tw);
        } else if (step == 1) {                           // s: the cepstrum, packed
            for (int n = tid; n < H; n += NT) s[n] = eqmin_window<T>(s[n], n, H);
        } else {
            for (int k = tid; k <= H / 2; k += NT) eqmin_spectrum_fold<T>(s, s, lb, b.n, k, H, tw);
        }
        __syncthreads();
        eqmin_forget(twr);
        lds_fft<T, LOG2H, NT, true>(s, twr);
    }
    for (int n = tid; n < H; n += NT) taps[n] = s[n];
}

// H >= 16384: one thread per bin pair (k <= H/2) or per packed pair (n < H)
template <typename T>
__global__ __launch_bounds__(256) void
eq_minphase_log_kernel(const EqBands b, c2<T> *__restrict__ zin, const c2<T> *__restrict__ twL, int H) {
    __shared__ double lb[3 * kEqMaxBands];
    eq_load_bands(lb, b, threadIdx.x, 256);
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k <= H / 2) eqmin_log_fold<T>(zin, lb, b.n, k, H, twL);
}

template <typename T>
__global__ __launch_bounds__(256) void
eq_minphase_window_kernel(const c2<T> *__restrict__ c, c2<T> *__restrict__ zin, int H) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < H) zin[n] = eqmin_window<T>(c[n], n, H);
}

template <typename T>
__global__ __launch_bounds__(256) void
eq_minphase_spectrum_kernel(const EqBands b, const c2<T> *__restrict__ z, c2<T> *__restrict__ zin,
                            const c2<T> *__restrict__ twL, int H) {
    __shared__ double lb[3 * kEqMaxBands];
    eq_load_bands(lb, b, threadIdx.x, 256);
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k <= H / 2) eqmin_spectrum_fold<T>(z, zin, lb, b.n, k, H, twL);
}

// ---- host

// what bfhip_nupc_reserve_eq_minimum adds to an EqRender: the big-FFT sequence's third buffer
// (cepstrum, then its forward transform; max_taps reals, when max_taps > 16384) and float32's table
// for H = 8192 at 512 threads (when max_taps >= 16384)
struct EqMinphase {
    bool reserved = false;
    void *zc = nullptr;
    void *tw512 = nullptr;
};

inline hipError_t eq_minphase_alloc(EqMinphase &m, const EqRender &e) {
    const int top = eq_log2(e.max_taps) - 1;
    hipError_t err;
    if (top >= BIG_LOG2M && e.rs == 4) {
        const std::vector<unsigned char> t = make_twiddle_table(BIG_LOG2M, 4, eqmin_threads<float>(BIG_LOG2M));
        if ((err = bfhip_internal_dev_alloc(&m.tw512, t.size())) != hipSuccess) return err;
        if ((err = hipMemcpy(m.tw512, t.data(), t.size(), hipMemcpyHostToDevice)) != hipSuccess) return err;
    }
    if (top > BIG_LOG2M && (err = bfhip_internal_dev_alloc(&m.zc, (size_t)e.max_taps * e.rs)) != hipSuccess) return err;
    return hipSuccess;
}

inline void eq_minphase_free(EqMinphase &m) {
    void **p[] = {&m.zc, &m.tw512};
    for (void **q : p) if (*q) { (void)hipFree(*q); *q = nullptr; }
}

template <typename T, int LOG2H>
inline hipError_t eq_minphase_launch_lds(const EqRender &e, const EqMinphase &m, const EqBands &b, hipStream_t st) {
    auto kern = eq_minphase_lds_kernel<T, LOG2H>;
    const size_t lds = eq_lds_bytes<LOG2H>(sizeof(c2<T>));
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return err;
    const void *tw = eqmin_threads<T>(LOG2H) == fft_threads<T>(LOG2H) ? e.tw[LOG2H] : m.tw512;
    hipLaunchKernelGGL(kern, dim3(1), dim3(eqmin_threads<T>(LOG2H)), lds, st, b, (const c2<T> *)tw, (c2<T> *)e.taps);
    return hipGetLastError();
}

// enqueue the minimum-phase render of `taps` reals (a power of two, 8 .. max_taps) into e.taps
template <typename T>
inline hipError_t eq_minphase_launch(const EqRender &e, const EqMinphase &m, const EqBands &b, long taps, hipStream_t st) {
    const int l = eq_log2(taps) - 1;
    switch (l) {
    case 2: return eq_minphase_launch_lds<T, 2>(e, m, b, st);
    case 3: return eq_minphase_launch_lds<T, 3>(e, m, b, st);
    case 4: return eq_minphase_launch_lds<T, 4>(e, m, b, st);
    case 5: return eq_minphase_launch_lds<T, 5>(e, m, b, st);
    case 6: return eq_minphase_launch_lds<T, 6>(e, m, b, st);
    case 7: return eq_minphase_launch_lds<T, 7>(e, m, b, st);
    case 8: return eq_minphase_launch_lds<T, 8>(e, m, b, st);
    case 9: return eq_minphase_launch_lds<T, 9>(e, m, b, st);
    case 10: return eq_minphase_launch_lds<T, 10>(e, m, b, st);
    case 11: return eq_minphase_launch_lds<T, 11>(e, m, b, st);
    case 12: return eq_minphase_launch_lds<T, 12>(e, m, b, st);
    case 13: return eq_minphase_launch_lds<T, 13>(e, m, b, st);
    default: break;
    }
    const int H = 1 << l;
    const dim3 pairs((unsigned)(H / 2 / 256 + 1)), all((unsigned)(H / 256));
    c2<T> *zin = (c2<T> *)e.zin, *zmid = (c2<T> *)e.zmid, *zc = (c2<T> *)m.zc;
    const c2<T> *tw13 = (const c2<T> *)e.tw[BIG_LOG2M], *twL = (const c2<T> *)e.tw[l];
    hipError_t err;
    hipLaunchKernelGGL(eq_minphase_log_kernel<T>, pairs, dim3(256), 0, st, b, zin, twL, H);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if ((err = big_fft_run<T, true>(zin, zmid, zc, l, 1, tw13, twL, st)) != hipSuccess) return err;
    hipLaunchKernelGGL(eq_minphase_window_kernel<T>, all, dim3(256), 0, st, (const c2<T> *)zc, zin, H);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if ((err = big_fft_run<T, true>(zin, zmid, zc, l, 1, tw13, twL, st)) != hipSuccess) return err;
    hipLaunchKernelGGL(eq_minphase_spectrum_kernel<T>, pairs, dim3(256), 0, st, b, (const c2<T> *)zc, zin, twL, H);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    return big_fft_run<T, true>(zin, zmid, (c2<T> *)e.taps, l, 1, tw13, twL, st);
}

}  // namespace bfhip
