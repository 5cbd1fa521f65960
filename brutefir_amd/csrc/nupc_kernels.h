// nupc_kernels.h -- every kernel of the non-uniform convolver, its device helpers, and the host wrappers
// that launch them: accumulate (plain and fading), the delay / mute step, the input conversion with
// sub-delay, and the emit step (plain and dithering).  Included by nupc.hip only: the kernels live in an
// anonymous namespace.  The host decides (nupc_sched.h); nothing here does.
#pragma once
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "nupc.h"

namespace {

// acc[(pos + j) mod A][o] += seg[j][o] for an L_k x n_out block of a segment's output; during a
// coefficient switch a block that ran under both assignments adds its second output (seg2) into
// the other ring (acc2) in the same pass
template <typename T>
__global__ __launch_bounds__(256) void
nupc_accumulate_kernel(T *__restrict__ acc, const T *__restrict__ seg, T *__restrict__ acc2,
                       const T *__restrict__ seg2, unsigned long long pos, int A, int n_out, int n_frames) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_frames * n_out) return;
    const size_t j = i / n_out, o = i % n_out;
    const size_t cell = (size_t)((pos + j) % (unsigned long long)A) * n_out + o;
    acc[cell] += seg[i];
    if (acc2) acc2[cell] += seg2[i];
}

// a staggered switch (BFHIP_NUPC_SWITCH_STAGGERED): segment k fades at its own switch frame t_k, so
// the blend happens here, per segment block, and not in the emit step.  A block that ran under both
// assignments adds  (1 - w) seg + w seg2  into the live ring, w the weight emit_take gives frame
// rel = pos + j - t_k: 0 below the switch frame, rel / (F - 1) on the ramp, 1 from F on.  One thread
// per [frame][out] cell, adjacent threads on adjacent cells of all three arrays.
template <typename T>
__global__ __launch_bounds__(256) void
nupc_accumulate_fade_kernel(T *__restrict__ acc, const T *__restrict__ seg, const T *__restrict__ seg2,
                            unsigned long long pos, int A, int n_out, int n_frames, long long rel0, int F) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_frames * n_out) return;
    const size_t j = i / n_out, o = i % n_out;
    const size_t cell = (size_t)((pos + j) % (unsigned long long)A) * n_out + o;
    const long long rel = rel0 + (long long)j;
    T y = seg[i];
    if (rel >= F) y = seg2[i];
    else if (rel >= 0) {
        const T w = (T)((double)rel / (double)(F - 1));
        y = ((T)1 - w) * y + w * seg2[i];
    }
    acc[cell] += y;
}

// frame n of output block b out of the ring(s), its cells cleared.  Outside a coefficient switch
// (acc_new == nullptr) only the live ring is read.  Inside one, acc_old holds the old assignment's
// output and acc_new the new one's; frame t of the block (rel = t - t_sw) is old before the switch
// frame, new from t_sw + F on, and the linear ramp (1 - w) old + w new, w = rel / (F - 1), in
// between.
template <typename T>
__device__ __forceinline__ T emit_take(T *__restrict__ acc_old, T *__restrict__ acc_new, unsigned long long pos,
                                       int A, int n_out, int ch, int n, long long rel0, int F) {
    const size_t c = (size_t)((pos + n) % (unsigned long long)A) * n_out + ch;
    T y = acc_old[c];
    acc_old[c] = (T)0;
    if (acc_new) {
        const T y_new = acc_new[c];
        acc_new[c] = (T)0;
        const long long rel = rel0 + n;
        if (rel >= F) y = y_new;
        else if (rel >= 0) {
            const T w = (T)((double)rel / (double)(F - 1));
            y = ((T)1 - w) * y + w * y_new;
        }
    }
    return y;
}

// thread 0 of every emit workgroup, after its channel's status bits are in *status: the last
// channel to finish hands the status bits of all segments (they OR into the same word) to the
// host's pinned word: no device-to-host copy after the sync
__device__ __forceinline__ void emit_hand_off(int *__restrict__ status, unsigned int *__restrict__ arrive,
                                              int *__restrict__ host_status) {
    __threadfence();
    if (atomicAdd(arrive, 1u) + 1u == gridDim.x) {
        *arrive = 0;
        const int all_bits = atomicExch(status, 0);
        if (all_bits) *host_status = *host_status | all_bits;
        __threadfence_system();
    }
}

// ---- per-output factor: 1/scale of the format times the output gain, which may be on a ramp
// (the record, NupcGain, and the host's mirror of it are in nupc_sched.h)
// what a thread of the emit step keeps of its channel's record for one period: at(n) is the factor
// of the period's frame n, a pure function of n
template <typename T> struct GainFactor {
    T sc;                          // off the ramp
    double inv, a, d, len;
    int done, on;                  // frames n < on of this period are on the ramp
    __device__ __forceinline__ void load(const NupcGain &r, int L0) {
        sc = (T)(r.inv * r.g);
        inv = r.inv; a = r.a; d = r.g - r.a; len = (double)r.len; done = r.done;
        const int left = r.len - 1 - r.done;
        on = left < 0 ? 0 : left < L0 ? left : L0;
    }
    __device__ __forceinline__ T at(int n) const {
        if (n >= on) return sc;
        return (T)(inv * (a + d * ((double)(done + n + 1) / len)));
    }
};
// thread 0, after every thread of the workgroup has loaded the record: the period has been emitted
__device__ __forceinline__ void gain_advance(NupcGain *__restrict__ r, int L0) {
    const int done = r->done, len = r->len;
    if (done < len) r->done = len - done < L0 ? len : done + L0;
}

// ---- per-channel sub-sample delay (subdelay: / sdf_length; delay.c:416-442 at a period of L0)
//
// What the reference computes per period is the causal FIR  y[t] = sum_k h[k] x[t - k]  over the
// channel's stream, h one of the 199 filters of the bank (subdelay_filter.h) and the last `bs`
// unfiltered samples carried from period to period.  This period's value of every channel of a
// side travels in the kernel arguments (-100: the channel has no filter), so a change needs no
// host wait and reaches the device with the block call it was made before.
constexpr int kSdChannels = 256;   // channels per side when the side uses sub-delay (BF_MAXCHANNELS)
constexpr int kSdTile = 2048;      // frames filtered per pass through LDS
constexpr int kSdMaxBs = 1024;     // largest filter block size: 4 history samples per thread
struct NupcSdVals { signed char v[kSdChannels]; };
template <typename T> struct NupcSd {
    const T *bank;                 // [199][flen] taps, index 99 + value
    T *hist;                       // [channels of the side][bs]: the last bs unfiltered samples
    int bs, flen, tile;            // tile = min(L0, kSdTile); bs <= tile, both powers of two
    NupcSdVals vals;
};
static size_t nupc_sd_lds(int bs, int flen, int tile, int rs) { return (size_t)(bs + tile + flen) * rs; }

// One channel's period, by its whole workgroup (256 threads, every thread calls): src(n) is the
// unfiltered sample of frame n, each asked for once and in order of the tiles; sink(n, y) takes
// the filtered one.  LDS: xx[bs + tile] = [history | tile], hh[flen] the taps, so no tap and no
// sample is read from global memory more than once.  L0 above the tile is filtered tile by tile
// with the history moved down in between.
template <typename T, typename Src, typename Sink>
__device__ __forceinline__ void
sd_fir_period(unsigned char *smem, const NupcSd<T> &sd, int ch, int L0, Src src, Sink sink) {
    const int tid = threadIdx.x, bs = sd.bs, flen = sd.flen, tile = sd.tile;
    T *xx = reinterpret_cast<T *>(smem), *hh = xx + bs + tile;
    const T *taps = sd.bank + (size_t)(99 + sd.vals.v[ch]) * flen;
    T *hist = sd.hist + (size_t)ch * bs;
    for (int k = tid; k < flen; k += 256) hh[k] = taps[k];
    for (int n = tid; n < bs; n += 256) xx[n] = hist[n];
    for (int t0 = 0; t0 < L0; t0 += tile) {
        for (int n = tid; n < tile; n += 256) xx[bs + n] = src(t0 + n);
        __syncthreads();
        for (int n = tid; n < tile; n += 256) {
            T acc = (T)0;
            for (int k = 0; k < flen; k++) acc += hh[k] * xx[bs + n - k];      // flen <= bs: index >= 1
            sink(t0 + n, acc);
        }
        T keep[kSdMaxBs / 256];
#pragma unroll
        for (int i = 0; i < kSdMaxBs / 256; i++) { const int n = tid + i * 256; if (n < bs) keep[i] = xx[tile + n]; }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kSdMaxBs / 256; i++) { const int n = tid + i * 256; if (n < bs) xx[n] = keep[i]; }
    }
    for (int n = tid; n < bs; n += 256) hist[n] = xx[n];          // each thread's own writes: no barrier
}

// Input side, one launch per period behind the delay / mute step: one workgroup per input channel
// converts the period's L0 raw samples with load_raw -- the conversion the engines' input transform
// uses -- into the ring of reals the segment engines read ([frame][n_in], interleaved), through the
// FIR for a channel that has a filter.  Each channel has its own format, offset and stride in `raw`
// (a frame slot of the raw ring, or the staged period buffer of a side with planes or several
// devices); adjacent threads take adjacent samples, so a contiguous plane is read coalesced.
template <typename T>
__global__ __launch_bounds__(256) void
nupc_subdelay_in_kernel(const uint8_t *__restrict__ raw, const DevFormat *__restrict__ fmt, T *__restrict__ real,
                        int n_in, int L0, const NupcSd<T> sd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sd_smem[];
    const int ch = blockIdx.x;
    const DevFormat f = fmt[ch];
    const uint8_t *base = raw + f.byte_offset;
    const size_t stride = (size_t)f.sample_spacing * f.bytes;
    if (sd.vals.v[ch] == -100) {
        for (int n = threadIdx.x; n < L0; n += 256) real[(size_t)n * n_in + ch] = load_raw<T>(base + (size_t)n * stride, f);
        return;
    }
    sd_fir_period<T>(sd_smem, sd, ch, L0, [&](int n) { return load_raw<T>(base + (size_t)n * stride, f); },
                     [&](int n, T y) { real[(size_t)n * n_in + ch] = y; });
}

// output block b: L_0 frames out of the ring (emit_take), scaled into output units (1/scale times
// the output gain of the frame, GainFactor), requantised like convolver_cbuf2raw (real2raw.h / dither_funs.h:71-114),
// ring region cleared.  One workgroup per output channel.  SD: the output side uses sub-delay; a
// channel that has a filter runs the FIR over the scaled reals -- the values it would have been
// quantised from -- and quantises the result (sd_fir_period); the others take the plain path.
template <typename T, bool SD>
__global__ __launch_bounds__(256) void
nupc_emit_kernel(T *__restrict__ acc_old, T *__restrict__ acc_new, unsigned long long pos, int A, int n_out, int L0,
                 long long rel0, int F, const DevFormat *__restrict__ fmt, NupcGain *__restrict__ gain,
                 DevOverflow *__restrict__ over, uint8_t *__restrict__ raw, double safety_limit,
                 int *__restrict__ status, unsigned int *__restrict__ arrive, int *__restrict__ host_status,
                 const NupcSd<T> sd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sd_smem[];
    const int ch = blockIdx.x, tid = threadIdx.x;
    const DevFormat f = fmt[ch];
    DevOverflow of = over[ch];
    uint8_t *base = raw + f.byte_offset;
    const size_t stride = (size_t)f.sample_spacing * f.bytes;
    GainFactor<T> sc;
    sc.load(gain[ch], L0);
    Quantiser<T> qz;
    qz.init(f, of, safety_limit);
    if (SD && sd.vals.v[ch] != -100)
        sd_fir_period<T>(sd_smem, sd, ch, L0,
                         [&](int n) { return emit_take(acc_old, acc_new, pos, A, n_out, ch, n, rel0, F) * sc.at(n); },
                         [&](int n, T y) { qz.put(y, base + (size_t)n * stride); });
    else
        for (int n = tid; n < L0; n += 256)
            qz.put(emit_take(acc_old, acc_new, pos, A, n_out, ch, n, rel0, F) * sc.at(n), base + (size_t)n * stride);
    qz.reduce(tid, 256);
    if (tid == 0) {
        qz.commit(of);
        over[ch] = of;
        gain_advance(gain + ch, L0);
        if (qz.st) atomicOr(status, qz.st);
        emit_hand_off(status, arrive, host_status);
    }
}

// the emit step of a convolver with dithered outputs (launched instead of nupc_emit_kernel, same
// grid).  A channel without a dither slot (slot[ch] < 0) is requantised exactly as there.  A
// dithered one stages its L_0 blended, scaled reals -- the very values nupc_emit_kernel would
// hand to the quantiser, behind the sub-delay FIR if the channel has a filter -- in
// stage[slot][L0], and wave 0 runs the HP-TPDF chain over them (dither_chain, kernels.h: the
// uniform engine's dither pass).  The chain ORs its status bits in before thread 0 takes part in
// the hand-off, so they reach the host with this block's call.
template <typename T, bool SD>
__global__ __launch_bounds__(256) void
nupc_emit_dither_kernel(T *__restrict__ acc_old, T *__restrict__ acc_new, unsigned long long pos, int A, int n_out,
                        int L0, long long rel0, int F, const DevFormat *__restrict__ fmt,
                        NupcGain *__restrict__ gain, DevOverflow *__restrict__ over, uint8_t *__restrict__ raw,
                        double safety_limit, int *__restrict__ status, unsigned int *__restrict__ arrive,
                        int *__restrict__ host_status, const int *__restrict__ dslot, T *__restrict__ stage,
                        DitherState<T> *__restrict__ dstate, const int8_t *__restrict__ table, int table_size,
                        const T *__restrict__ randmap /* index -256..255 (centre pointer) */, const NupcSd<T> sd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sd_smem[];
    __shared__ T rmap[512];
    const int ch = blockIdx.x, tid = threadIdx.x;
    const int slot = dslot[ch];
    const DevFormat f = fmt[ch];
    GainFactor<T> sc;
    sc.load(gain[ch], L0);
    const bool fir = SD && sd.vals.v[ch] != -100;
    if (slot < 0) {
        DevOverflow of = over[ch];
        uint8_t *base = raw + f.byte_offset;
        const size_t stride = (size_t)f.sample_spacing * f.bytes;
        Quantiser<T> qz;
        qz.init(f, of, safety_limit);
        if (fir)
            sd_fir_period<T>(sd_smem, sd, ch, L0,
                             [&](int n) { return emit_take(acc_old, acc_new, pos, A, n_out, ch, n, rel0, F) * sc.at(n); },
                             [&](int n, T y) { qz.put(y, base + (size_t)n * stride); });
        else
            for (int n = tid; n < L0; n += 256)
                qz.put(emit_take(acc_old, acc_new, pos, A, n_out, ch, n, rel0, F) * sc.at(n), base + (size_t)n * stride);
        qz.reduce(tid, 256);
        if (tid == 0) {
            qz.commit(of);
            over[ch] = of;
            gain_advance(gain + ch, L0);
            if (qz.st) atomicOr(status, qz.st);
            emit_hand_off(status, arrive, host_status);
        }
        return;
    }
    T *x = stage + (size_t)slot * L0;
    if (fir)
        sd_fir_period<T>(sd_smem, sd, ch, L0,
                         [&](int n) { return emit_take(acc_old, acc_new, pos, A, n_out, ch, n, rel0, F) * sc.at(n); },
                         [&](int n, T y) { x[n] = y; });
    else
        for (int n = tid; n < L0; n += 256) x[n] = emit_take(acc_old, acc_new, pos, A, n_out, ch, n, rel0, F) * sc.at(n);
    for (int i = tid; i < 512; i += 256) rmap[i] = randmap[i - 256];
    __syncthreads();                  // the staged samples are visible to wave 0 (same workgroup)
    if (tid < 64) {
        dither_chain<T>(x, dstate + slot, table, table_size, rmap, f, over + ch, raw, L0, safety_limit, status, tid);
        if (tid == 0) {
            gain_advance(gain + ch, L0);               // behind the barrier: every thread has its copy
            emit_hand_off(status, arrive, host_status);
        }
    }
}

// ---- look-ahead peak limiter (bfhip_nupc_enable_limiter; the definition is in include/bfhip_nupc.h and,
// frame by frame, in limiter_host.h).  A convolver with a limiter launches these two kernels instead of
// one of the emit kernels above, on the same grid: one workgroup per output channel.
constexpr int kLimTile = 1024;     // frames of envelope per pass through LDS
// LDS of the limit kernel: three float64 arrays [D + tile], D the envelope's look-ahead
static size_t nupc_lim_lds(int D, int tile) { return (size_t)3 * (D + tile) * sizeof(double); }
// and, under true-peak detection, the staging window of one member: the tile and the 2 H - 1 frames before it
static size_t nupc_lim_tp_lds(int De, int tile) { return nupc_lim_lds(De, tile) + (size_t)(tile + kTpTaps - 1) * sizeof(double); }

// What true-peak detection adds to the limit kernel's arguments: the interpolator's taps (truepeak_host.h)
// and the reset bits of the true-peak meters.  The sample-peak instantiations take an empty placeholder.
template <bool TP> struct NupcLimTp { int none; };
template <> struct NupcLimTp<true> { TruepeakTaps taps; unsigned int tp_reset; };

// The front half of the emit step: the period's x_c -- emit_take times the frame's factor, behind the
// sub-delay FIR if the channel has a filter, the very device functions of nupc_emit_kernel in their order --
// into the channel's ring of R = D + L0 reals, frame t in cell t mod R (base = opos mod R).  The cells it
// overwrites held frames opos - R .. opos - D - 1, which the previous period's limit kernel was the last
// to need.  Ring cells of the accumulator are cleared by emit_take, the gain ramp advances here.
template <typename T, bool SD>
__global__ __launch_bounds__(256) void
nupc_limit_stage_kernel(T *__restrict__ acc_old, T *__restrict__ acc_new, unsigned long long pos, int A, int n_out, int L0,
                        long long rel0, int F, NupcGain *__restrict__ gain, T *__restrict__ ring, int R, int base,
                        const NupcSd<T> sd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sd_smem[];
    const int ch = blockIdx.x, tid = threadIdx.x;
    GainFactor<T> sc;
    sc.load(gain[ch], L0);
    T *x = ring + (size_t)ch * R;
    if (SD && sd.vals.v[ch] != -100)
        sd_fir_period<T>(sd_smem, sd, ch, L0,
                         [&](int n) { return emit_take(acc_old, acc_new, pos, A, n_out, ch, n, rel0, F) * sc.at(n); },
                         [&](int n, T y) { x[(base + n) % R] = y; });
    else
        for (int n = tid; n < L0; n += 256)
            x[(base + n) % R] = emit_take(acc_old, acc_new, pos, A, n_out, ch, n, rel0, F) * sc.at(n);
    __syncthreads();                                   // every thread has its copy of the record
    if (tid == 0) gain_advance(gain + ch, L0);
}

// (A1, v1) o (A2, v2) = (A1 A2, max(A2 v1, v2)): the deficit d = 1 - e of the release recursion,
// d[t] = max(1 - m[t], a d[t - 1]), composes with it, so a period's recursion is a prefix scan
struct LimScan { double A, v; };
__device__ __forceinline__ LimScan lim_op(const LimScan &p, const LimScan &c) { return {p.A * c.A, fmax(c.A * p.v, c.v)}; }

// The group envelope of `cnt` frames (one tile), by the whole workgroup (256 threads, every thread calls).
// On entry rr = [D history | cnt new] values of r and ee[0 .. D) the history of e; on return ee[D + n] is
// e of the tile's frame n, and rr and ww hold scratch (the caller keeps r's history in registers).
//   sliding minimum  m[n] = min rr[n .. n + D]: log-step doubling between rr and ww, k = floor(log2(D + 1))
//       passes give the minima of 2^k cells, two of which cover the D + 1 (min is exact: any order, same bits)
//   release          the scan above: each thread folds its `per` consecutive frames, the wave scans the
//       threads' pairs with __shfl_up, the waves' totals go through LDS, and the thread walks its frames again
//       from the deficit in front of it.  The carry into the tile is 1 - e of the frame before it.
//   e[t] = min(m[t], 1 - d[t]): never above m[t], whatever the scan rounds.
__device__ __forceinline__ void
lim_envelope_tile(double *rr, double *ww, double *ee, int D, int cnt, double a) {
    __shared__ LimScan wave_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, total = D + cnt;
    double *src = rr, *dst = ww;
    int span = 1;
    for (; 2 * span <= D + 1; span *= 2) {
        for (int i = tid; i < total; i += 256) dst[i] = i >= span ? fmin(src[i], src[i - span]) : src[i];
        __syncthreads();
        double *t = src; src = dst; dst = t;
    }
    const int back = D + 1 - span;                     // the second window of `span` cells ends `back` cells earlier
    const int per = (cnt + 255) / 256, n0 = tid * per, n1 = min(n0 + per, cnt);
    LimScan mine = {1.0, 0.0};
    for (int n = n0; n < n1; n++) {
        const double m = fmin(src[D + n], src[D + n - back]);
        dst[n] = m;                                    // each thread's own cells, read back below by itself only
        mine = lim_op(mine, {a, 1.0 - m});
    }
    LimScan inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const LimScan p = {__shfl_up(inc.A, off), __shfl_up(inc.v, off)};
        if (lane >= off) inc = lim_op(p, inc);
    }
    LimScan ex = {__shfl_up(inc.A, 1), __shfl_up(inc.v, 1)};
    if (lane == 0) ex = {1.0, 0.0};
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    LimScan front = {1.0, 1.0 - ee[D - 1]};            // the deficit of the frame in front of the tile
    for (int w = 0; w < wave; w++) front = lim_op(front, wave_tot[w]);
    double d = lim_op(front, ex).v;
    for (int n = n0; n < n1; n++) {
        const double m = dst[n];
        d = fmax(a * d, 1.0 - m);
        ee[D + n] = fmin(m, 1.0 - d);
    }
    __syncthreads();
}

// The back half: the group's envelope for the period, y for this workgroup's channel, and the rest of the
// emit step on y -- the Quantiser path or the dither chain (DITHER: through the stage buffer the dither
// path already uses), overflow commit, the status hand-off of the n_out workgroups.  Every member of a
// group computes the group's envelope itself from the members' staged x: the same code on the same
// inputs gives the same bits, so the members agree without exchanging anything, and only the group's first
// member writes the state, into the other parity.  A channel in no group takes x D frames late, unmultiplied.
// D is the envelope's look-ahead; the delay of x is in the ring's geometry (R - L0 frames).
// TP (bfhip_nupc_set_limiter_detector, TRUE_PEAK): p is the peak over the four phases of the interpolator
// instead of the sample's.  The ring holds frames opos - (R - L0) .. opos + L0 - 1 and the detector of frame
// opos reads back to opos - (2 H - 1), inside it since R - L0 >= 2 H.  Per tile and member in turn, the member's
// cnt + 2 H - 1 cells are staged into LDS as float64 (a non-finite one as 0; the window is shorter than the
// ring, so it wraps at most once: two runs); each thread forms the three 24-tap sums of its frames, k
// ascending, from consecutive doubles (consecutive lanes, consecutive cells: no bank conflict), takes phase 0
// from cell n + H - 1, and folds the peak over its ceiling into rr[D + n], which no other thread touches.  D is
// then the look-ahead less H, and the state gains the true-peak meter's maximum behind the reduction meter.
template <typename T, bool DITHER, bool TP = false>
__global__ __launch_bounds__(256) void
nupc_limit_emit_kernel(const T *__restrict__ ring, int R, int base, int D, int L0, int tile, double a,
                       const NupcLimGroup *__restrict__ groups, const int *__restrict__ group_of,
                       double *__restrict__ state, int parity, const NupcLimThr thr, unsigned int meter_reset,
                       const DevFormat *__restrict__ fmt, DevOverflow *__restrict__ over, uint8_t *__restrict__ raw,
                       double safety_limit, int *__restrict__ status, unsigned int *__restrict__ arrive,
                       int *__restrict__ host_status, const int *__restrict__ dslot, T *__restrict__ stage,
                       DitherState<T> *__restrict__ dstate, const int8_t *__restrict__ table, int table_size,
                       const T *__restrict__ randmap /* index -256..255 (centre pointer) */, const NupcLimTp<TP> tp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lim_smem[];
    __shared__ T rmap[DITHER ? 512 : 1];
    __shared__ double red_min[4], g_ceil[kLimGroupMax];
    __shared__ double red_max[TP ? 4 : 1], g_scale[TP ? kLimGroupMax : 1];
    __shared__ int g_ch[kLimGroupMax];
    const int ch = blockIdx.x, tid = threadIdx.x;
    const DevFormat f = fmt[ch];
    const int slot = DITHER ? dslot[ch] : -1;
    const int g = group_of[ch];
    const T *x = ring + (size_t)ch * R;
    uint8_t *out = raw + f.byte_offset;
    const size_t stride = (size_t)f.sample_spacing * f.bytes;
    T *staged = slot < 0 ? nullptr : stage + (size_t)slot * L0;
    DevOverflow of;
    Quantiser<T> qz;
    if (slot < 0) { of = over[ch]; qz.init(f, of, safety_limit); }
    // frame n of the period leaves as x[n - D] (cell base + n + L0 mod R) times s
    auto put = [&](int n, T y) {
        if (slot < 0) qz.put(y, out + (size_t)n * stride);
        else staged[n] = y;
    };
    if (g < 0) {
        for (int n = tid; n < L0; n += 256) put(n, x[(base + n + L0) % R]);
    } else {
        // the group's row and its members' ceilings thr_g / scale_c through LDS: indexed by a loop counter
        const NupcLimGroup *grp = groups + g;
        const int n_ch = grp->n_ch;
        if (tid < n_ch) {
            g_ch[tid] = grp->ch[tid];
            g_ceil[tid] = thr.v[g] / grp->scale[tid];
            if constexpr (TP) g_scale[tid] = grp->scale[tid];
        }
        const size_t ss = (size_t)2 * D + (TP ? 2 : 1);
        const double *st_in = state + ((size_t)g * 2 + parity) * ss;
        double *st_out = state + ((size_t)g * 2 + (1 - parity)) * ss;
        double *rr = reinterpret_cast<double *>(lim_smem), *ww = rr + D + tile, *ee = ww + D + tile;
        for (int i = tid; i < D; i += 256) { rr[i] = st_in[i]; ee[i] = st_in[D + i]; }
        __syncthreads();
        double s_min = 1.0;
        [[maybe_unused]] double tp_max = 0.0;
        for (int t0 = 0; t0 < L0; t0 += tile) {
            const int cnt = min(tile, L0 - t0);
            if constexpr (TP) {
                double *win = ee + D + tile;                    // [tile + 2 H - 1]: frames t0 - (2 H - 1) .. t0 + cnt - 1
                const int len = cnt + kTpTaps - 1, start = (base + t0 - (kTpTaps - 1) + R) % R, first = min(len, R - start);
                for (int n = tid; n < cnt; n += 256) rr[D + n] = 0.0;
                for (int k = 0; k < n_ch; k++) {
                    const T *xk = ring + (size_t)g_ch[k] * R;
                    for (int i = tid; i < first; i += 256) { const double v = (double)xk[start + i]; win[i] = isfinite(v) ? v : 0.0; }
                    for (int i = first + tid; i < len; i += 256) { const double v = (double)xk[i - first]; win[i] = isfinite(v) ? v : 0.0; }
                    __syncthreads();
                    const double ceil_k = g_ceil[k], scale_k = g_scale[k];
                    for (int n = tid; n < cnt; n += 256) {
                        const double *w = win + n + kTpTaps - 1;            // frame t0 + n; frame t0 + n - j is w[-j]
                        double peak = fabs(w[-kTpHalf]);
#pragma unroll
                        for (int q = 0; q < kTpPhases; q++) {
                            double u = 0.0;
#pragma unroll
                            for (int j = 0; j < kTpTaps; j++) u += tp.taps.g[q][j] * w[-j];
                            peak = fmax(peak, fabs(u));
                        }
                        tp_max = fmax(tp_max, peak * scale_k);
                        rr[D + n] = fmax(rr[D + n], peak / ceil_k);
                    }
                    __syncthreads();                            // the window is free for the next member
                }
                for (int n = tid; n < cnt; n += 256) { const double p = rr[D + n]; rr[D + n] = p > 1.0 ? 1.0 / p : 1.0; }
            } else {
                for (int n = tid; n < cnt; n += 256) {
                    double p = 0.0;
                    for (int k = 0; k < n_ch; k++) {
                        const double v = (double)ring[(size_t)g_ch[k] * R + (base + t0 + n) % R];
                        if (isfinite(v)) p = fmax(p, fabs(v) / g_ceil[k]);
                    }
                    rr[D + n] = p > 1.0 ? 1.0 / p : 1.0;
                }
            }
            __syncthreads();
            double keep_r[kLimLookaheadMax / 256], keep_e[kLimLookaheadMax / 256];
#pragma unroll
            for (int i = 0; i < kLimLookaheadMax / 256; i++) { const int n = tid + i * 256; if (n < D) keep_r[i] = rr[cnt + n]; }
            __syncthreads();
            lim_envelope_tile(rr, ww, ee, D, cnt, a);
            const double w1 = (double)(D + 1);
            for (int n = tid; n < cnt; n += 256) {
                double sum = 0.0;
                for (int j = 0; j <= D; j++) sum += ee[D + n - j];
                const double s = sum / w1;
                s_min = fmin(s_min, s);
                put(t0 + n, x[(base + t0 + n + L0) % R] * (T)s);
            }
            // the histories moved down: the last D values of r and of e in front of the next tile
#pragma unroll
            for (int i = 0; i < kLimLookaheadMax / 256; i++) { const int n = tid + i * 256; if (n < D) keep_e[i] = ee[cnt + n]; }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < kLimLookaheadMax / 256; i++) {
                const int n = tid + i * 256;
                if (n < D) { rr[n] = keep_r[i]; ee[n] = keep_e[i]; }
            }
            __syncthreads();
        }
        if (g_ch[0] == ch) {                          // the group's first member keeps its state
            for (int i = tid; i < D; i += 256) { st_out[i] = rr[i]; st_out[D + i] = ee[i]; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s_min = fmin(s_min, __shfl_down(s_min, off));
            if ((tid & 63) == 0) red_min[tid >> 6] = s_min;
            if constexpr (TP) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) tp_max = fmax(tp_max, __shfl_down(tp_max, off));
                if ((tid & 63) == 0) red_max[tid >> 6] = tp_max;
            }
            __syncthreads();
            if (tid == 0) {
                const double before = (meter_reset >> g) & 1u ? 1.0 : st_in[2 * D];
                st_out[2 * D] = fmin(fmin(before, fmin(red_min[0], red_min[1])), fmin(red_min[2], red_min[3]));
                if constexpr (TP) {
                    const double seen = (tp.tp_reset >> g) & 1u ? 0.0 : st_in[2 * D + 1];
                    st_out[2 * D + 1] = fmax(fmax(seen, fmax(red_max[0], red_max[1])), fmax(red_max[2], red_max[3]));
                }
            }
        }
    }
    if (slot < 0) {
        qz.reduce(tid, 256);
        if (tid == 0) {
            qz.commit(of);
            over[ch] = of;
            if (qz.st) atomicOr(status, qz.st);
            emit_hand_off(status, arrive, host_status);
        }
        return;
    }
    if constexpr (DITHER) {
        for (int i = tid; i < 512; i += 256) rmap[i] = randmap[i - 256];
        __syncthreads();              // the staged samples are visible to wave 0 (same workgroup)
        if (tid < 64) {
            dither_chain<T>(staged, dstate + slot, table, table_size, rmap, f, over + ch, raw, L0, safety_limit, status, tid);
            if (tid == 0) emit_hand_off(status, arrive, host_status);
        }
    }
}

// ---- per-channel integer delay and mute on the raw I/O blocks: the device half of the delay machine
// (the job, NupcDelayJob, and the host half that makes it, NupcDelay, are in nupc_sched.h)
constexpr int kDelayJobs = 32;     // jobs per launch (2048 bytes of kernel arguments)
static_assert(sizeof(NupcDelayJob) <= 64, "32 jobs must stay well inside the 4 KB of kernel arguments");
struct NupcDelayJobs { NupcDelayJob j[kDelayJobs]; };

__device__ __forceinline__ unsigned long long smp_ld(const uint8_t *p, int ss) {
    unsigned long long v = 0;
    for (int b = 0; b < ss; b++) v |= (unsigned long long)p[b] << (8 * b);
    return v;
}
__device__ __forceinline__ void smp_st(uint8_t *p, unsigned long long v, int ss) {
    for (int b = 0; b < ss; b++) p[b] = (uint8_t)(v >> (8 * b));
}
// p is 16-byte aligned (arena fragments)
__device__ __forceinline__ void zero_bytes(uint8_t *p, unsigned long long n) {
    const unsigned long long n16 = n / 16;
    for (unsigned long long i = threadIdx.x; i < n16; i += blockDim.x) ((uint4 *)p)[i] = make_uint4(0, 0, 0, 0);
    for (unsigned long long i = n16 * 16 + threadIdx.x; i < n; i += blockDim.x) p[i] = 0;
}

// One workgroup per job, on the raw block `raw` of F frames (the job's stride apart, ss-byte
// samples).  mute_first: input side (do_mute before update_delay: zeros enter the line); else
// output side (the delayed block is muted).  Every thread reads and writes only its own samples of
// the raw block; the exchange between samples goes through the arena's scratch fragment.
__global__ __launch_bounds__(256) void
nupc_delay_kernel(const NupcDelayJobs jobs, uint8_t *__restrict__ raw, int F, int mute_first) {
    const NupcDelayJob j = jobs.j[blockIdx.x];
    uint8_t *buf = raw + j.byte_offset;
    const int ss = j.ss;
    const size_t stride = (size_t)j.stride, fragp = (size_t)j.fragp;
    if (j.kind == 0) {                                             // no delay in force: a muted channel
        for (int n = threadIdx.x; n < F; n += blockDim.x) smp_st(buf + n * stride, 0, ss);
        return;
    }
    uint8_t *rest = j.line + (size_t)j.rest_frag * fragp, *sh0 = rest + fragp, *sh1 = sh0 + fragp, *tmp = sh1 + fragp;
    // change_delay's zero-fills, and the block into the scratch (zeros if muted before the line)
    zero_bytes(j.line, j.zfull);
    zero_bytes(rest, (unsigned long long)j.zrest);
    zero_bytes(sh0, (unsigned long long)j.zshort);
    zero_bytes(sh1, (unsigned long long)j.zshort);
    const bool mute_in = mute_first && j.muted, mute_out = !mute_first && j.muted;
    for (int n = threadIdx.x; n < F; n += blockDim.x)
        smp_st(tmp + (size_t)n * ss, mute_in ? 0ull : smp_ld(buf + n * stride, ss), ss);
    __syncthreads();                                               // scratch and zero-fills are visible
    __threadfence_block();
    const int rr = j.rr;
    if (j.kind == 1) {                                             // update_delay_buffer, delay.c:229-262
        uint8_t *fcur = j.line + (size_t)j.cur * fragp;
        const uint8_t *last = j.line + (size_t)j.last * fragp;
        for (int n = threadIdx.x; n < F; n += blockDim.x) {
            smp_st(fcur + (size_t)n * ss, smp_ld(tmp + (size_t)n * ss, ss), ss);
            unsigned long long y;
            if (n < rr) {
                y = smp_ld(rest + (size_t)n * ss, ss);
                smp_st(rest + (size_t)n * ss, smp_ld(last + (size_t)(F - rr + n) * ss, ss), ss);
            } else
                y = smp_ld(last + (size_t)(n - rr) * ss, ss);
            smp_st(buf + n * stride, mute_out ? 0ull : y, ss);
        }
    } else {                                                       // update_delay_short_buffer, :264-281
        uint8_t *shw = j.cur ? sh1 : sh0;
        const uint8_t *shr = j.last ? sh1 : sh0;
        for (int n = threadIdx.x; n < F; n += blockDim.x) {
            const unsigned long long y = n < rr ? smp_ld(shr + (size_t)n * ss, ss) : smp_ld(tmp + (size_t)(n - rr) * ss, ss);
            if (n < rr) smp_st(shw + (size_t)n * ss, smp_ld(tmp + (size_t)(F - rr + n) * ss, ss), ss);
            smp_st(buf + n * stride, mute_out ? 0ull : y, ss);
        }
    }
}

// ---- host: the launches

// the kernels are instantiated per real type, the emit kernels also per "the output side uses sub-delay":
// f(T(), std::bool_constant<SD>()) with the convolver's two
template <typename F> void nupc_dispatch(const bfhip_nupc *n, F f) {
    const bool sd = n->sd.use[1];
    if (n->rs == 4) { if (sd) f(float(), std::true_type()); else f(float(), std::false_type()); }
    else { if (sd) f(double(), std::true_type()); else f(double(), std::false_type()); }
}

// a segment block's output into the ring(s) its plan names: a block that ran under both assignments adds
// its second output into the second ring (aligned switch) or blends the two into the one (staggered)
int nupc_accumulate(bfhip_nupc *n, const Seg &s, const BlockPlan &b) {
    const size_t cnt = (size_t)s.L * n->n_out;
    const dim3 grid((unsigned)((cnt + 255) / 256));
    nupc_dispatch(n, [&](auto t, auto) {
        using T = decltype(t);
        if (b.fade)
            hipLaunchKernelGGL(nupc_accumulate_fade_kernel<T>, grid, dim3(256), 0, n->stream, (T *)n->ring(b.ring),
                               (const T *)s.d_out, (const T *)s.d_out2, b.pos, n->A, n->n_out, s.L,
                               (long long)b.pos - b.t_k, b.F);
        else
            hipLaunchKernelGGL(nupc_accumulate_kernel<T>, grid, dim3(256), 0, n->stream, (T *)n->ring(b.ring),
                               (const T *)s.d_out, (T *)(b.ring2 < 0 ? nullptr : n->ring(b.ring2)), (const T *)s.d_out2,
                               b.pos, n->A, n->n_out, s.L);
    });
    NCHK(hipGetLastError());
    return BFHIP_OK;
}

// this period's delay / mute step of one side on its raw block; no launch if no channel of the
// side is muted or has a delay line with work
int nupc_delay_side(bfhip_nupc *n, int io, uint8_t *raw) {
    // (a side with a declared buffer had every channel's samples checked against it at finalize)
    for (size_t ch = 0; ch < n->dl[io].size() && !n->io.buf_bytes[io]; ch++) {
        const bfhip_format &f = n->io.fmt[io][ch];
        if ((n->dl[io][ch].arena || n->dl[io][ch].muted) &&
            (f.byte_offset < 0 || (size_t)f.byte_offset + f.bytes > n->io.frame_bytes[io]))
            return nfail(BFHIP_EINVAL, "nupc: delay / mute on a channel whose samples lie outside the raw frame");
    }
    NupcDelayJobs args;
    int cnt = 0;
    auto launch = [&]() {
        hipLaunchKernelGGL(nupc_delay_kernel, dim3(cnt), dim3(256), 0, n->stream, args, raw, n->L0(), io == BFHIP_IN ? 1 : 0);
        cnt = 0;
        return hipGetLastError();
    };
    for (size_t ch = 0; ch < n->dl[io].size(); ch++) {
        if (cnt == 0) memset(&args, 0, sizeof(args));
        NupcDelayJob &jb = args.j[cnt];
        if (!n->dl[io][ch].step(jb)) continue;
        const bfhip_format &f = n->io.fmt[io][ch];
        jb.byte_offset = f.byte_offset;
        jb.ss = f.bytes;
        jb.stride = f.sample_spacing * f.bytes;
        if (++cnt == kDelayJobs) NCHK(launch());
    }
    if (cnt > 0) NCHK(launch());
    return BFHIP_OK;
}

// this period's sub-delay arguments of one side: the values in force now
template <typename T> NupcSd<T> nupc_sd_args(const bfhip_nupc *n, int io) {
    NupcSd<T> a;
    memset(&a, 0, sizeof(a));
    memset(a.vals.v, -100, sizeof(a.vals.v));                     // no channel has a filter
    if (!n->sd.use[io]) return a;
    a.bank = (const T *)n->sd.d_bank;
    a.hist = (T *)n->sd.d_hist[io];
    a.bs = n->sd.bs; a.flen = n->sd.flen; a.tile = std::min(n->L0(), kSdTile);
    for (size_t ch = 0; ch < n->sd.val[io].size(); ch++) a.vals.v[ch] = (signed char)n->sd.val[io][ch];
    return a;
}
size_t nupc_sd_smem(const bfhip_nupc *n, int io) {
    return n->sd.use[io] ? nupc_sd_lds(n->sd.bs, n->sd.flen, std::min(n->L0(), kSdTile), n->rs) : 0;
}

// input side with sub-delay or a declared buffer: the period's raw samples (delayed and muted
// already; the raw ring's slot, or the stage) become the reals of slot wpos of the ring the segment
// engines read
int nupc_subdelay_in(bfhip_nupc *n, const uint8_t *raw_slot, size_t wpos) {
    uint8_t *real = n->d_in_real + wpos * (size_t)n->n_in * n->rs;
    nupc_dispatch(n, [&](auto t, auto) {
        using T = decltype(t);
        hipLaunchKernelGGL(nupc_subdelay_in_kernel<T>, dim3(n->n_in), dim3(256), nupc_sd_smem(n, 0), n->stream, raw_slot,
                           n->io.d_fmt[0], (T *)real, n->n_in, n->L0(), nupc_sd_args<T>(n, 0));
    });
    NCHK(hipGetLastError());
    return BFHIP_OK;
}

// the emit step of the period whose first frame is opos: the four kernels (dither or not, sub-delay on the
// output side or not) share their leading arguments; the schedule says which rings are read
int nupc_emit(bfhip_nupc *n, unsigned long long opos, void *rawout_dev) {
    const Switcher &sw = n->sets.sched;
    void *acc_old = n->ring(sw.cur), *acc_new = sw.two_rings() ? n->ring(1 - sw.cur) : nullptr;
    const long long rel0 = sw.rel0(opos);
    const int L0 = n->L0();
    nupc_dispatch(n, [&](auto t, auto sd_side) {
        using T = decltype(t);
        constexpr bool SD = decltype(sd_side)::value;
        const NupcSd<T> sd = nupc_sd_args<T>(n, 1);
        const size_t smem = SD ? nupc_sd_smem(n, 1) : 0;
        if (!n->dither.ch.empty())
            hipLaunchKernelGGL((nupc_emit_dither_kernel<T, SD>), dim3(n->n_out), dim3(256), smem, n->stream, (T *)acc_old,
                               (T *)acc_new, opos, n->A, n->n_out, L0, rel0, sw.sw_F, n->io.d_fmt[1], n->og.d,
                               n->st.d_over, (uint8_t *)rawout_dev, n->safety_limit, n->st.d_status, n->st.d_arrive,
                               n->st.h_status, n->dither.d_slot, (T *)n->dither.d_stage,
                               (DitherState<T> *)n->dither.d_state, n->dither.d_table, (int)n->dither.table.size(),
                               (const T *)n->dither.d_randmap + 256, sd);
        else
            hipLaunchKernelGGL((nupc_emit_kernel<T, SD>), dim3(n->n_out), dim3(256), smem, n->stream, (T *)acc_old,
                               (T *)acc_new, opos, n->A, n->n_out, L0, rel0, sw.sw_F, n->io.d_fmt[1], n->og.d, n->st.d_over,
                               (uint8_t *)rawout_dev, n->safety_limit, n->st.d_status, n->st.d_arrive, n->st.h_status, sd);
    });
    NCHK(hipGetLastError());
    return BFHIP_OK;
}

// the emit step of a convolver with a limiter: the stage launch and the limit-and-emit launch, this period's
// thresholds and the meters' reset bits as kernel arguments
int nupc_limit_emit(bfhip_nupc *n, unsigned long long opos, void *rawout_dev) {
    const Switcher &sw = n->sets.sched;
    NupcLimiter &lm = n->lim;
    void *acc_old = n->ring(sw.cur), *acc_new = sw.two_rings() ? n->ring(1 - sw.cur) : nullptr;
    const long long rel0 = sw.rel0(opos);
    const int L0 = n->L0(), R = lm.D + L0, base = (int)(opos % (unsigned long long)R), tile = std::min(L0, kLimTile);
    NupcLimThr thr;
    for (int g = 0; g < kLimGroupsMax; g++) thr.v[g] = g < (int)lm.thr.size() ? lm.thr[g] : 1.0;
    nupc_dispatch(n, [&](auto t, auto sd_side) {
        using T = decltype(t);
        constexpr bool SD = decltype(sd_side)::value;
        hipLaunchKernelGGL((nupc_limit_stage_kernel<T, SD>), dim3(n->n_out), dim3(256), SD ? nupc_sd_smem(n, 1) : 0, n->stream,
                           (T *)acc_old, (T *)acc_new, opos, n->A, n->n_out, L0, rel0, sw.sw_F, n->og.d, (T *)lm.d_ring, R,
                           base, nupc_sd_args<T>(n, 1));
        // the detector picks the instantiation, its LDS and its extra arguments; everything else is shared
        auto back = [&](auto dith, auto det, size_t lds) {
            constexpr bool DITHER = decltype(dith)::value, TP = decltype(det)::value;
            NupcLimTp<TP> tp = {};
            if constexpr (TP) { tp.taps = lm.taps; tp.tp_reset = lm.tp_reset; }
            hipLaunchKernelGGL((nupc_limit_emit_kernel<T, DITHER, TP>), dim3(n->n_out), dim3(256), lds,
                               n->stream, (const T *)lm.d_ring, R, base, lm.De(), L0, tile, lm.a, lm.d_groups, lm.d_group_of,
                               lm.d_state, (int)(n->block & 1), thr, lm.meter_reset, n->io.d_fmt[1], n->st.d_over,
                               (uint8_t *)rawout_dev, n->safety_limit, n->st.d_status, n->st.d_arrive, n->st.h_status,
                               n->dither.d_slot, (T *)n->dither.d_stage, (DitherState<T> *)n->dither.d_state,
                               n->dither.d_table, (int)n->dither.table.size(),
                               DITHER ? (const T *)n->dither.d_randmap + 256 : nullptr, tp);
        };
        auto detector = [&](auto dith) {
            if (lm.true_peak()) back(dith, std::true_type(), nupc_lim_tp_lds(lm.De(), tile));
            else back(dith, std::false_type(), nupc_lim_lds(lm.D, tile));
        };
        if (!n->dither.ch.empty()) detector(std::true_type()); else detector(std::false_type());
    });
    NCHK(hipGetLastError());
    lm.meter_reset = 0;
    lm.tp_reset = 0;
    return BFHIP_OK;
}

}  // namespace
