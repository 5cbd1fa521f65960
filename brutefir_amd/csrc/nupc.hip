// nupc.hip -- non-uniform partitioned convolution (low-latency first block) on top of the
// uniform engines.  An EXTENSION: the reference only has uniform partitions
// (`filter_length: L,N`, bfconf.c:1495-1520); BASELINE.json's room-correction
// config asks for "non-uniform partition sizes (low-latency first block)".  Results are the
// same linear convolution a uniform run computes (tests compare against the oracle's uniform
// engine on the same stream); only the I/O block -- the latency -- shrinks from L to the
// smallest segment length.
//
// The impulse response is cut into segments; segment k is a uniform partitioned convolver
// (a bfhip_engine) with partition length L_k (ascending powers of two) and N_k partitions,
// covering taps [off_k, off_k + N_k * L_k), off_0 = 0.  I/O happens in blocks of L_0 frames.
// After input block b, every segment whose block is complete ((b+1) * L_0 multiple of L_k)
// runs on the last L_k frames; its L_k output frames belong at absolute sample
// (b+1) * L_0 - L_k + off_k and are added into a time-domain accumulator ring; then the L_0
// frames of output block b are requantised out of the ring.  A contribution is in time iff
//     off_k >= L_k - L_0
// (checked at create); e.g. 2 x 64, 2 x 128, ... doubling satisfies it with equality + L_0.
// A segment that starts later than it has to (slack = off_k - (L_k - L_0) > 0 frames; one period
// for every segment but the first in the "two blocks per size, doubling" schedule, L_k - L_0
// at most) does not have to be finished within the period it is launched in: it runs on its
// own low-priority stream beside the periods that follow, and the main stream only waits for
// it in the period its first output frame is due.  So the worst period costs about as much
// as the common one, which is what real-time use needs.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bfhip_nupc.h"
#include "alloc.h"
#include "coeff_async.h"
#include "dither_init.h"
#include "eq_minphase.h"
#include "eq_render.h"
#include "kernels.h"
#include "subdelay_filter.h"

using namespace bfhip;

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
//
// One record per output channel in device memory (bfhip_nupc_set_output_gain / _set_gain_ramp).
// The gain of the frame `idx` frames after the ramp's first one is
//     idx < len - 1:  a + (g - a) (idx + 1) / len        else g (len 0: a step, always g)
// in float64 for both precisions; the factor handed to the sample is (T)(inv * gain).  The emit
// step evaluates it per frame and advances `done` itself, so a ramp in progress needs no upload;
// the host uploads the records only when a target changes (its mirror advances the same way).
struct NupcGain {
    double inv;                    // 1 / the output format's scale
    double a, g;                   // gain of the last frame before the ramp, target
    int done, len;                 // frames of the ramp emitted so far (saturates at len), ramp length
};
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

// ---- per-channel integer delay and mute on the raw I/O blocks (dai.c's do_mute / update_delay)
//
// One channel's period step of the reference's delay machine (delay.c:229-340).  The state
// transitions (change_delay, curbuf) depend on the requested delays only, never on the samples,
// so the host keeps them (NupcDelay below) and passes each period's step as a job in the kernel
// arguments.  The line's data lives in a device arena per channel:
//     [n_full_cap whole fragments][rest][short 0][short 1][scratch], `fragp` bytes each
// (fragp = L0 * bytes rounded up to 16, so change_delay's whole-fragment zero-fill is one range).
// A channel's sample size, its stride in the raw block and so its fragment pitch are its own: the
// channels of a side may come from devices with different sample formats and layouts.
struct NupcDelayJob {
    uint8_t *line;                 // the channel's arena
    unsigned long long zfull;      // change_delay: bytes of whole fragments to zero, from line[0]
    int rest_frag;                 // index of the rest fragment (n_full_cap)
    int byte_offset;               // the channel's first sample in the raw block
    int ss, stride;                // bytes of a sample, bytes from one sample to the next in the raw block
    unsigned int fragp;            // bytes from one fragment of the arena to the next
    int kind;                      // 0 mute only, 1 whole fragments (update_delay_buffer),
                                   // 2 short (update_delay_short_buffer)
    int muted;
    int cur, last;                 // kind 1: fragment written / read; kind 2: short buffer written / read
    int rr;                        // n_rest
    int zrest, zshort;             // change_delay: bytes to zero in the rest / in each short buffer
};
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

// host side of one channel's delay machine: delay_allocate_buffer / change_delay / the curbuf
// walk of delay.c, mirrored from the oracle's bfo_delay (pinned to delay.c by the CPU tests)
struct NupcDelay {
    int maxdelay = -1;             // < 0: fixed
    int req = 0;                   // before finalize the initial delay, after it the requested one
    int extra = 0;                 // whole frames added at finalize to a channel without a sub-delay filter
                                   // on a side that uses sub-delay (dai.c:230-243): part of req, maxdelay
                                   // and curdelay from then on, never reported
    bool muted = false;
    int curdelay = 0, cur = 0, n_full = 0, n_rest = 0, n_full_cap = 0, F = 0, ss = 0;
    uint8_t *arena = nullptr;      // null: no line (a delay of 0 that cannot change)
    size_t fragp = 0;

    // delay_allocate_buffer's state (delay.c:357-407); returns the arena bytes, 0 = no line
    size_t init(int fragment, int sample_size) {
        F = fragment; ss = sample_size;
        int initdelay = req;
        int delay = maxdelay <= 0 ? initdelay : maxdelay;
        if (maxdelay >= 0 && delay > maxdelay) delay = initdelay = maxdelay;
        if (maxdelay > 0 && initdelay > maxdelay) initdelay = maxdelay;
        curdelay = req = initdelay;
        if (delay == 0) return 0;
        fragp = ((size_t)F * ss + 15) / 16 * 16;
        n_full_cap = delay > F ? delay / F + 1 : 0;
        if (delay <= F) n_rest = initdelay;
        else {
            n_rest = initdelay % F;
            n_full = initdelay / F + 1;
            if (n_full == 1) n_full = 0;
        }
        return (size_t)(n_full_cap + 4) * fragp;
    }

    // this period's step (change_delay with the requested delay, then the update); false: nothing to do
    bool step(NupcDelayJob &jb) {
        jb = NupcDelayJob();
        jb.muted = muted;
        if (arena) {
            const int nd = req;
            if (nd != curdelay && nd <= maxdelay) {                // change_delay, delay.c:283-318
                if (nd <= F) {
                    n_rest = nd;
                    if (curdelay > F || curdelay < nd) jb.zshort = nd * ss;
                    n_full = 0;
                } else {
                    n_rest = nd % F;
                    n_full = nd / F + 1;
                    if (curdelay < nd) { jb.zfull = (unsigned long long)n_full * fragp; jb.zrest = n_rest * ss; }
                }
                cur = 0; curdelay = nd;
            }
            jb.line = arena; jb.rest_frag = n_full_cap; jb.rr = n_rest; jb.fragp = (unsigned int)fragp;
            if (n_full > 0) {
                jb.kind = 1; jb.cur = cur; jb.last = cur == n_full - 1 ? 0 : cur + 1;
                if (++cur == n_full) cur = 0;
            } else if (n_rest > 0) {
                jb.kind = 2; jb.cur = cur; jb.last = !cur;
                cur = !cur;
            }
        }
        return jb.kind != 0 || muted;
    }
};

thread_local std::string n_err;

// (a runtime failure's sticky error is cleared; argument / state errors make no HIP call)
int nfail(int code, const std::string &msg) { n_err = msg; if (code == BFHIP_EHIP || code == BFHIP_ENOMEM) (void)hipGetLastError(); return code; }

#define NCHK(expr)                                                                          \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) return nfail(BFHIP_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

#define OWNER(n)                                                                            \
    do {                                                                                    \
        if ((n)->owner != getpid())                                                         \
            return nfail(BFHIP_ESTATE, "this convolver belongs to another process: HIP state does not survive fork()"); \
    } while (0)

#define ECHK(expr)                                                                          \
    do {                                                                                    \
        int _r = (expr);                                                                    \
        if (_r < 0) return nfail(_r, std::string(#expr) + ": " + bfhip_last_error());       \
    } while (0)

// what a filter runs under: an assignment is one of these per filter.  gain multiplies the filter's
// out_scale; `set` < 0 / a NaN gain in a queued request mean "not asked for"
struct Asg {
    int set = 0;
    double gain = 1.0;
    bool operator==(const Asg &o) const { return set == o.set && gain == o.gain; }
};

// an output's overflow struct before its first sample (bf_reset_peak)
DevOverflow over_initial(const bfhip_format &f) {
    DevOverflow o;
    memset(&o, 0, sizeof(o));
    o.max = f.isfloat ? 1.0 : (double)((uint64_t)1 << ((f.sbytes << 3) - 1)) - 1;
    return o;
}

struct Seg {
    int L = 0, N = 0;
    long off = 0;               // first tap this segment covers
    bfhip_engine *eng = nullptr;
    void *d_out = nullptr;      // [L][n_out] reals
    // background execution (delay_steps > 0): launched on `stream`, added to the accumulator
    // by the main stream delay_steps periods later
    int delay_steps = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_done = nullptr, ev_consumed = nullptr;
    bool pending = false, consumed_once = false;
    unsigned long long pending_pos = 0, due_block = 0;
    void *pending_acc[2] = {nullptr, nullptr};   // the rings d_out / d_out2 of the pending block go to
    // a pending block of a staggered switch carries its own fade: by the time it is accumulated the
    // switch may have left busy and another may have been committed
    bool pending_fade = false;
    long long pending_tk = 0;
    int pending_F = 0;
    // coefficient switches (only allocated when some filter has more than one set)
    void *d_out2 = nullptr;     // [L][n_out]: the second assignment's output of a block run under both
    void *d_z = nullptr;        // spectra between the split-phase MAC and output calls
    std::vector<Asg> eng_set;   // per filter: the set and gain the engine's filter runs now
    std::vector<std::vector<int>> n_blocks;   // [filter][set]: partitions the set has in this engine
    hipEvent_t ev_upd = nullptr;   // background segment with a reservation: its share of a rewrite is done
};

}  // namespace

struct bfhip_nupc {
    int device = 0, rs = 4, n_in = 0, n_out = 0;
    pid_t owner = 0;                       // like an engine, it lives in the process that created it
    std::vector<Seg> seg;
    std::vector<bfhip_format> fmt[2];
    double safety_limit = 0;
    bool finalized = false, finalize_failed = false;
    unsigned long long block = 0;          // L0-blocks processed
    hipStream_t stream = nullptr;          // main stream: I/O, zero-slack segments, accumulate, emit
    hipEvent_t ev_in = nullptr;            // this period's frames are in the input ring
    int in_frames = 0;                     // input ring length: 2 * Lmax
    unsigned int *d_arrive = nullptr;
    int *h_status = nullptr;               // pinned
    uint8_t *h_in = nullptr, *h_out = nullptr;   // pinned staging of one period (bfhip_nupc_block)
    DevOverflow *h_over = nullptr;         // pinned
    bool background = true;
    int A = 0;                             // accumulator ring length in frames
    void *d_acc = nullptr;                 // [A][n_out] reals
    uint8_t *d_in = nullptr;               // raw input ring: 2 * Lmax frames (not for an input side with a declared buffer)
    size_t frame_bytes[2] = {0, 0};        // interleaved raw frame size in / out (no meaning on a side with a declared buffer)
    // bfhip_nupc_set_buffer_bytes: > 0 = the side declared its period buffer, every channel laid out
    // on its own (planes, several devices).  Such an input side stages the period in d_stage, runs
    // delay and mute in place there and converts it into d_in_real: per-period planes are not
    // contiguous across periods, so no raw ring could give segment k its L_k consecutive frames.
    long buf_bytes[2] = {0, 0};
    size_t period_bytes[2] = {0, 0};       // bytes of one period buffer in / out, whichever way it was declared
    uint8_t *d_stage = nullptr;            // [buf_bytes[0]]: its readers are all ordered on the main stream
    bool in_real = false;                  // the segment engines read d_in_real (fixed at finalize)
    uint8_t *d_rawout = nullptr;
    DevFormat *d_fmt_out = nullptr;
    NupcGain *d_gain = nullptr;            // [n_out]: 1/scale, output gain and its ramp (the emit step advances it)
    DevOverflow *d_over = nullptr;
    int *d_status = nullptr;
    // coefficient sets and switches (filters numbered in add_filter order; set j of filter f is
    // engine coefficient coeff[f][j] in every segment engine)
    std::vector<std::vector<int>> coeff;
    std::vector<double> out_scale;         // per filter: add_filter's, multiplied by the assignment's gain
    std::vector<Asg> live;                 // per filter: the newest committed assignment
    std::vector<Asg> queued;               // per filter: requested set (-1 = none) and gain (NaN = none)
    int crossfade = 0;                     // frames for the next switch (default L0)
    bool gain_reserve = false;             // bfhip_nupc_reserve_filter_gain: gain-only switches need the spare ring
    bool can_switch = false;               // some filter has a second set, or gain_reserve: the spare ring exists
    void *d_acc2 = nullptr;                // the spare ring
    int cur = 0;                           // ring of the live assignment: 0 = d_acc, 1 = d_acc2
    bool sw = false;                       // a committed switch has old-assignment work or fade frames left
    long long t_sw = -1;                   // its switch frame (-1: none committed yet)
    int sw_F = 0;                          // its fade length
    long long old_hi = 0;                  // end of the frames the old assignment has written
    std::vector<Asg> sw_old;               // the old assignment (the new one is `live`)
    // staggered switches (bfhip_nupc_set_switch_mode): every segment switches at its own frame, the
    // fade is blended into the live ring per segment block; the spare ring and `cur` play no part
    int switch_mode = BFHIP_NUPC_SWITCH_ALIGNED;   // for the switches committed from now on
    bool sw_stag = false;                  // the switch in flight (sw) is a staggered one
    std::vector<long long> t_seg;          // per segment: switch frame of the last committed switch
    // output gain: `gain` is the value asked for last, gain_len the ramp length in force at that
    // call; a block call that finds gain != ramp.g starts a ramp (or steps) from the gain of the last
    // emitted frame.  `ramp` mirrors the device records: they are a pure function of the calls.
    std::vector<double> gain;
    std::vector<int> gain_len;
    std::vector<NupcGain> ramp;
    int gain_ramp = 0;                     // bfhip_nupc_set_gain_ramp: for the set_output_gain calls from now on
    bool gain_dirty = false;
    NupcGain *h_gain = nullptr;            // pinned staging of the records
    hipEvent_t ev_gain = nullptr;          // the last upload out of h_gain has been done
    // HP-TPDF dither (dither.c; bfhip_nupc_enable_dither): one slot per dithered output, in
    // ascending channel order; the table walk advances L0 per block call
    std::vector<int> dither_ch;            // output channel of each slot
    std::vector<int8_t> dither_table;
    int dither_spacing = 0;
    int *d_dither_slot = nullptr;          // [n_out]: slot of the channel, -1 = not dithered
    void *d_dither_state = nullptr;        // [n_dither] DitherState
    int8_t *d_dither_table = nullptr;
    void *d_randmap = nullptr;             // 512 reals
    void *d_dither_stage = nullptr;        // [n_dither][L0] reals: the emit step's input to the chain
    // integer delay and mute per raw channel (bfhip_nupc_set_delay / _set_mute): [io][channel]
    std::vector<NupcDelay> dl[2];
    std::vector<NupcDelayJob> dl_jobs;     // this period's jobs of one side (host scratch)
    // sub-sample delay (bfhip_nupc_enable_subdelay / _set_subdelay): [io][channel] values in
    // hundredths of a sample, -100 = the channel has no filter
    int sdf_length = 0, sd_flen = 0, sd_bs = 0;
    std::vector<int> sd[2];
    bool sd_use[2] = {false, false};       // the side has a filter (fixed at finalize)
    void *d_sd_bank = nullptr;             // [199][sd_flen] reals
    void *d_sd_hist[2] = {nullptr, nullptr};   // [channels][sd_bs] reals: unfiltered history
    DevFormat *d_fmt_in = nullptr;         // input formats for the conversion kernel
    uint8_t *d_in_real = nullptr;          // [in_frames][n_in] reals: the ring the engines read instead of d_in
    // asynchronous set rewrite (bfhip_nupc_reserve_update / _update_coeff_async): everything is
    // allocated at finalize; one rewrite in flight at a time
    bool upd_reserve = false;              // asked for before finalize
    uint8_t *h_upd = nullptr;              // pinned staging: taps() reals (bfhip_nupc_update_buffer)
    uint8_t *d_upd = nullptr;              // device staging: the segment engines prepare out of their slices
    hipStream_t upd_stream = nullptr;      // loader: low priority, uploads the background segments' slices
    hipEvent_t ev_upd_load = nullptr;      // the loader's upload is done
    hipEvent_t ev_upd_main = nullptr;      // the main-stream segments' share is done
    int *h_upd_bad = nullptr;              // pinned, one word per segment: the engine's non-finite flag
    bool upd_inflight = false;
    bool upd_failed = false;               // enqueuing it failed part-way: the set's contents are unknown
    int upd_filter = -1, upd_set = -1;     // the set being rewritten / rewritten last
    int upd_result = BFHIP_OK;             // result of the last completed rewrite
    std::vector<std::vector<char>> upd_bad;   // [filter][set]: the last rewrite ended non-finite
    // equaliser render (bfhip_nupc_reserve_eq / _render_eq_async, eq_render.h): a producer in front of
    // the rewrite, on the loader stream; everything is allocated at finalize
    long eq_reserve = 0;                   // max_taps asked for before finalize, 0 = none
    EqRender eq;
    EqMinphase eq_min;                     // bfhip_nupc_reserve_eq_minimum (eq_minphase.h)
    hipEvent_t ev_eq = nullptr;            // the render into eq.taps is done
    void *ring(int i) const { return i ? d_acc2 : d_acc; }
};

extern "C" {

const char *bfhip_nupc_last_error(void) { return n_err.c_str(); }

bfhip_nupc *bfhip_nupc_create(int device, int realsize, int n_in, int n_out, int n_segments,
                              const int seg_length[], const int seg_blocks[]) {
    if (n_segments < 1 || !seg_length || !seg_blocks || n_in < 1 || n_out < 1) { nfail(BFHIP_EINVAL, "nupc_create: bad argument"); return nullptr; }
    bfhip_nupc *n = new bfhip_nupc();
    n->device = device; n->rs = realsize; n->n_in = n_in; n->n_out = n_out;
    n->owner = getpid();
    long off = 0;
    for (int k = 0; k < n_segments; k++) {
        Seg s;
        s.L = seg_length[k]; s.N = seg_blocks[k]; s.off = off;
        if (s.N < 1 || (k > 0 && (s.L <= seg_length[k - 1] || s.L % seg_length[k - 1] != 0))) {
            nfail(BFHIP_EINVAL, "nupc_create: segment lengths must ascend and divide each other");
            delete n; return nullptr;
        }
        if (off < (long)s.L - seg_length[0]) {
            char buf[200];
            snprintf(buf, sizeof(buf), "nupc_create: segment %d (length %d) starts at tap %ld, before %d: its output "
                     "would not be ready in time", k, s.L, off, s.L - seg_length[0]);
            nfail(BFHIP_EINVAL, buf);
            delete n; return nullptr;
        }
        off += (long)s.L * s.N;
        n->seg.push_back(s);
    }
    for (auto &s : n->seg) {
        s.eng = bfhip_engine_create(device, s.L, s.N, realsize, n_in, n_out);
        if (!s.eng) { nfail(BFHIP_EINVAL, std::string("nupc_create: ") + bfhip_last_error()); bfhip_nupc_destroy(n); return nullptr; }
    }
    for (int io = 0; io < 2; io++) {
        const int c = io ? n_out : n_in;
        n->fmt[io].resize(c);
        for (int ch = 0; ch < c; ch++) {
            bfhip_format &f = n->fmt[io][ch];
            f.isfloat = 1; f.swap = 0; f.bytes = f.sbytes = realsize; f.scale = 1.0;
            f.sample_spacing = c; f.byte_offset = ch * realsize;         // interleaved frames
        }
    }
    n->crossfade = seg_length[0];          // the reference's one-block fade
    n->gain.assign(n_out, 1.0);
    n->gain_len.assign(n_out, 0);
    n->dl[0].resize(n_in);
    n->dl[1].resize(n_out);
    n->sd[0].assign(n_in, BFHIP_UNDEFINED_SUBDELAY);
    n->sd[1].assign(n_out, BFHIP_UNDEFINED_SUBDELAY);
    return n;
}

void bfhip_nupc_destroy(bfhip_nupc *n) {
    if (!n) return;
    if (n->owner != getpid()) { for (auto &sg : n->seg) if (sg.eng) bfhip_engine_destroy(sg.eng); delete n; return; }   // a forked child
    (void)hipSetDevice(n->device);
    if (n->stream) (void)hipStreamSynchronize(n->stream);
    for (auto &s : n->seg) if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (n->upd_stream) (void)hipStreamSynchronize(n->upd_stream);
    for (auto &s : n->seg) {
        if (s.eng) bfhip_engine_destroy(s.eng);
        if (s.ev_upd) (void)hipEventDestroy(s.ev_upd);
        if (s.d_out) (void)hipFree(s.d_out);
        if (s.d_out2) (void)hipFree(s.d_out2);
        if (s.d_z) (void)hipFree(s.d_z);
        if (s.ev_done) (void)hipEventDestroy(s.ev_done);
        if (s.ev_consumed) (void)hipEventDestroy(s.ev_consumed);
        if (s.stream) (void)hipStreamDestroy(s.stream);
    }
    void *p[] = {n->d_acc, n->d_acc2, n->d_in, n->d_rawout, n->d_fmt_out, n->d_gain, n->d_over, n->d_status, n->d_arrive,
                 n->d_dither_slot, n->d_dither_state, n->d_dither_table, n->d_randmap, n->d_dither_stage,
                 n->d_sd_bank, n->d_sd_hist[0], n->d_sd_hist[1], n->d_fmt_in, n->d_in_real, n->d_stage};
    for (void *q : p) if (q) (void)hipFree(q);
    for (auto &side : n->dl) for (auto &d : side) if (d.arena) (void)hipFree(d.arena);
    if (n->h_status) (void)hipHostFree(n->h_status);
    if (n->h_in) (void)hipHostFree(n->h_in);
    if (n->h_out) (void)hipHostFree(n->h_out);
    if (n->h_over) (void)hipHostFree(n->h_over);
    if (n->h_gain) (void)hipHostFree(n->h_gain);
    if (n->h_upd) (void)hipHostFree(n->h_upd);
    if (n->h_upd_bad) (void)hipHostFree(n->h_upd_bad);
    if (n->d_upd) (void)hipFree(n->d_upd);
    eq_render_free(n->eq);
    eq_minphase_free(n->eq_min);
    if (n->ev_eq) (void)hipEventDestroy(n->ev_eq);
    if (n->ev_upd_load) (void)hipEventDestroy(n->ev_upd_load);
    if (n->ev_upd_main) (void)hipEventDestroy(n->ev_upd_main);
    if (n->upd_stream) (void)hipStreamDestroy(n->upd_stream);
    if (n->ev_gain) (void)hipEventDestroy(n->ev_gain);
    if (n->ev_in) (void)hipEventDestroy(n->ev_in);
    if (n->stream) (void)hipStreamDestroy(n->stream);
    delete n;
}

long bfhip_nupc_taps(const bfhip_nupc *n) { return n ? n->seg.back().off + (long)n->seg.back().L * n->seg.back().N : 0; }
int bfhip_nupc_latency(const bfhip_nupc *n) { return n ? n->seg[0].L : 0; }

// raw formats of the L0-frame I/O buffers.  On a side that does not declare its buffer
// (bfhip_nupc_set_buffer_bytes) frames must be interleaved (every channel of the side has the same
// sample_spacing = frame size in samples), the way dai.c lays out one interleaved device, because
// segment k reads L_k consecutive frames of the raw input ring; on one that does, every channel is
// laid out on its own
int bfhip_nupc_set_format(bfhip_nupc *n, int io, int ch, const bfhip_format *f) {
    if (!n || !f || io < 0 || io > 1 || ch < 0 || ch >= (io ? n->n_out : n->n_in)) return nfail(BFHIP_EINVAL, "nupc_set_format: bad argument");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_format after finalize");
    n->fmt[io][ch] = *f;
    return BFHIP_OK;
}

int bfhip_nupc_set_buffer_bytes(bfhip_nupc *n, int io, long bytes) {
    if (!n || io < 0 || io > 1 || bytes < 1) return nfail(BFHIP_EINVAL, "nupc_set_buffer_bytes: bad argument");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_buffer_bytes after finalize");
    n->buf_bytes[io] = bytes;
    return BFHIP_OK;
}

long bfhip_nupc_buffer_bytes(const bfhip_nupc *n, int io) {
    if (!n || io < 0 || io > 1) return nfail(BFHIP_EINVAL, "nupc_buffer_bytes: bad argument");
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc_buffer_bytes before finalize");
    return (long)n->period_bytes[io];
}

// dither_init for the listed outputs (bfhip_engine_enable_dither's checks; max_samples_per_loop =
// L0): the tables are made here, uploaded at finalize
int bfhip_nupc_enable_dither(bfhip_nupc *n, const int out_channels[], int n_ch, int sample_rate, int max_size) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_enable_dither after finalize");
    if (!out_channels || n_ch < 1 || sample_rate < 1) return nfail(BFHIP_EINVAL, "nupc_enable_dither: bad argument");
    std::vector<int> chs(out_channels, out_channels + n_ch);
    for (int i = 0; i < n_ch; i++) {
        if (chs[i] < 0 || chs[i] >= n->n_out) return nfail(BFHIP_EINVAL, "nupc_enable_dither: output channel " + std::to_string(chs[i]));
        if (i > 0 && chs[i] <= chs[i - 1]) return nfail(BFHIP_EINVAL, "nupc_enable_dither: channels must be ascending");
        if (n->fmt[1][chs[i]].isfloat)
            return nfail(BFHIP_EINVAL, "cannot dither floating point format (output " + std::to_string(chs[i]) + ")");
    }
    int spacing = 0;
    std::vector<int8_t> table;
    const std::string msg = dither_make_table(n_ch, sample_rate, max_size, n->seg[0].L, &spacing, &table);
    if (!msg.empty()) return nfail(BFHIP_EINVAL, msg);
    n->dither_spacing = spacing;
    n->dither_table.swap(table);
    n->dither_ch = chs;
    return BFHIP_OK;
}

int bfhip_nupc_set_safety_limit(bfhip_nupc *n, double limit) { if (!n) return BFHIP_EINVAL; n->safety_limit = limit; return BFHIP_OK; }

// one filter = one impulse response from an input to an output (taps in host memory, realsize
// wide); it is cut along the segment boundaries and loaded into every segment's engine
int bfhip_nupc_add_filter(bfhip_nupc *n, int in_ch, int out_ch, const void *taps, long n_taps,
                          double in_scale, double out_scale) {
    if (!n || !taps || n_taps < 1 || in_ch < 0 || in_ch >= n->n_in || out_ch < 0 || out_ch >= n->n_out) return nfail(BFHIP_EINVAL, "nupc_add_filter: bad argument");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_add_filter after finalize");
    int set0 = -1;
    for (auto &s : n->seg) {
        const long avail = n_taps - s.off;
        const long cap = (long)s.L * s.N;
        const long take = avail < 0 ? 0 : (avail > cap ? cap : avail);
        std::vector<unsigned char> zero;
        const void *src = (const unsigned char *)taps + (size_t)s.off * n->rs;
        if (take == 0) { zero.assign((size_t)n->rs, 0); src = zero.data(); }
        const int c = bfhip_engine_add_coeff(s.eng, src, take == 0 ? 1 : (int)take, 1.0, take == 0 ? 1 : 0);
        if (c < 0) return nfail(c, std::string("nupc_add_filter: ") + bfhip_last_error());
        if (set0 >= 0 && c != set0) return nfail(BFHIP_EINVAL, "nupc_add_filter: the segment engines disagree on coefficient numbering");
        set0 = c;
        s.eng_set.push_back(Asg());
        s.n_blocks.push_back({take == 0 ? 1 : (int)((take + s.L - 1) / s.L)});
        // the engines emit plain reals: the output format's 1/scale is applied at the emit step
        const int r = bfhip_engine_add_filter(s.eng, 1, &in_ch, &in_scale, 0, nullptr, nullptr, 1, &out_ch, &out_scale, c, 0, 0);
        if (r < 0) return nfail(r, std::string("nupc_add_filter: ") + bfhip_last_error());
    }
    n->coeff.push_back({set0});
    n->out_scale.push_back(out_scale);
    n->live.push_back(Asg());
    n->queued.push_back(Asg{-1, NAN});
    return BFHIP_OK;
}

// another impulse response for a filter (before finalize): loaded into every segment engine as a
// set of its own with the segment's full partition count, so that update_coeff can rewrite all of it
int bfhip_nupc_add_coeff(bfhip_nupc *n, int filter, const void *taps, long n_taps) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_add_coeff after finalize");
    if (filter < 0 || filter >= (int)n->coeff.size() || !taps || n_taps < 1 || n_taps > bfhip_nupc_taps(n))
        return nfail(BFHIP_EINVAL, "nupc_add_coeff: bad argument");
    OWNER(n);
    int c0 = -1;
    for (auto &s : n->seg) {
        const long cap = (long)s.L * s.N;
        const long avail = n_taps - s.off;
        const long take = avail < 0 ? 0 : (avail > cap ? cap : avail);
        std::vector<unsigned char> zero;
        const void *src = (const unsigned char *)taps + (size_t)s.off * n->rs;
        if (take == 0) { zero.assign((size_t)n->rs, 0); src = zero.data(); }
        const int c = bfhip_engine_add_coeff(s.eng, src, take == 0 ? 1 : (int)take, 1.0, s.N);
        if (c < 0) return nfail(c, std::string("nupc_add_coeff: ") + bfhip_last_error());
        if (c0 >= 0 && c != c0) return nfail(BFHIP_EINVAL, "nupc_add_coeff: the segment engines disagree on coefficient numbering");
        c0 = c;
    }
    for (auto &s : n->seg) s.n_blocks[filter].push_back(s.N);
    n->coeff[filter].push_back(c0);
    return (int)n->coeff[filter].size() - 1;
}

static int nupc_finalize_impl(bfhip_nupc *n);
namespace { int seg_assign(Seg &s, const bfhip_nupc *n, const std::vector<Asg> &asg); }

int bfhip_nupc_finalize(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return BFHIP_OK;
    // half-built state is cleaned up by bfhip_nupc_destroy only: a failed finalize is not retried
    if (n->finalize_failed) return nfail(BFHIP_ESTATE, "nupc_finalize failed before: destroy this convolver");
    const int r = nupc_finalize_impl(n);
    if (r != BFHIP_OK) { n->finalize_failed = true; n->finalized = false; }
    return r;
}

// a side that declared its buffer: every channel's L0 samples lie inside it and no byte belongs to
// two channels (a byte map of the buffer)
static int nupc_check_layout(const bfhip_nupc *n, int io) {
    const size_t total = (size_t)n->buf_bytes[io], L0 = (size_t)n->seg[0].L;
    std::vector<unsigned char> owned(total, 0);
    for (size_t ch = 0; ch < n->fmt[io].size(); ch++) {
        const bfhip_format &f = n->fmt[io][ch];
        const std::string who = std::string("nupc: ") + (io ? "output " : "input ") + std::to_string(ch);
        if (f.sample_spacing < 1 || f.byte_offset < 0 || f.bytes < 1)
            return nfail(BFHIP_EINVAL, who + ": sample_spacing must be >= 1, byte_offset >= 0 and bytes >= 1");
        const size_t stride = (size_t)f.sample_spacing * f.bytes;
        if ((size_t)f.byte_offset + (L0 - 1) * stride + f.bytes > total)
            return nfail(BFHIP_EINVAL, who + ": its last sample lies past the side's buffer of " + std::to_string(total) + " bytes");
        for (size_t t = 0; t < L0; t++)
            for (int b = 0; b < f.bytes; b++) {
                unsigned char &o = owned[(size_t)f.byte_offset + t * stride + b];
                if (o) return nfail(BFHIP_EINVAL, who + ": its samples overlap another channel's in the side's buffer");
                o = 1;
            }
    }
    return BFHIP_OK;
}

static int nupc_finalize_impl(bfhip_nupc *n) {
    OWNER(n);
    for (int io = 0; io < 2; io++) {
        for (size_t ch = 0; ch < n->sd[io].size(); ch++) {
            if (n->sd[io][ch] == BFHIP_UNDEFINED_SUBDELAY) continue;
            if (n->sdf_length <= 0)
                return nfail(BFHIP_EINVAL, std::string("nupc: ") + (io ? "output " : "input ") + std::to_string(ch) +
                             " has a sub-sample delay but bfhip_nupc_enable_subdelay was not called");
            n->sd_use[io] = true;
        }
        if (n->sd_use[io] && n->sd[io].size() > (size_t)kSdChannels)
            return nfail(BFHIP_EINVAL, "nupc: a side that uses sub-sample delay can have at most " + std::to_string(kSdChannels) + " channels");
        if (!n->sd_use[io]) continue;
        // a channel without a filter follows the filtered ones sdf_length whole frames later, through
        // its integer delay line (dai.c:205-215, 230-243); a fixed line stays fixed
        for (size_t ch = 0; ch < n->sd[io].size(); ch++) {
            if (n->sd[io][ch] != BFHIP_UNDEFINED_SUBDELAY) continue;
            NupcDelay &d = n->dl[io][ch];
            d.extra = n->sdf_length;
            if (d.maxdelay > 0 && d.req > d.maxdelay) d.req = d.maxdelay;
            if (d.maxdelay == 0) d.req = 0;
            d.req += d.extra;
            if (d.maxdelay >= 0) d.maxdelay += d.extra;
        }
    }
    NCHK(hipSetDevice(n->device));
    int prio_least = 0, prio_greatest = 0;
    NCHK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    NCHK(hipStreamCreateWithPriority(&n->stream, hipStreamNonBlocking, prio_greatest));
    NCHK(hipEventCreateWithFlags(&n->ev_in, hipEventDisableTiming));
    if (const char *bg = getenv("BFHIP_NUPC_BACKGROUND")) n->background = atoi(bg) != 0;
    const int L0 = n->seg[0].L, Lmax = n->seg.back().L;
    for (int io = 0; io < 2; io++) {
        const int c = io ? n->n_out : n->n_in;
        if (n->buf_bytes[io]) {
            // the input side goes through the conversion kernel's argument block (NupcSdVals)
            if (io == BFHIP_IN && c > kSdChannels)
                return nfail(BFHIP_EINVAL, "nupc: an input side that declares its buffer can have at most " + std::to_string(kSdChannels) + " channels");
            { const int r = nupc_check_layout(n, io); if (r < 0) return r; }
            n->period_bytes[io] = (size_t)n->buf_bytes[io];
            continue;
        }
        const int spacing = n->fmt[io][0].sample_spacing, bytes = n->fmt[io][0].bytes;
        for (int ch = 0; ch < c; ch++)
            if (n->fmt[io][ch].sample_spacing != spacing || n->fmt[io][ch].bytes != bytes)
                return nfail(BFHIP_EINVAL, "nupc: all channels of a side must share one interleaved frame layout");
        n->frame_bytes[io] = (size_t)spacing * bytes;
        n->period_bytes[io] = (size_t)L0 * n->frame_bytes[io];
    }
    n->in_real = n->sd_use[0] || n->buf_bytes[0];
    long reach = 0;
    for (auto &s : n->seg) reach = std::max(reach, s.off + 2L * s.L);
    int A = 1;
    while (A < reach + L0) A <<= 1;
    n->A = A;
    NCHK(bfhip_internal_dev_alloc((void **)&n->d_acc, (size_t)A * n->n_out * n->rs));
    NCHK(hipMemset(n->d_acc, 0, (size_t)A * n->n_out * n->rs));
    // two periods of the longest segment: its forward transform may still be reading one while
    // the next is being filled
    n->in_frames = 2 * Lmax;
    if (n->buf_bytes[0]) {
        NCHK(bfhip_internal_dev_alloc((void **)&n->d_stage, n->period_bytes[0]));
        NCHK(hipMemset(n->d_stage, 0, n->period_bytes[0]));
    } else {
        NCHK(bfhip_internal_dev_alloc((void **)&n->d_in, (size_t)n->in_frames * n->frame_bytes[0]));
        NCHK(hipMemset(n->d_in, 0, (size_t)n->in_frames * n->frame_bytes[0]));
    }
    // bytes no output channel owns are never written: they stay zero
    NCHK(bfhip_internal_dev_alloc((void **)&n->d_rawout, n->period_bytes[1]));
    NCHK(hipMemset(n->d_rawout, 0, n->period_bytes[1]));
    std::vector<DevFormat> df(n->n_out);
    n->ramp.resize(n->n_out);
    std::vector<DevOverflow> ov(n->n_out);
    for (int ch = 0; ch < n->n_out; ch++) {
        const bfhip_format &f = n->fmt[1][ch];
        df[ch].isfloat = f.isfloat; df[ch].swap = f.swap; df[ch].bytes = f.bytes; df[ch].sbytes = f.sbytes;
        df[ch].sample_spacing = f.sample_spacing; df[ch].byte_offset = f.byte_offset; df[ch].alt = nullptr;
        n->ramp[ch] = NupcGain{1.0 / f.scale, n->gain[ch], n->gain[ch], 0, 0};   // bfrun.c:1850: inv * g
        ov[ch] = over_initial(f);
    }
    NCHK(bfhip_internal_dev_alloc((void **)&n->d_fmt_out, df.size() * sizeof(DevFormat)));
    NCHK(hipMemcpy(n->d_fmt_out, df.data(), df.size() * sizeof(DevFormat), hipMemcpyHostToDevice));
    NCHK(bfhip_internal_dev_alloc((void **)&n->d_gain, n->ramp.size() * sizeof(NupcGain)));
    NCHK(hipMemcpy(n->d_gain, n->ramp.data(), n->ramp.size() * sizeof(NupcGain), hipMemcpyHostToDevice));
    NCHK(bfhip_internal_dev_alloc((void **)&n->d_over, ov.size() * sizeof(DevOverflow)));
    NCHK(hipMemcpy(n->d_over, ov.data(), ov.size() * sizeof(DevOverflow), hipMemcpyHostToDevice));
    NCHK(bfhip_internal_dev_alloc((void **)&n->d_status, sizeof(int)));
    NCHK(hipMemset(n->d_status, 0, sizeof(int)));
    NCHK(bfhip_internal_dev_alloc((void **)&n->d_arrive, sizeof(unsigned int)));
    NCHK(hipMemset(n->d_arrive, 0, sizeof(unsigned int)));
    NCHK(bfhip_internal_pin_alloc((void **)&n->h_status, sizeof(int), hipHostMallocDefault));
    NCHK(bfhip_internal_pin_alloc((void **)&n->h_in, n->period_bytes[0], hipHostMallocDefault));
    NCHK(bfhip_internal_pin_alloc((void **)&n->h_out, n->period_bytes[1], hipHostMallocDefault));
    NCHK(bfhip_internal_pin_alloc((void **)&n->h_over, (size_t)n->n_out * sizeof(DevOverflow), hipHostMallocDefault));
    *n->h_status = 0;
    NCHK(bfhip_internal_pin_alloc((void **)&n->h_gain, (size_t)n->n_out * sizeof(NupcGain), hipHostMallocDefault));
    NCHK(hipEventCreateWithFlags(&n->ev_gain, hipEventDisableTiming));
    NCHK(hipEventRecord(n->ev_gain, n->stream));
    n->gain_dirty = false;
    if (!n->dither_ch.empty()) {
        std::vector<int> slot(n->n_out, -1), rank(n->dither_ch.size());
        for (size_t i = 0; i < n->dither_ch.size(); i++) {
            if (n->fmt[1][n->dither_ch[i]].isfloat)
                return nfail(BFHIP_EINVAL, "cannot dither floating point format (output " + std::to_string(n->dither_ch[i]) + ")");
            slot[n->dither_ch[i]] = (int)i;
            rank[i] = (int)i;
        }
        NCHK(bfhip_internal_dev_alloc((void **)&n->d_dither_slot, slot.size() * sizeof(int)));
        NCHK(hipMemcpy(n->d_dither_slot, slot.data(), slot.size() * sizeof(int), hipMemcpyHostToDevice));
        NCHK(dither_upload_tables(n->dither_table, n->dither_spacing, rank, n->rs, &n->d_dither_table, &n->d_randmap,
                                  &n->d_dither_state));
        NCHK(bfhip_internal_dev_alloc(&n->d_dither_stage, n->dither_ch.size() * L0 * n->rs));
    }
    for (int io = 0; io < 2; io++)
        for (size_t ch = 0; ch < n->dl[io].size(); ch++) {
            NupcDelay &d = n->dl[io][ch];
            const size_t bytes = d.init(L0, n->fmt[io][ch].bytes);    // delay_allocate_buffer, the channel's own sample size
            if (bytes == 0) continue;
            NCHK(bfhip_internal_dev_alloc((void **)&d.arena, bytes));
            NCHK(hipMemset(d.arena, 0, bytes));
        }
    if (n->sd_use[0] || n->sd_use[1]) {
        const std::vector<unsigned char> bank = sd_make_bank(n->sdf_length, n->rs);
        NCHK(bfhip_internal_dev_alloc(&n->d_sd_bank, bank.size()));
        NCHK(hipMemcpy(n->d_sd_bank, bank.data(), bank.size(), hipMemcpyHostToDevice));
        for (int io = 0; io < 2; io++) {
            if (!n->sd_use[io]) continue;
            const size_t bytes = n->sd[io].size() * n->sd_bs * n->rs;
            NCHK(bfhip_internal_dev_alloc(&n->d_sd_hist[io], bytes));
            NCHK(hipMemset(n->d_sd_hist[io], 0, bytes));
        }
    }
    if (n->in_real) {
        std::vector<DevFormat> dfi(n->n_in);
        for (int ch = 0; ch < n->n_in; ch++) {
            const bfhip_format &f = n->fmt[0][ch];
            if (!n->buf_bytes[0] && (f.byte_offset < 0 || (size_t)f.byte_offset + f.bytes > n->frame_bytes[0]))
                return nfail(BFHIP_EINVAL, "nupc: sub-sample delay on a side with a channel whose samples lie outside the raw frame");
            dfi[ch].isfloat = f.isfloat; dfi[ch].swap = f.swap; dfi[ch].bytes = f.bytes; dfi[ch].sbytes = f.sbytes;
            dfi[ch].sample_spacing = f.sample_spacing; dfi[ch].byte_offset = f.byte_offset; dfi[ch].alt = nullptr;
        }
        NCHK(bfhip_internal_dev_alloc((void **)&n->d_fmt_in, dfi.size() * sizeof(DevFormat)));
        NCHK(hipMemcpy(n->d_fmt_in, dfi.data(), dfi.size() * sizeof(DevFormat), hipMemcpyHostToDevice));
        NCHK(bfhip_internal_dev_alloc((void **)&n->d_in_real, (size_t)n->in_frames * n->n_in * n->rs));
        NCHK(hipMemset(n->d_in_real, 0, (size_t)n->in_frames * n->n_in * n->rs));
    }
    n->can_switch = n->gain_reserve;
    for (auto &c : n->coeff) n->can_switch = n->can_switch || c.size() > 1;
    if (n->can_switch) {
        NCHK(bfhip_internal_dev_alloc((void **)&n->d_acc2, (size_t)A * n->n_out * n->rs));
        NCHK(hipMemset(n->d_acc2, 0, (size_t)A * n->n_out * n->rs));
    }
    for (auto &s : n->seg) {
        for (int ch = 0; ch < n->n_in; ch++) {
            bfhip_format f = n->fmt[0][ch];
            if (n->in_real) {
                // the ring of converted (and filtered) reals; the format's scale stays where it is
                // applied today, in the engines' filter scales
                f.isfloat = 1; f.swap = 0; f.bytes = f.sbytes = n->rs;
                f.sample_spacing = n->n_in; f.byte_offset = ch * n->rs;
            }
            ECHK(bfhip_engine_set_format(s.eng, BFHIP_IN, ch, &f));
        }
        for (int ch = 0; ch < n->n_out; ch++) {
            bfhip_format f;
            f.isfloat = 1; f.swap = 0; f.bytes = f.sbytes = n->rs; f.scale = 1.0;
            f.sample_spacing = n->n_out; f.byte_offset = ch * n->rs;
            ECHK(bfhip_engine_set_format(s.eng, BFHIP_OUT, ch, &f));
        }
        { const int r = seg_assign(s, n, n->live); if (r < 0) return r; }   // initial gains other than 1
        ECHK(bfhip_engine_set_overlap(s.eng, 0));          // a segment's kernels are ordered on ONE stream
        ECHK(bfhip_engine_finalize(s.eng));
        const long slack = s.off - ((long)s.L - L0);       // >= 0, checked at create
        const long room = (long)s.L - L0;                  // its next block is launched L frames later
        s.delay_steps = n->background ? (int)(std::min(slack, room) / L0) : 0;
        if (s.delay_steps > 0) {
            NCHK(hipStreamCreateWithPriority(&s.stream, hipStreamNonBlocking, prio_least));
            NCHK(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
            NCHK(hipEventCreateWithFlags(&s.ev_consumed, hipEventDisableTiming));
        }
        ECHK(bfhip_engine_set_stream(s.eng, s.delay_steps > 0 ? s.stream : n->stream));
        ECHK(bfhip_engine_set_status_dev(s.eng, n->d_status));
        NCHK(bfhip_internal_dev_alloc((void **)&s.d_out, (size_t)s.L * n->n_out * n->rs));
        if (n->can_switch) {
            NCHK(bfhip_internal_dev_alloc((void **)&s.d_out2, (size_t)s.L * n->n_out * n->rs));
            // n_out spectra of L complex numbers (rounded up to the MAC's output groups)
            NCHK(bfhip_internal_dev_alloc((void **)&s.d_z, (size_t)((n->n_out + 7) / 8 * 8) * s.L * 2 * n->rs));
        }
    }
    if (n->upd_reserve) {
        // everything the asynchronous rewrite touches, so that it allocates nothing on the audio path
        const size_t bytes = (size_t)bfhip_nupc_taps(n) * n->rs;
        NCHK(bfhip_internal_pin_alloc((void **)&n->h_upd, bytes, hipHostMallocDefault));
        memset(n->h_upd, 0, bytes);
        NCHK(bfhip_internal_dev_alloc((void **)&n->d_upd, bytes));
        NCHK(hipMemset(n->d_upd, 0, bytes));
        NCHK(bfhip_internal_pin_alloc((void **)&n->h_upd_bad, n->seg.size() * sizeof(int), hipHostMallocDefault));
        memset(n->h_upd_bad, 0, n->seg.size() * sizeof(int));
        NCHK(hipStreamCreateWithPriority(&n->upd_stream, hipStreamNonBlocking, prio_least));
        NCHK(hipEventCreateWithFlags(&n->ev_upd_load, hipEventDisableTiming));
        NCHK(hipEventCreateWithFlags(&n->ev_upd_main, hipEventDisableTiming));
        for (auto &s : n->seg) {
            if (s.delay_steps > 0) NCHK(hipEventCreateWithFlags(&s.ev_upd, hipEventDisableTiming));
            ECHK(bfhip_internal_engine_reserve_update(s.eng));
        }
        n->upd_bad.resize(n->coeff.size());
        for (size_t f = 0; f < n->coeff.size(); f++) n->upd_bad[f].assign(n->coeff[f].size(), 0);
    }
    if (n->eq_reserve) {
        NCHK(eq_render_alloc(n->eq, n->rs, n->eq_reserve));
        if (n->eq_min.reserved) NCHK(eq_minphase_alloc(n->eq_min, n->eq));
        NCHK(hipEventCreateWithFlags(&n->ev_eq, hipEventDisableTiming));
    }
    n->finalized = true;
    return BFHIP_OK;
}

}  // extern "C"

namespace {

int nupc_accumulate(bfhip_nupc *n, const Seg &s, unsigned long long pos, void *acc, void *acc2) {
    const size_t cnt = (size_t)s.L * n->n_out;
    if (n->rs == 4)
        hipLaunchKernelGGL(nupc_accumulate_kernel<float>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, n->stream,
                           (float *)acc, (const float *)s.d_out, (float *)acc2, (const float *)s.d_out2, pos, n->A, n->n_out, s.L);
    else
        hipLaunchKernelGGL(nupc_accumulate_kernel<double>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, n->stream,
                           (double *)acc, (const double *)s.d_out, (double *)acc2, (const double *)s.d_out2, pos, n->A, n->n_out, s.L);
    NCHK(hipGetLastError());
    return BFHIP_OK;
}

// a block of a staggered switch that ran under both assignments: blended into the live ring
int nupc_accumulate_fade(bfhip_nupc *n, const Seg &s, unsigned long long pos, void *acc, long long t_k, int F) {
    const size_t cnt = (size_t)s.L * n->n_out;
    const long long rel0 = (long long)pos - t_k;
    if (n->rs == 4)
        hipLaunchKernelGGL(nupc_accumulate_fade_kernel<float>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, n->stream,
                           (float *)acc, (const float *)s.d_out, (const float *)s.d_out2, pos, n->A, n->n_out, s.L, rel0, F);
    else
        hipLaunchKernelGGL(nupc_accumulate_fade_kernel<double>, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, n->stream,
                           (double *)acc, (const double *)s.d_out, (const double *)s.d_out2, pos, n->A, n->n_out, s.L, rel0, F);
    NCHK(hipGetLastError());
    return BFHIP_OK;
}

// this period's delay / mute step of one side on its raw block; no launch if no channel of the
// side is muted or has a delay line with work
int nupc_delay_side(bfhip_nupc *n, int io, uint8_t *raw) {
    // (a side with a declared buffer had every channel's samples checked against it at finalize)
    for (size_t ch = 0; ch < n->dl[io].size() && !n->buf_bytes[io]; ch++) {
        const bfhip_format &f = n->fmt[io][ch];
        if ((n->dl[io][ch].arena || n->dl[io][ch].muted) &&
            (f.byte_offset < 0 || (size_t)f.byte_offset + f.bytes > n->frame_bytes[io]))
            return nfail(BFHIP_EINVAL, "nupc: delay / mute on a channel whose samples lie outside the raw frame");
    }
    auto &jobs = n->dl_jobs;
    jobs.clear();
    for (size_t ch = 0; ch < n->dl[io].size(); ch++) {
        NupcDelayJob jb;
        if (!n->dl[io][ch].step(jb)) continue;
        const bfhip_format &f = n->fmt[io][ch];
        jb.byte_offset = f.byte_offset;
        jb.ss = f.bytes;
        jb.stride = f.sample_spacing * f.bytes;
        jobs.push_back(jb);
    }
    for (size_t first = 0; first < jobs.size(); first += kDelayJobs) {
        const int cnt = (int)std::min(jobs.size() - first, (size_t)kDelayJobs);
        NupcDelayJobs args;
        memset(&args, 0, sizeof(args));
        std::copy(jobs.begin() + first, jobs.begin() + first + cnt, args.j);
        hipLaunchKernelGGL(nupc_delay_kernel, dim3(cnt), dim3(256), 0, n->stream, args, raw, n->seg[0].L,
                           io == BFHIP_IN ? 1 : 0);
        NCHK(hipGetLastError());
    }
    return BFHIP_OK;
}

// this period's sub-delay arguments of one side: the values in force now
template <typename T> NupcSd<T> nupc_sd_args(const bfhip_nupc *n, int io) {
    NupcSd<T> a;
    memset(&a, 0, sizeof(a));
    memset(a.vals.v, -100, sizeof(a.vals.v));                     // no channel has a filter
    if (!n->sd_use[io]) return a;
    a.bank = (const T *)n->d_sd_bank;
    a.hist = (T *)n->d_sd_hist[io];
    a.bs = n->sd_bs; a.flen = n->sd_flen; a.tile = std::min(n->seg[0].L, kSdTile);
    for (size_t ch = 0; ch < n->sd[io].size(); ch++) a.vals.v[ch] = (signed char)n->sd[io][ch];
    return a;
}
size_t nupc_sd_smem(const bfhip_nupc *n, int io) {
    return n->sd_use[io] ? nupc_sd_lds(n->sd_bs, n->sd_flen, std::min(n->seg[0].L, kSdTile), n->rs) : 0;
}

// input side with sub-delay or a declared buffer: the period's raw samples (delayed and muted
// already; the raw ring's slot, or the stage) become the reals of slot wpos of the ring the segment
// engines read
int nupc_subdelay_in(bfhip_nupc *n, const uint8_t *raw_slot, size_t wpos) {
    const int L0 = n->seg[0].L;
    uint8_t *real = n->d_in_real + wpos * (size_t)n->n_in * n->rs;
    if (n->rs == 4)
        hipLaunchKernelGGL(nupc_subdelay_in_kernel<float>, dim3(n->n_in), dim3(256), nupc_sd_smem(n, 0), n->stream, raw_slot,
                           n->d_fmt_in, (float *)real, n->n_in, L0, nupc_sd_args<float>(n, 0));
    else
        hipLaunchKernelGGL(nupc_subdelay_in_kernel<double>, dim3(n->n_in), dim3(256), nupc_sd_smem(n, 0), n->stream, raw_slot,
                           n->d_fmt_in, (double *)real, n->n_in, L0, nupc_sd_args<double>(n, 0));
    NCHK(hipGetLastError());
    return BFHIP_OK;
}

// one emit launch: the four kernels (dither or not, sub-delay on the output side or not) share
// their leading arguments
template <typename T, bool SD>
void nupc_emit_launch(bfhip_nupc *n, void *acc_old, void *acc_new, unsigned long long opos, long long rel0, void *rawout_dev) {
    const int L0 = n->seg[0].L;
    const NupcSd<T> sd = nupc_sd_args<T>(n, 1);
    const size_t smem = SD ? nupc_sd_smem(n, 1) : 0;
    if (!n->dither_ch.empty())
        hipLaunchKernelGGL((nupc_emit_dither_kernel<T, SD>), dim3(n->n_out), dim3(256), smem, n->stream, (T *)acc_old,
                           (T *)acc_new, opos, n->A, n->n_out, L0, rel0, n->sw_F, n->d_fmt_out, n->d_gain,
                           n->d_over, (uint8_t *)rawout_dev, n->safety_limit, n->d_status, n->d_arrive, n->h_status,
                           n->d_dither_slot, (T *)n->d_dither_stage, (DitherState<T> *)n->d_dither_state,
                           n->d_dither_table, (int)n->dither_table.size(), (const T *)n->d_randmap + 256, sd);
    else
        hipLaunchKernelGGL((nupc_emit_kernel<T, SD>), dim3(n->n_out), dim3(256), smem, n->stream, (T *)acc_old, (T *)acc_new,
                           opos, n->A, n->n_out, L0, rel0, n->sw_F, n->d_fmt_out, n->d_gain, n->d_over,
                           (uint8_t *)rawout_dev, n->safety_limit, n->d_status, n->d_arrive, n->h_status, sd);
}

// point a segment engine's filters at an assignment (a plan rebuild at its next call if any moved)
int seg_assign(Seg &s, const bfhip_nupc *n, const std::vector<Asg> &asg) {
    for (size_t f = 0; f < asg.size(); f++) {
        if (s.eng_set[f] == asg[f]) continue;
        if (s.eng_set[f].set != asg[f].set) ECHK(bfhip_engine_set_coeff(s.eng, (int)f, n->coeff[f][asg[f].set]));
        // an output scale dirties the plan only (no private ring); out_scale * 1.0 is out_scale
        if (s.eng_set[f].gain != asg[f].gain)
            ECHK(bfhip_engine_set_scale(s.eng, (int)f, BFHIP_OUT, 0, n->out_scale[f] * asg[f].gain));
        s.eng_set[f] = asg[f];
    }
    return BFHIP_OK;
}

// one block of a segment: under one assignment into d_out, or (dual) the input transform once and
// the MAC + inverse transform under the old assignment into d_out and under the new one into
// d_out2.  The engine keeps whichever assignment it ran last, so a run of dual blocks costs one
// plan rebuild each, not two.
int seg_run(bfhip_nupc *n, Seg &s, const uint8_t *in, int mode /* 0 old, 1 new, 2 both */) {
    const std::vector<Asg> &old_asg = n->sw ? n->sw_old : n->live;
    if (mode != 2) {
        { const int r = seg_assign(s, n, mode == 0 ? old_asg : n->live); if (r < 0) return r; }
        ECHK(bfhip_engine_block_dev(s.eng, in, s.d_out));
        return BFHIP_OK;
    }
    const bool new_first = s.eng_set == n->live;
    ECHK(bfhip_engine_inputs_dev(s.eng, in));
    for (int k = 0; k < 2; k++) {
        const bool is_new = (k == 0) == new_first;
        { const int r = seg_assign(s, n, is_new ? n->live : old_asg); if (r < 0) return r; }
        ECHK(bfhip_engine_mac_dev(s.eng, s.d_z));
        ECHK(bfhip_engine_outputs_dev(s.eng, s.d_z, 0, n->n_out, is_new ? s.d_out2 : s.d_out));
    }
    ECHK(bfhip_engine_advance(s.eng));
    return BFHIP_OK;
}

// the queued requests become one switch whose first output block is the one starting at t_req
void nupc_commit(bfhip_nupc *n, unsigned long long t_req) {
    std::vector<Asg> asg = n->live;
    for (size_t f = 0; f < asg.size(); f++) {
        if (n->queued[f].set >= 0) asg[f].set = n->queued[f].set;
        if (!std::isnan(n->queued[f].gain)) asg[f].gain = n->queued[f].gain;
    }
    std::fill(n->queued.begin(), n->queued.end(), Asg{-1, NAN});
    if (asg == n->live) return;                                   // nothing changes
    const unsigned long long L0 = (unsigned long long)n->seg[0].L;
    n->t_seg.resize(n->seg.size());
    if (n->switch_mode == BFHIP_NUPC_SWITCH_STAGGERED) {
        // segment k switches at the first frame its next launch writes: t_k = e_k - L_k + off_k >= t_req
        // (off_k >= L_k - L0), t_0 = t_req.  A hard switch needs no block under both assignments: every
        // segment simply runs the new one from its next launch on, and there is nothing to be busy with.
        for (size_t k = 0; k < n->seg.size(); k++) {
            const unsigned long long L = (unsigned long long)n->seg[k].L;
            const unsigned long long e = (t_req + L0 + L - 1) / L * L;
            n->t_seg[k] = (long long)(e - L) + n->seg[k].off;
        }
        n->sw_old = n->live;
        n->live = asg;
        n->t_sw = (long long)t_req;
        n->sw_F = n->crossfade;
        n->sw_stag = true;
        n->sw = n->sw_F > 0;
        return;
    }
    long long t_sw = (long long)t_req;
    for (const Seg &s : n->seg) {
        // segment k's first block launched from now on computes frames from e_k - L_k + off_k on
        const unsigned long long L = (unsigned long long)s.L;
        const unsigned long long e = (t_req + L0 + L - 1) / L * L;
        t_sw = std::max(t_sw, (long long)(e - L) + s.off);
    }
    n->sw_old = n->live;
    n->live = asg;
    n->sw = true;
    n->t_sw = t_sw;
    n->sw_F = n->crossfade;
    n->old_hi = t_sw;          // what was launched before wrote frames < t_sw only
    n->sw_stag = false;
    std::fill(n->t_seg.begin(), n->t_seg.end(), t_sw);
}

// a staggered switch after the block call that received `end` frames: does some segment's next
// block start before the segment's own fade ends?
bool nupc_stagger_left(const bfhip_nupc *n, unsigned long long end) {
    for (size_t k = 0; k < n->seg.size(); k++) {
        const unsigned long long L = (unsigned long long)n->seg[k].L;
        if ((long long)(end / L * L) + n->seg[k].off < n->t_seg[k] + n->sw_F) return true;
    }
    return false;
}

// after the block call that emitted frames up to `end`: is old-assignment work or fade left?
bool nupc_switch_left(const bfhip_nupc *n, unsigned long long end) {
    const long long old_end = n->t_sw + n->sw_F;                  // old output is needed below this frame
    if ((long long)end < std::max(n->old_hi, old_end)) return true;
    for (const Seg &s : n->seg) {
        const unsigned long long L = (unsigned long long)s.L;
        const unsigned long long next = (end / L + 1) * L;
        if ((long long)(next - L) + s.off < old_end) return true;
    }
    return false;
}

// ---- asynchronous set rewrite

// has every piece of the rewrite in flight completed?  hipEventQuery only: never blocks.  On
// completion the segment engines' non-finite flags (pinned, written behind each preparation)
// become the rewrite's result.
int upd_poll(bfhip_nupc *n) {
    if (!n->upd_inflight) return BFHIP_OK;
    NCHK(hipSetDevice(n->device));
    for (size_t k = 0; k < n->seg.size() + 2; k++) {
        const hipEvent_t ev = k == 0 ? n->ev_upd_load : k == 1 ? n->ev_upd_main : n->seg[k - 2].ev_upd;
        if (!ev) continue;                                        // a main-stream segment: ev_upd_main covers it
        const hipError_t e = hipEventQuery(ev);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); return BFHIP_OK; }
        if (e != hipSuccess) return nfail(BFHIP_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
    }
    int bad = 0;
    for (size_t k = 0; k < n->seg.size(); k++) bad |= ((volatile int *)n->h_upd_bad)[k];
    n->upd_result = bad ? BFHIP_EINVAL : n->upd_failed ? BFHIP_EHIP : BFHIP_OK;
    n->upd_bad[n->upd_filter][n->upd_set] = bad || n->upd_failed ? 1 : 0;
    n->upd_inflight = false;
    return BFHIP_OK;
}

// enqueue the upload and every segment engine's preparation of set (filter, coeff); no host wait,
// no allocation.  Host source: `taps` is the pinned staging buffer or is copied into it.  Device
// source: the loader (and the main stream, for its own slices) waits on ready_event.
// eq: the taps are rendered from this curve (in mode eq_mode) into eq.taps on the loader stream first,
// and ev_eq is the ready event (the caller passes taps = eq.taps, on_device).
int upd_enqueue(bfhip_nupc *n, int filter, int coeff, const void *taps, bool on_device, long n_taps, void *ready_event);
static hipError_t eq_launch(const bfhip_nupc *n, const EqBands &b, long taps, int mode) {
    if (mode == BFHIP_EQ_MINIMUM)
        return n->rs == 4 ? eq_minphase_launch<float>(n->eq, n->eq_min, b, taps, n->upd_stream)
                          : eq_minphase_launch<double>(n->eq, n->eq_min, b, taps, n->upd_stream);
    return n->rs == 4 ? eq_render_launch<float>(n->eq, b, taps, n->upd_stream) : eq_render_launch<double>(n->eq, b, taps, n->upd_stream);
}
int upd_start(bfhip_nupc *n, int filter, int coeff, const void *taps, bool on_device, long n_taps, void *ready_event,
              const EqBands *eq = nullptr, int eq_mode = BFHIP_EQ_LINEAR) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (filter < 0 || filter >= (int)n->coeff.size() || coeff < 0 || coeff >= (int)n->coeff[filter].size() ||
        !taps || n_taps < 1 || n_taps > bfhip_nupc_taps(n))
        return nfail(BFHIP_EINVAL, "nupc_update_coeff_async: bad argument");
    if (!n->finalized || !n->upd_reserve)
        return nfail(BFHIP_ESTATE, "nupc_update_coeff_async: needs bfhip_nupc_reserve_update before finalize, and finalize");
    if (coeff == n->live[filter].set || coeff == n->queued[filter].set || (n->sw && coeff == n->sw_old[filter].set))
        return nfail(BFHIP_ESTATE, "nupc_update_coeff_async: the set is live or part of a queued / in-flight switch");
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (n->upd_inflight) return nfail(BFHIP_ESTATE, "nupc_update_coeff_async: a rewrite is in flight (bfhip_nupc_update_busy)");
    // set 0 keeps the partitions add_filter gave it: taps past them must be zero (a device source
    // cannot be looked at without a wait: it must not reach past them at all)
    for (const Seg &s : n->seg) {
        const long covered = s.off + (long)s.n_blocks[filter][coeff] * s.L;
        const long from = std::min(covered, n_taps), to = std::min(s.off + (long)s.L * s.N, n_taps);
        bool past = on_device && from < to;
        if (!on_device)
            for (long i = from; i < to && !past; i++)
                past = n->rs == 4 ? ((const float *)taps)[i] != 0.0f : ((const double *)taps)[i] != 0.0;
        if (past) return nfail(BFHIP_EINVAL, "nupc_update_coeff_async: set 0 of this filter is shorter than these taps (add_filter's length)");
    }
    if (!on_device && taps != (const void *)n->h_upd) memcpy(n->h_upd, taps, (size_t)n_taps * n->rs);
    NCHK(hipSetDevice(n->device));
    if (eq) {
        // a failure here has touched eq.taps only: the set is as it was
        NCHK(eq_launch(n, *eq, n_taps, eq_mode));
        NCHK(hipEventRecord(n->ev_eq, n->upd_stream));
        ready_event = n->ev_eq;
    }
    // from here on work may be enqueued: a failure leaves the set's contents unknown
    n->upd_inflight = true;
    n->upd_filter = filter; n->upd_set = coeff;
    n->upd_bad[filter][coeff] = 1;
    n->upd_failed = false;
    const int r = upd_enqueue(n, filter, coeff, taps, on_device, n_taps, ready_event);
    if (r < 0) n->upd_failed = true;
    return r;
}

int upd_enqueue(bfhip_nupc *n, int filter, int coeff, const void *taps, bool on_device, long n_taps, void *ready_event) {
    const size_t rs = (size_t)n->rs;
    const uint8_t *src = on_device ? (const uint8_t *)taps : n->h_upd;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    bool main_waits = false;
    if (on_device && ready_event) NCHK(hipStreamWaitEvent(n->upd_stream, (hipEvent_t)ready_event, 0));
    // upload: a segment that runs on the main stream gets its own slice there (the high-priority
    // stream never waits for the whole upload); the rest goes through the loader, adjacent slices
    // in one copy
    long run_from = -1, run_to = -1;
    auto flush = [&]() -> hipError_t {
        if (run_from < 0 || run_to <= run_from) { run_from = run_to = -1; return hipSuccess; }
        const hipError_t e = hipMemcpyAsync(n->d_upd + (size_t)run_from * rs, src + (size_t)run_from * rs,
                                            (size_t)(run_to - run_from) * rs, kind, n->upd_stream);
        run_from = run_to = -1;
        return e;
    };
    for (const Seg &s : n->seg) {
        const long from = s.off, to = std::min(s.off + (long)s.L * s.N, n_taps);
        if (to <= from) continue;
        if (s.delay_steps > 0) {
            if (run_to != from) { NCHK(flush()); run_from = from; }
            run_to = to;
            continue;
        }
        if (on_device && ready_event && !main_waits) { NCHK(hipStreamWaitEvent(n->stream, (hipEvent_t)ready_event, 0)); main_waits = true; }
        NCHK(hipMemcpyAsync(n->d_upd + (size_t)from * rs, src + (size_t)from * rs, (size_t)(to - from) * rs, kind, n->stream));
    }
    NCHK(flush());
    NCHK(hipEventRecord(n->ev_upd_load, n->upd_stream));
    // preparation: one launch per segment engine on the engine's own stream, in order with its blocks
    for (size_t k = 0; k < n->seg.size(); k++) {
        Seg &s = n->seg[k];
        const long cap = (long)s.L * s.N;
        const long left = std::max(0L, std::min(n_taps - s.off, cap));
        if (s.delay_steps > 0) NCHK(hipStreamWaitEvent(s.stream, n->ev_upd_load, 0));
        ECHK(bfhip_internal_engine_update_coeff_dev_async(s.eng, n->coeff[filter][coeff], n->d_upd + (size_t)s.off * rs,
                                                          (int)left, s.n_blocks[filter][coeff], n->h_upd_bad + k));
        if (s.delay_steps > 0) NCHK(hipEventRecord(s.ev_upd, s.stream));
    }
    NCHK(hipEventRecord(n->ev_upd_main, n->stream));
    return BFHIP_OK;
}

}  // namespace

extern "C" {

// one I/O block of L_0 frames, device-resident raw buffers, asynchronous on the nupc's stream
int bfhip_nupc_block_dev(bfhip_nupc *n, const void *rawin_dev, void *rawout_dev) {
    if (!n || !n->finalized) return nfail(BFHIP_ESTATE, "nupc not finalized");
    if (!rawin_dev || !rawout_dev) return nfail(BFHIP_EINVAL, "nupc_block_dev: null buffer");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    const int L0 = n->seg[0].L;
    const unsigned long long end = (n->block + 1) * (unsigned long long)L0;       // samples received
    // append to the input ring (segment blocks are aligned: never split by the wrap)
    const size_t wpos = (size_t)((end - L0) % (unsigned long long)n->in_frames);
    // (a side with a declared buffer has no raw ring: the period is staged, and only its reals are kept)
    uint8_t *slot = n->buf_bytes[0] ? n->d_stage : n->d_in + wpos * n->frame_bytes[0];
    if ((const uint8_t *)rawin_dev != slot)                                   // block() uploads straight into the slot
        NCHK(hipMemcpyAsync(slot, rawin_dev, n->period_bytes[0], hipMemcpyDeviceToDevice, n->stream));
    // input delay and mute on the slot, before any segment (or ev_in, which the background
    // segment streams wait on) reads it
    { const int r = nupc_delay_side(n, BFHIP_IN, slot); if (r < 0) return r; }
    // sub-delay or a declared buffer on the input side: convert (and filter) the period once, in
    // front of all segments
    if (n->in_real) { const int r = nupc_subdelay_in(n, slot, wpos); if (r < 0) return r; }
    if (n->gain_dirty) {
        // output gains set since the last block: this block's first frame is the first of the step
        // or ramp, which starts from the gain of the last emitted frame.  Every record goes up as
        // the mirror has it: where the other channels' ramps are now.
        bool changed = false;
        for (int ch = 0; ch < n->n_out; ch++) {
            NupcGain &r = n->ramp[ch];
            if (n->gain[ch] == r.g) continue;
            const double prev = r.done >= r.len ? r.g : r.a + (r.g - r.a) * ((double)r.done / (double)r.len);
            r.a = n->gain_len[ch] ? prev : n->gain[ch];
            r.g = n->gain[ch]; r.done = 0; r.len = n->gain_len[ch];
            changed = true;
        }
        if (changed) {
            NCHK(hipEventSynchronize(n->ev_gain));                // the previous upload has read h_gain
            std::copy(n->ramp.begin(), n->ramp.end(), n->h_gain);
            NCHK(hipMemcpyAsync(n->d_gain, n->h_gain, (size_t)n->n_out * sizeof(NupcGain), hipMemcpyHostToDevice, n->stream));
            NCHK(hipEventRecord(n->ev_gain, n->stream));
        }
        n->gain_dirty = false;
    }
    if (!n->sw) nupc_commit(n, end - L0);
    const long long old_end = n->t_sw + n->sw_F;
    bool ev_in_recorded = false;
    for (auto &s : n->seg) {
        if (end % (unsigned long long)s.L != 0) continue;
        const size_t rpos = (size_t)((end - s.L) % (unsigned long long)n->in_frames);
        const unsigned long long pos = end - s.L + (unsigned long long)s.off;
        // which assignment(s) this block's frames [pos, pos + L) need, and into which ring
        int mode = 1;
        void *acc = n->ring(n->cur), *acc2 = nullptr;
        bool fade = false;
        const size_t k = (size_t)(&s - n->seg.data());
        if (n->sw && n->sw_stag) {
            // the segment's own switch frame decides; everything goes into the live ring
            fade = (long long)pos < n->t_seg[k] + n->sw_F && (long long)(pos + s.L) > n->t_seg[k];
            mode = fade ? 2 : 1;
        } else if (n->sw) {
            const bool need_old = (long long)pos < old_end, need_new = (long long)(pos + s.L) > n->t_sw;
            mode = need_old && need_new ? 2 : need_old ? 0 : 1;
            if (mode == 1) acc = n->ring(1 - n->cur);
            if (mode == 2) acc2 = n->ring(1 - n->cur);
            if (need_old) n->old_hi = std::max(n->old_hi, (long long)(pos + s.L));
        }
        const uint8_t *in = n->in_real ? n->d_in_real + rpos * (size_t)n->n_in * n->rs : n->d_in + rpos * n->frame_bytes[0];
        if (s.delay_steps == 0) {
            { const int r = seg_run(n, s, in, mode); if (r < 0) return r; }
            { const int r = fade ? nupc_accumulate_fade(n, s, pos, acc, n->t_seg[k], n->sw_F) : nupc_accumulate(n, s, pos, acc, acc2);
              if (r < 0) return r; }
            continue;
        }
        if (s.pending) return nfail(BFHIP_ESTATE, "nupc: a background segment block was never collected");
        if (!ev_in_recorded) { NCHK(hipEventRecord(n->ev_in, n->stream)); ev_in_recorded = true; }
        NCHK(hipStreamWaitEvent(s.stream, n->ev_in, 0));
        if (s.consumed_once) NCHK(hipStreamWaitEvent(s.stream, s.ev_consumed, 0));   // d_out is free again
        { const int r = seg_run(n, s, in, mode); if (r < 0) return r; }
        NCHK(hipEventRecord(s.ev_done, s.stream));
        s.pending = true;
        s.pending_pos = pos;
        s.pending_acc[0] = acc;
        s.pending_acc[1] = acc2;
        s.pending_fade = fade;
        s.pending_tk = n->t_seg.empty() ? 0 : n->t_seg[k];
        s.pending_F = n->sw_F;
        s.due_block = n->block + (unsigned long long)s.delay_steps;
    }
    for (auto &s : n->seg) {
        if (!s.pending || s.due_block != n->block) continue;
        NCHK(hipStreamWaitEvent(n->stream, s.ev_done, 0));
        { const int r = s.pending_fade ? nupc_accumulate_fade(n, s, s.pending_pos, s.pending_acc[0], s.pending_tk, s.pending_F)
                                       : nupc_accumulate(n, s, s.pending_pos, s.pending_acc[0], s.pending_acc[1]);
          if (r < 0) return r; }
        NCHK(hipEventRecord(s.ev_consumed, n->stream));
        s.pending = false;
        s.consumed_once = true;
    }
    const unsigned long long opos = end - L0;
    // inside a switch window the old assignment's ring is read beside the new one's
    // (a staggered switch has blended its fades into the live ring already: the single-ring path)
    const bool two_rings = n->sw && !n->sw_stag;
    void *acc_old = n->ring(n->cur), *acc_new = two_rings ? n->ring(1 - n->cur) : nullptr;
    const long long rel0 = two_rings ? (long long)opos - n->t_sw : 0;
    if (n->rs == 4) {
        if (n->sd_use[1]) nupc_emit_launch<float, true>(n, acc_old, acc_new, opos, rel0, rawout_dev);
        else nupc_emit_launch<float, false>(n, acc_old, acc_new, opos, rel0, rawout_dev);
    } else {
        if (n->sd_use[1]) nupc_emit_launch<double, true>(n, acc_old, acc_new, opos, rel0, rawout_dev);
        else nupc_emit_launch<double, false>(n, acc_old, acc_new, opos, rel0, rawout_dev);
    }
    NCHK(hipGetLastError());
    for (NupcGain &r : n->ramp) if (r.done < r.len) r.done = r.len - r.done < L0 ? r.len : r.done + L0;   // gain_advance's mirror
    // output delay and mute on the quantised block (block() copies it out behind this)
    { const int r = nupc_delay_side(n, BFHIP_OUT, (uint8_t *)rawout_dev); if (r < 0) return r; }
    n->block++;
    if (n->sw && n->sw_stag) {
        if (!nupc_stagger_left(n, end)) n->sw = false;            // the live ring stays the live ring
    } else if (n->sw && !nupc_switch_left(n, end)) {
        // the old ring has been emitted and cleared down to its last written frame: it is the spare now
        n->sw = false;
        n->cur = 1 - n->cur;
    }
    return BFHIP_OK;
}

// waits for the periods handed in so far (NOT for background segment blocks that are not due
// yet) and returns the status bits collected since the last call
int bfhip_nupc_sync(bfhip_nupc *n) {
    if (!n || !n->finalized) return nfail(BFHIP_ESTATE, "nupc not finalized");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    NCHK(hipStreamSynchronize(n->stream));
    const int st = *(volatile int *)n->h_status;
    *n->h_status = 0;
    return st;
}

// host buffers: copies in, runs, copies out, waits; returns status bits
int bfhip_nupc_block(bfhip_nupc *n, const void *rawin, void *rawout, bfhip_overflow overflow[]) {
    if (!n || !n->finalized || !rawin || !rawout) return nfail(BFHIP_ESTATE, "nupc_block: bad state or argument");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    const int L0 = n->seg[0].L;
    // upload straight into this block's slot of the input ring
    const unsigned long long end = (n->block + 1) * (unsigned long long)L0;
    const size_t wpos = (size_t)((end - L0) % (unsigned long long)n->in_frames);
    uint8_t *slot = n->buf_bytes[0] ? n->d_stage : n->d_in + wpos * n->frame_bytes[0];
    // through pinned staging buffers: copies from pageable memory stall in the runtime every so often
    memcpy(n->h_in, rawin, n->period_bytes[0]);
    NCHK(hipMemcpyAsync(slot, n->h_in, n->period_bytes[0], hipMemcpyHostToDevice, n->stream));
    if (overflow) {
        memcpy(n->h_over, overflow, n->n_out * sizeof(DevOverflow));
        NCHK(hipMemcpyAsync(n->d_over, n->h_over, n->n_out * sizeof(DevOverflow), hipMemcpyHostToDevice, n->stream));
    }
    int r = bfhip_nupc_block_dev(n, slot, n->d_rawout);
    if (r < 0) return r;
    NCHK(hipMemcpyAsync(n->h_out, n->d_rawout, n->period_bytes[1], hipMemcpyDeviceToHost, n->stream));
    if (overflow) NCHK(hipMemcpyAsync(n->h_over, n->d_over, n->n_out * sizeof(DevOverflow), hipMemcpyDeviceToHost, n->stream));
    r = bfhip_nupc_sync(n);
    if (r < 0) return r;
    memcpy(rawout, n->h_out, n->period_bytes[1]);
    if (overflow) memcpy(overflow, n->h_over, n->n_out * sizeof(DevOverflow));
    return r;
}

int bfhip_nupc_get_overflow(bfhip_nupc *n, int ch, bfhip_overflow *of) {
    if (!n || !n->finalized || !of || ch < 0 || ch >= n->n_out) return nfail(BFHIP_EINVAL, "nupc_get_overflow: bad argument");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    NCHK(hipStreamSynchronize(n->stream));
    NCHK(hipMemcpy(of, n->d_over + ch, sizeof(DevOverflow), hipMemcpyDeviceToHost));
    return BFHIP_OK;
}

// ---- run-time control: coefficient switches and output gain --------------------------------

int bfhip_nupc_set_crossfade(bfhip_nupc *n, int frames) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (frames < 0 || frames == 1 || frames > 1048576) return nfail(BFHIP_EINVAL, "nupc_set_crossfade: 0 (hard switch) or 2 .. 1048576 frames");
    n->crossfade = frames;
    return BFHIP_OK;
}

int bfhip_nupc_set_coeff(bfhip_nupc *n, int filter, int coeff) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (filter < 0 || filter >= (int)n->coeff.size() || coeff < 0 || coeff >= (int)n->coeff[filter].size())
        return nfail(BFHIP_EINVAL, "nupc_set_coeff: bad filter or set");
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_coeff before finalize");
    if (n->sw) return nfail(BFHIP_ESTATE, "nupc_set_coeff: the previous switch is still in flight (bfhip_nupc_switch_busy)");
    if (n->upd_reserve) {
        { const int r = upd_poll(n); if (r < 0) return r; }
        if (n->upd_inflight && filter == n->upd_filter && coeff == n->upd_set)
            return nfail(BFHIP_ESTATE, "nupc_set_coeff: a rewrite of this set is in flight (bfhip_nupc_update_busy)");
        if (n->upd_bad[filter][coeff])
            return nfail(BFHIP_ESTATE, "nupc_set_coeff: the last rewrite of this set found a NaN or Inf value among its coefficients");
    }
    n->queued[filter].set = coeff;
    return BFHIP_OK;
}

long bfhip_nupc_switch_frame(const bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_ESTATE, "null");                 // not BFHIP_EINVAL: -1 means "no switch yet"
    return n->t_sw;
}

int bfhip_nupc_switch_busy(const bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    return n->sw ? 1 : 0;
}

int bfhip_nupc_set_switch_mode(bfhip_nupc *n, int mode) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (mode != BFHIP_NUPC_SWITCH_ALIGNED && mode != BFHIP_NUPC_SWITCH_STAGGERED)
        return nfail(BFHIP_EINVAL, "nupc_set_switch_mode: BFHIP_NUPC_SWITCH_ALIGNED or BFHIP_NUPC_SWITCH_STAGGERED");
    if (n->sw) return nfail(BFHIP_ESTATE, "nupc_set_switch_mode: the previous switch is still in flight (bfhip_nupc_switch_busy)");
    for (const Asg &q : n->queued)
        if (q.set >= 0 || !std::isnan(q.gain))
            return nfail(BFHIP_ESTATE, "nupc_set_switch_mode: a set_coeff / set_filter_gain request is queued");
    n->switch_mode = mode;
    return BFHIP_OK;
}

int bfhip_nupc_get_switch_mode(const bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    return n->switch_mode;
}

long bfhip_nupc_switch_frame_segment(const bfhip_nupc *n, int segment) {
    if (!n) return nfail(BFHIP_ESTATE, "null");                 // not -1: that means "no switch yet"
    if (segment < 0 || segment >= (int)n->seg.size()) return nfail(BFHIP_ESTATE, "nupc_switch_frame_segment: bad segment");
    return n->t_seg.empty() ? -1 : (long)n->t_seg[segment];
}

// rewrite every partition of an idle set in every segment engine
int bfhip_nupc_update_coeff(bfhip_nupc *n, int filter, int coeff, const void *taps, long n_taps) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (filter < 0 || filter >= (int)n->coeff.size() || coeff < 0 || coeff >= (int)n->coeff[filter].size() ||
        !taps || n_taps < 1 || n_taps > bfhip_nupc_taps(n))
        return nfail(BFHIP_EINVAL, "nupc_update_coeff: bad argument");
    if (coeff == n->live[filter].set || coeff == n->queued[filter].set || (n->sw && coeff == n->sw_old[filter].set))
        return nfail(BFHIP_ESTATE, "nupc_update_coeff: the set is live or part of a queued / in-flight switch");
    OWNER(n);
    if (n->upd_reserve && n->finalized) {
        { const int r = upd_poll(n); if (r < 0) return r; }
        if (n->upd_inflight) return nfail(BFHIP_ESTATE, "nupc_update_coeff: an asynchronous rewrite is in flight (bfhip_nupc_update_busy)");
    }
    // set 0 keeps the partitions add_filter gave it: taps past them must be zero
    const unsigned char *t = (const unsigned char *)taps;
    auto nonzero = [&](long from, long to) {
        for (long i = from; i < to; i++)
            if (n->rs == 4 ? ((const float *)t)[i] != 0.0f : ((const double *)t)[i] != 0.0) return true;
        return false;
    };
    for (const Seg &s : n->seg) {
        const long covered = s.off + (long)s.n_blocks[filter][coeff] * s.L;
        if (nonzero(std::min(covered, n_taps), std::min(s.off + (long)s.L * s.N, n_taps)))
            return nfail(BFHIP_EINVAL, "nupc_update_coeff: set 0 of this filter is shorter than these taps (add_filter's length)");
    }
    NCHK(hipSetDevice(n->device));
    for (Seg &s : n->seg) {
        std::vector<unsigned char> part((size_t)s.L * n->rs);
        for (int p = 0; p < s.n_blocks[filter][coeff]; p++) {
            const long first = s.off + (long)p * s.L;
            const long take = std::max(0L, std::min((long)s.L, n_taps - first));
            std::fill(part.begin(), part.end(), 0);
            if (take > 0) memcpy(part.data(), t + (size_t)first * n->rs, (size_t)take * n->rs);
            ECHK(bfhip_engine_update_coeff_block(s.eng, n->coeff[filter][coeff], p, part.data()));
        }
    }
    if (n->upd_reserve && n->finalized) n->upd_bad[filter][coeff] = 0;
    return BFHIP_OK;
}

// ---- run-time control: asynchronous set rewrite ---------------------------------------------

int bfhip_nupc_reserve_update(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_update after finalize");
    n->upd_reserve = true;
    return BFHIP_OK;
}

void *bfhip_nupc_update_buffer(bfhip_nupc *n) { return n && n->finalized ? n->h_upd : nullptr; }

int bfhip_nupc_update_coeff_async(bfhip_nupc *n, int filter, int coeff, const void *taps, long n_taps) {
    return upd_start(n, filter, coeff, taps, false, n_taps, nullptr);
}

int bfhip_nupc_update_coeff_dev_async(bfhip_nupc *n, int filter, int coeff, const void *taps_dev, long n_taps,
                                      void *ready_event) {
    return upd_start(n, filter, coeff, taps_dev, true, n_taps, ready_event);
}

int bfhip_nupc_update_busy(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->upd_reserve) return 0;
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    return n->upd_inflight ? 1 : 0;
}

int bfhip_nupc_update_result(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->upd_reserve) return nfail(BFHIP_ESTATE, "nupc_update_result: no reservation (bfhip_nupc_reserve_update)");
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (n->upd_inflight) return nfail(BFHIP_ESTATE, "nupc_update_result: the rewrite is still in flight (bfhip_nupc_update_busy)");
    if (n->upd_result == BFHIP_EHIP) return nfail(BFHIP_EHIP, "nupc_update_result: the rewrite could not be enqueued completely");
    if (n->upd_result != BFHIP_OK) return nfail(n->upd_result, "NaN or Inf value among coefficients.");
    return BFHIP_OK;
}

// ---- run-time control: equaliser curves rendered on the device ------------------------------

int bfhip_nupc_reserve_eq(bfhip_nupc *n, long max_taps) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_eq after finalize");
    if (!n->upd_reserve) return nfail(BFHIP_ESTATE, "nupc_reserve_eq: needs bfhip_nupc_reserve_update first");
    if (max_taps < 8 || (max_taps & (max_taps - 1)) || max_taps > std::min(bfhip_nupc_taps(n), 1L << (kEqMaxLog2H + 1)))
        return nfail(BFHIP_EINVAL, "nupc_reserve_eq: max_taps must be a power of two, 8 .. min(taps, 1048576)");
    n->eq_reserve = max_taps;
    return BFHIP_OK;
}

int bfhip_nupc_reserve_eq_minimum(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_minimum after finalize");
    if (!n->eq_reserve) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_minimum: needs bfhip_nupc_reserve_eq first");
    n->eq_min.reserved = true;
    return BFHIP_OK;
}

// state and curve checks shared by the render calls; fills the kernel-argument copy of the bands
static int eq_check(const bfhip_nupc *n, long taps, int n_bands, const double freq[], const double mag[],
                    const double phase[], int mode, EqBands *b) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->eq_reserve)
        return nfail(BFHIP_ESTATE, "nupc_render_eq: needs bfhip_nupc_reserve_eq before finalize, and finalize");
    if (mode != BFHIP_EQ_LINEAR && mode != BFHIP_EQ_MINIMUM)
        return nfail(BFHIP_EINVAL, "nupc_render_eq: mode must be BFHIP_EQ_LINEAR or BFHIP_EQ_MINIMUM");
    if (mode == BFHIP_EQ_MINIMUM && !n->eq_min.reserved)
        return nfail(BFHIP_ESTATE, "nupc_render_eq: minimum phase needs bfhip_nupc_reserve_eq_minimum before finalize");
    if (taps < 8 || (taps & (taps - 1)) || taps > n->eq_reserve)
        return nfail(BFHIP_EINVAL, "nupc_render_eq: taps must be a power of two, 8 .. max_taps");
    if (!freq || !mag || !phase || n_bands < 2 || n_bands > kEqMaxBands)
        return nfail(BFHIP_EINVAL, "nupc_render_eq: 2 .. 130 bands");
    if (freq[0] != 0.0 || freq[n_bands - 1] != 0.5)
        return nfail(BFHIP_EINVAL, "nupc_render_eq: the first band must be at 0 and the last at 0.5");
    for (int i = 0; i < n_bands; i++) {
        if (i > 0 && !(freq[i] > freq[i - 1])) return nfail(BFHIP_EINVAL, "nupc_render_eq: band frequencies must ascend");
        if (!std::isfinite(mag[i]) || mag[i] < 0.0 || !std::isfinite(phase[i]))
            return nfail(BFHIP_EINVAL, "nupc_render_eq: magnitudes must be finite and >= 0, phases finite");
        if (mode == BFHIP_EQ_MINIMUM && !(mag[i] > 0.0))
            return nfail(BFHIP_EINVAL, "nupc_render_eq: minimum phase needs every magnitude > 0");
        b->freq[i] = freq[i]; b->mag[i] = mag[i]; b->phase[i] = phase[i];
    }
    b->n = n_bands;
    return BFHIP_OK;
}

int bfhip_nupc_render_eq_mode_async(bfhip_nupc *n, int filter, int coeff, long taps, int n_bands, const double freq[],
                                    const double mag[], const double phase[], int mode) {
    EqBands b;
    { const int r = eq_check(n, taps, n_bands, freq, mag, phase, mode, &b); if (r < 0) return r; }
    return upd_start(n, filter, coeff, n->eq.taps, true, taps, nullptr, &b, mode);
}

int bfhip_nupc_render_eq_async(bfhip_nupc *n, int filter, int coeff, long taps, int n_bands, const double freq[],
                               const double mag[], const double phase[]) {
    return bfhip_nupc_render_eq_mode_async(n, filter, coeff, taps, n_bands, freq, mag, phase, BFHIP_EQ_LINEAR);
}

int bfhip_nupc_render_eq_mode(bfhip_nupc *n, long taps, int n_bands, const double freq[], const double mag[],
                              const double phase[], int mode, void *taps_out) {
    EqBands b;
    { const int r = eq_check(n, taps, n_bands, freq, mag, phase, mode, &b); if (r < 0) return r; }
    if (!taps_out) return nfail(BFHIP_EINVAL, "nupc_render_eq: null buffer");
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (n->upd_inflight) return nfail(BFHIP_ESTATE, "nupc_render_eq: a rewrite is in flight (bfhip_nupc_update_busy)");
    NCHK(hipSetDevice(n->device));
    NCHK(eq_launch(n, b, taps, mode));
    NCHK(hipMemcpyAsync(taps_out, n->eq.taps, (size_t)taps * n->rs, hipMemcpyDeviceToHost, n->upd_stream));
    NCHK(hipStreamSynchronize(n->upd_stream));
    return BFHIP_OK;
}

int bfhip_nupc_render_eq(bfhip_nupc *n, long taps, int n_bands, const double freq[], const double mag[],
                         const double phase[], void *taps_out) {
    return bfhip_nupc_render_eq_mode(n, taps, n_bands, freq, mag, phase, BFHIP_EQ_LINEAR, taps_out);
}

// blocks: not for the audio thread
int bfhip_nupc_update_wait(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->upd_reserve) return nfail(BFHIP_ESTATE, "nupc_update_wait: no reservation (bfhip_nupc_reserve_update)");
    OWNER(n);
    if (n->upd_inflight) {
        NCHK(hipSetDevice(n->device));
        NCHK(hipEventSynchronize(n->ev_upd_load));
        NCHK(hipEventSynchronize(n->ev_upd_main));
        for (auto &s : n->seg) if (s.ev_upd) NCHK(hipEventSynchronize(s.ev_upd));
    }
    return bfhip_nupc_update_result(n);
}

int bfhip_nupc_set_output_gain(bfhip_nupc *n, int out_ch, double gain) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (out_ch < 0 || out_ch >= n->n_out || !std::isfinite(gain)) return nfail(BFHIP_EINVAL, "nupc_set_output_gain: bad argument");
    if (n->gain[out_ch] != gain) { n->gain[out_ch] = gain; n->gain_len[out_ch] = n->gain_ramp; n->gain_dirty = true; }
    return BFHIP_OK;
}

int bfhip_nupc_set_gain_ramp(bfhip_nupc *n, int frames) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (frames < 0 || frames > 1048576) return nfail(BFHIP_EINVAL, "nupc_set_gain_ramp: 0 (step) or 1 .. 1048576 frames");
    n->gain_ramp = frames;
    return BFHIP_OK;
}

// ---- run-time control: per-filter gain as part of a switch ----------------------------------

int bfhip_nupc_reserve_filter_gain(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_filter_gain after finalize");
    n->gain_reserve = true;
    return BFHIP_OK;
}

int bfhip_nupc_set_filter_gain(bfhip_nupc *n, int filter, double gain) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (filter < 0 || filter >= (int)n->coeff.size() || !std::isfinite(gain))
        return nfail(BFHIP_EINVAL, "nupc_set_filter_gain: bad filter, or a gain that is not finite");
    if (!n->finalized) { n->live[filter].gain = gain; return BFHIP_OK; }     // the initial gain
    if (!n->gain_reserve) return nfail(BFHIP_ESTATE, "nupc_set_filter_gain: needs bfhip_nupc_reserve_filter_gain before finalize");
    if (n->sw) return nfail(BFHIP_ESTATE, "nupc_set_filter_gain: the previous switch is still in flight (bfhip_nupc_switch_busy)");
    n->queued[filter].gain = gain;
    return BFHIP_OK;
}

double bfhip_nupc_get_filter_gain(const bfhip_nupc *n, int filter) {
    if (!n || filter < 0 || filter >= (int)n->coeff.size()) { nfail(BFHIP_EINVAL, "nupc_get_filter_gain: bad argument"); return NAN; }
    return n->live[filter].gain;
}

// bf_reset_peak(): the initial structs go up behind the periods handed in so far and in front of
// the next one, through block()'s pinned staging (idle between block() calls; a second reset
// writes the same bytes into it); no host wait
int bfhip_nupc_reset_overflow(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc not finalized");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    for (int ch = 0; ch < n->n_out; ch++) n->h_over[ch] = over_initial(n->fmt[1][ch]);
    NCHK(hipMemcpyAsync(n->d_over, n->h_over, (size_t)n->n_out * sizeof(DevOverflow), hipMemcpyHostToDevice, n->stream));
    return BFHIP_OK;
}

// ---- run-time control: per-channel delay and mute -------------------------------------------

static int delay_channel_ok(const bfhip_nupc *n, int io, int ch) {
    return n && io >= 0 && io <= 1 && ch >= 0 && ch < (io ? n->n_out : n->n_in);
}

int bfhip_nupc_set_maxdelay(bfhip_nupc *n, int io, int ch, int maxdelay) {
    if (!delay_channel_ok(n, io, ch)) return nfail(BFHIP_EINVAL, "nupc_set_maxdelay: bad argument");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_maxdelay after finalize");
    n->dl[io][ch].maxdelay = maxdelay;
    return BFHIP_OK;
}

int bfhip_nupc_set_delay(bfhip_nupc *n, int io, int ch, int delay) {
    if (!delay_channel_ok(n, io, ch) || delay < 0) return nfail(BFHIP_EINVAL, "nupc_set_delay: bad argument");
    n->dl[io][ch].req = delay + n->dl[io][ch].extra;   // change_delay at the next block call ignores what it must
    return BFHIP_OK;
}

int bfhip_nupc_set_mute(bfhip_nupc *n, int io, int ch, int muted) {
    if (!delay_channel_ok(n, io, ch)) return nfail(BFHIP_EINVAL, "nupc_set_mute: bad argument");
    n->dl[io][ch].muted = muted != 0;
    return BFHIP_OK;
}

int bfhip_nupc_get_delay(const bfhip_nupc *n, int io, int ch) {
    if (!delay_channel_ok(n, io, ch)) return nfail(BFHIP_EINVAL, "nupc_get_delay: bad argument");
    if (n->finalized) return n->dl[io][ch].curdelay - n->dl[io][ch].extra;
    NupcDelay d = n->dl[io][ch];                // what finalize will start with
    (void)d.init(n->seg[0].L, 1);
    return d.curdelay;
}

// ---- run-time control: per-channel sub-sample delay -----------------------------------------

int bfhip_nupc_enable_subdelay(bfhip_nupc *n, int sdf_length, double kaiser_beta) {
    (void)kaiser_beta;       // parsed by the reference (sdf_beta) but its filters are built with 9 (delay.c:73)
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_enable_subdelay after finalize");
    const int L0 = n->seg[0].L;
    if (sdf_length < 1) return nfail(BFHIP_EINVAL, "Invalid half filter length " + std::to_string(sdf_length) + ".");
    if (2 * sdf_length + 1 > L0) return nfail(BFHIP_EINVAL, "The filter_length must be at least 2 x sdf_length + 1.");
    int bs = 1;
    while (bs < 2 * sdf_length + 1) bs <<= 1;
    if (L0 % bs != 0)
        return nfail(BFHIP_EINVAL, "Incompatible fragment/filter sizes (" + std::to_string(L0) + "/" + std::to_string(2 * sdf_length + 1) + ").");
    if (bs > kSdMaxBs)
        return nfail(BFHIP_EINVAL, "nupc_enable_subdelay: sdf_length above " + std::to_string(kSdMaxBs / 2 - 1) + " is not supported");
    n->sdf_length = sdf_length; n->sd_flen = 2 * sdf_length + 1; n->sd_bs = bs;
    return BFHIP_OK;
}

int bfhip_nupc_set_subdelay(bfhip_nupc *n, int io, int ch, int subdelay) {
    if (!delay_channel_ok(n, io, ch)) return nfail(BFHIP_EINVAL, "nupc_set_subdelay: bad argument");
    const bool in_range = subdelay > -100 && subdelay < 100;
    if (!n->finalized) {
        if (!in_range && subdelay != BFHIP_UNDEFINED_SUBDELAY) return nfail(BFHIP_EINVAL, "nupc_set_subdelay: value out of range (-100, 100)");
        n->sd[io][ch] = subdelay;
        return BFHIP_OK;
    }
    // set_subdelay, bfrun.c:520-541
    if (n->sd[io][ch] == BFHIP_UNDEFINED_SUBDELAY) return nfail(BFHIP_EINVAL, "nupc_set_subdelay: the channel has no sub-sample delay filter");
    if (!in_range) return nfail(BFHIP_EINVAL, "nupc_set_subdelay: value out of range (-100, 100)");
    n->sd[io][ch] = subdelay;                   // read by the next block call
    return BFHIP_OK;
}

int bfhip_nupc_get_subdelay(const bfhip_nupc *n, int io, int ch) {
    if (!delay_channel_ok(n, io, ch)) return nfail(BFHIP_EINVAL, "nupc_get_subdelay: bad argument");
    return n->sd[io][ch];
}

// the taps the device filters with (no HIP call: the bank is made of these)
int bfhip_selftest_subdelay_filter(int sdf_length, int subdelay, int realsize, void *out) {
    if (sdf_length < 1 || subdelay <= -100 || subdelay >= 100 || (realsize != 4 && realsize != 8) || !out)
        return nfail(BFHIP_EINVAL, "selftest_subdelay_filter: bad argument");
    if (realsize == 4) {
        std::vector<float> f;
        sd_make_filter(f, sdf_length, (double)subdelay / 100, 9.0);
        memcpy(out, f.data(), f.size() * 4);
    } else {
        std::vector<double> f;
        sd_make_filter(f, sdf_length, (double)subdelay / 100, 9.0);
        memcpy(out, f.data(), f.size() * 8);
    }
    return 2 * sdf_length + 1;
}

}  // extern "C"
