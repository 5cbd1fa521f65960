// passes.hip -- every kernel launch of the engine (passes.h): the passes of a block on the transform path of
// its length, the MAC variants with the look-ahead bookkeeping, the coefficient kernels, real-time mode's copies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "passes.h"
#include "bigfft.h"

BFHIP_HOST_NS {

// ---------------------------------------------------------------- the transform path of a block length

// what transforms a block: the LDS FFT (fft_lds.h), the wave FFT (fft_wave.h: K1, K3 and their fusion, L = 1024 ..
// 8192 where the engine chose it) or, above 8192 points, the global-memory FFT (bigfft.h)
enum class Fft { Lds, Wave, Big };
static Fft fft_path(const bfhip_engine *e) { return e->big ? Fft::Big : e->wave ? Fft::Wave : Fft::Lds; }

// The two one-workgroup transforms as seen by a launch: threads, twiddle table, K1 and K3.
template <typename T, int LOG2L> struct Lds {
    using real = T;
    static constexpr int LOG2 = LOG2L, MIN_LOG2 = 2, NT = fft_threads<T>(LOG2L);
    static constexpr bool WAVE = false;
    static const c2<T> *tw(const bfhip_engine *e) { return (const c2<T> *)e->d_tw; }
    static auto fft_in() { return fft_in_kernel<T, LOG2L>; }
    static auto ifft_out() { return ifft_out_kernel<T, LOG2L>; }
};
template <typename T, int LOG2L> struct Wave {
    using real = T;
    static constexpr int LOG2 = LOG2L, MIN_LOG2 = 10, NT = WaveGeo<LOG2L>::NT;
    static constexpr bool WAVE = true;
    static const c2<T> *tw(const bfhip_engine *e) { return (const c2<T> *)e->d_tww; }
    static auto fft_in() { return fft_in_wave_kernel<T, LOG2L>; }
    static auto ifft_out() { return ifft_out_wave_kernel<T, LOG2L>; }
};

// f(P<T, LOG2L>()) for the block length 2^LOG2L, P's shortest .. 8192; no call for any other length
template <template <typename, int> class P, typename T, int LG = P<T, 13>::MIN_LOG2, typename F>
void with_length(int log2L, F &f) {
    if constexpr (LG <= 13) {
        if (log2L == LG) f(P<T, LG>());
        else with_length<P, T, LG + 1>(log2L, f);
    }
}
// f(T()) for the engine's precision
template <typename F> void with_real(const bfhip_engine *e, F &&f) {
    if (e->rs == 4) f(float()); else f(double());
}
// One pass on the engine's path: fft(P()) with P the traits of its one-workgroup transform, or big(T()).
// WAVE_TOO = false: a pass without wave kernels (level and coefficient transforms are LDS ones wherever they fit).
template <bool WAVE_TOO = true, typename F, typename B> void on_path(const bfhip_engine *e, F &&fft, B &&big) {
    const Fft path = fft_path(e);
    if (path == Fft::Big) return with_real(e, big);
    if constexpr (WAVE_TOO)
        if (path == Fft::Wave) return with_real(e, [&](auto t) { with_length<Wave, decltype(t)>(e->log2L, fft); });
    with_real(e, [&](auto t) { with_length<Lds, decltype(t)>(e->log2L, fft); });
}

static inline PowerSave ps_arg(const bfhip_engine *e) {
    PowerSave ps;
    ps.thr = e->d_ps_flags ? e->powersave : 0.0;
    ps.scale = e->d_ps_scale; ps.flags = e->d_ps_flags; ps.live = e->d_ps_live;
    return ps;
}

// ---------------------------------------------------------------- K1, K3 and their fusion in one workgroup per channel

template <typename P>
void launch_fft_in(bfhip_engine *e, const uint8_t *raw, int slot, hipError_t *err) {
    using T = typename P::real;
    const size_t lds = lds_fft_bytes(P::LOG2, sizeof(c2<T>));
    auto k = P::fft_in();
    *err = allow_lds(k, lds);
    if (*err != hipSuccess) return;
    hipLaunchKernelGGL(k, dim3(e->n_ch[0]), dim3(P::NT), lds, e->ls, raw, e->d_fmt[0],
                       (T *)e->d_prev, (c2<T> *)e->d_ring, P::tw(e), e->R, slot,
                       (const BlockState *)e->bs_arg, ps_arg(e));
    *err = hipGetLastError();
}

template <typename P>
void launch_ifft_out(bfhip_engine *e, const void *Zp, size_t chunk_stride, int n_chunks,
                     int first, int count, uint8_t *raw, hipError_t *err) {
    using T = typename P::real;
    const size_t lds = lds_fft_bytes(P::LOG2, sizeof(c2<T>));
    auto k = P::ifft_out();
    *err = allow_lds(k, lds);
    if (*err != hipSuccess) return;
    hipLaunchKernelGGL(k, dim3(count), dim3(P::NT), lds, e->ls, (const c2<T> *)Zp, chunk_stride,
                       n_chunks, first, e->d_fmt[1], e->d_over, e->ch.skip_quant(),
                       raw, e->ch.timeout<T>(first, e->L),
                       P::tw(e), e->safety_limit, e->d_status);
    *err = hipGetLastError();          // (the dither pass behind it: do_outputs)
}

// K3 of an earlier block (count channels from Zp) + K1 of the current block in one launch.  The two kernels'
// parameter lists differ: io_kernel reads ONE spectrum per channel (fused_outputs_inputs refuses more chunks)
// and takes no BlockState (no schedule that is captured into a graph fuses the two passes).
template <typename P>
void launch_io(bfhip_engine *e, const void *Zp, size_t chunk_stride, int n_chunks, int first, int count,
               uint8_t *rawout, const uint8_t *rawin, int slot, hipError_t *err) {
    using T = typename P::real;
    const size_t lds = lds_fft_bytes(P::LOG2, sizeof(c2<T>));
    const dim3 grid(count + e->n_ch[0]);
    if constexpr (P::WAVE) {
        auto k = io_wave_kernel<T, P::LOG2>;
        *err = allow_lds(k, lds);
        if (*err != hipSuccess) return;
        hipLaunchKernelGGL(k, grid, dim3(P::NT), lds, e->ls, count,
                           (const c2<T> *)Zp, chunk_stride, n_chunks, first, e->d_fmt[1], e->d_over,
                           e->ch.skip_quant(), rawout,
                           e->ch.timeout<T>(first, e->L),
                           e->safety_limit, e->d_status,
                           rawin, e->d_fmt[0], (T *)e->d_prev, (c2<T> *)e->d_ring, e->R, slot,
                           P::tw(e), ps_arg(e), (const BlockState *)e->bs_arg);
    } else {
        auto k = io_kernel<T, P::LOG2>;
        *err = allow_lds(k, lds);
        if (*err != hipSuccess) return;
        hipLaunchKernelGGL(k, grid, dim3(P::NT), lds, e->ls, count,
                           (const c2<T> *)Zp, first, e->d_fmt[1], e->d_over, e->ch.skip_quant(),
                           rawout, e->ch.timeout<T>(first, e->L),
                           e->safety_limit, e->d_status,
                           rawin, e->d_fmt[0], (T *)e->d_prev, (c2<T> *)e->d_ring, e->R, slot, P::tw(e), ps_arg(e));
    }
    *err = hipGetLastError();
}

template <typename P>
void launch_coeff_prep(bfhip_engine *e, const void *taps, int n_taps, double scale, void *H,
                       int n_blocks, hipError_t *err) {
    using T = typename P::real;
    const size_t lds = lds_fft_bytes(P::LOG2, sizeof(c2<T>));
    auto k = coeff_prep_kernel<T, P::LOG2>;
    *err = allow_lds(k, lds);
    if (*err != hipSuccess) return;
    hipLaunchKernelGGL(k, dim3(n_blocks), dim3(P::NT), lds, e->stream, (const T *)taps, n_taps,
                       (T)scale, (c2<T> *)H, P::tw(e), e->d_bad);
    *err = hipGetLastError();
}

// ---------------------------------------------------------------- the MAC

// the grid mac_decode (kernels.h) takes apart: n_tc (tile, chunk) pairs rounded up to the 8 XCDs, times the groups
static int mac_grid(int n_tc, int n_groups) { return ((n_tc + 7) / 8) * n_groups * 8; }

int block_age(const bfhip_engine *e, int ahead) {
    return (int)std::min<unsigned long long>(e->blocks_done + 1 + (unsigned long long)ahead, (unsigned long long)e->N);
}

// the spectrum of a diag job goes to `tsplit` workgroups (consecutive runs of `tiles` tiles): ~512 workgroups
// in all, no partial sums -- runs of 16 - 64 KiB either way (BFHIP_DIAG_TSPLIT: 1, 2, 4 ...; read at every launch)
struct DiagGeo { int tsplit, tiles; };
template <typename T> DiagGeo diag_geometry(const bfhip_engine *e, int n_jobs) {
    const int all_tiles = std::max(1, e->L / (256 * (int)(16 / sizeof(c2<T>))));
    int tsplit = 1;
    while (tsplit < all_tiles && tsplit < 8 && n_jobs * tsplit < 512) tsplit *= 2;
    if (const char *env = getenv("BFHIP_DIAG_TSPLIT")) {
        tsplit = 1;
        while (tsplit * 2 <= std::min(all_tiles, atoi(env))) tsplit *= 2;
    }
    while (all_tiles / tsplit > 16) tsplit *= 2;            // float64 at L = 8192: 32 tiles, 16 per workgroup
    return {tsplit, all_tiles / tsplit};
}

template <typename T>
void launch_mac(bfhip_engine *e, void *Zp, hipError_t *err) {
    const int n_tc = e->n_tiles * e->n_chunks;
    const int grid = mac_grid(n_tc, e->n_groups);
    const int age = block_age(e);
#define BFHIP_LAUNCH_MAC(NTFLAG, U)                                                                   \
    hipLaunchKernelGGL((mac_xbar_kernel<T, NTFLAG, U>), dim3(grid), dim3(e->mac_threads), 0, e->ls,      \
                       (const MacEntry<T> *)e->b_entries.p, (const ChunkRange *)e->b_chunks.p,               \
                       (c2<T> *)Zp, e->L, e->n_out_padded, e->n_groups, e->n_chunks, n_tc,               \
                       e->blockcounter, age, (const BlockState *)e->bs_arg,                              \
                       (NTFLAG && U == 0) ? e->hstream : StreamLayout{nullptr, 0, 0, 0})
    if (e->mac_diag) {
        const int n_jobs = e->n_chunks * e->n_out_padded;
        const DiagGeo g = diag_geometry<T>(e, n_jobs);
#define BFHIP_LAUNCH_DIAG(NTFLAG, TL)                                                                                  \
        hipLaunchKernelGGL((mac_diag_kernel<T, NTFLAG, TL>), dim3(n_jobs * g.tsplit), dim3(256), 0, e->ls,             \
                           (const MacEntry<T> *)e->b_entries.p, e->d_diag_jobs, (c2<T> *)Zp, e->L, e->n_out_padded,      \
                           e->blockcounter, age, (const BlockState *)e->bs_arg, g.tsplit)
#define BFHIP_DIAG_TILES(NTFLAG)                                              \
        switch (g.tiles) {                                                    \
        case 1: BFHIP_LAUNCH_DIAG(NTFLAG, 1); break;                          \
        case 2: BFHIP_LAUNCH_DIAG(NTFLAG, 2); break;                          \
        case 4: BFHIP_LAUNCH_DIAG(NTFLAG, 4); break;                          \
        case 8: BFHIP_LAUNCH_DIAG(NTFLAG, 8); break;                          \
        default: BFHIP_LAUNCH_DIAG(NTFLAG, 16); break;                        \
        }
        if (e->mac_nt) { BFHIP_DIAG_TILES(true) } else { BFHIP_DIAG_TILES(false) }
#undef BFHIP_DIAG_TILES
#undef BFHIP_LAUNCH_DIAG
    }
    else if (!e->mac_nt) BFHIP_LAUNCH_MAC(false, 2);
    // the pipelined variant needs ~290 VGPRs: worth it for the pure crossbar, a loss of occupancy
    // for plans that (also) run the latency-bound per-term paths
    else if (e->mac_unroll == 0 && e->all_dense) BFHIP_LAUNCH_MAC(true, 0);
    else if (e->mac_unroll == 0) BFHIP_LAUNCH_MAC(true, 2);
    else if (e->mac_unroll == 4) BFHIP_LAUNCH_MAC(true, 4);
    else if (e->mac_unroll == 3) BFHIP_LAUNCH_MAC(true, 3);
    else if (e->mac_unroll == 1) BFHIP_LAUNCH_MAC(true, 1);
    else BFHIP_LAUNCH_MAC(true, 2);
#undef BFHIP_LAUNCH_MAC
    *err = hipGetLastError();
}

// the long-window MAC (kernels.h): the crossbar kernel over the long entries, ring step 3
static void launch_mac_long(bfhip_engine *e, void *Zp, hipError_t *err) {
    const int n_tc = e->lw_tiles * e->lw_chunks;
    hipLaunchKernelGGL((mac_xbar_kernel<float, true, 0, 3>), dim3(mac_grid(n_tc, e->n_groups)), dim3(256), 0, e->ls,
                       (const MacEntry<float> *)e->b_lentries.p, (const ChunkRange *)e->b_lchunks.p, (c2<float> *)Zp,
                       2 * e->L, e->n_out_padded, e->n_groups, e->lw_chunks, n_tc, e->blockcounter, block_age(e),
                       (const BlockState *)e->bs_arg, e->lstream);
    *err = hipGetLastError();
}

// the look-ahead passes (kernels.h): ahead buffer of (block mod 4, slice)
static c2<float> *la_buffer(bfhip_engine *e, unsigned long long block, int slice) {
    const size_t one = (size_t)e->n_out_padded * 2 * e->L;
    return (c2<float> *)e->b_ahead.p + ((size_t)(block & 3ull) * 3 + (size_t)slice) * one;
}
static c2<float> *far_buffer(bfhip_engine *e, unsigned long long block, int slice) {
    const size_t one = (size_t)e->n_out_padded * 2 * e->L;
    return (c2<float> *)e->b_far.p + ((size_t)(block % 7ull) * LA_FAR + (size_t)slice) * one;
}
// head: the head pass of this block (its three ahead buffers are current) and the tail pass of this call's slice
// in one launch; else the tail pass alone, behind a full long MAC
static void launch_mac_la(bfhip_engine *e, void *Zp, bool head, hipError_t *err) {
    const int n_tc = e->lw_tiles;
    const unsigned long long T = e->blocks_done;
    const int slice = (int)(T % 3ull);
    const bool two = e->far_active && e->b_far.p != nullptr;
    LaFar<float> far = {};
    if (two) {
        far.slice = (int)(T % (unsigned long long)LA_FAR);
        for (int k = 0; k < LA_FAR; k++) {
            far.A[k] = far_buffer(e, T, k);
            far.Z[k] = far_buffer(e, T + 1 + k, far.slice);
            far.age[k] = block_age(e, k + 1);
        }
    }
#define BFHIP_LAUNCH_LA(PHASES)                                                                                        \
    hipLaunchKernelGGL((mac_la_kernel<float, PHASES>), dim3(mac_grid(n_tc, e->n_groups)), dim3(256), 0, e->ls,         \
                       (const MacEntry<float> *)e->b_lentries.p, (const ChunkRange *)e->b_lchunks.p, (c2<float> *)Zp,      \
                       (const c2<float> *)la_buffer(e, T, 0), (const c2<float> *)la_buffer(e, T, 1),                   \
                       (const c2<float> *)la_buffer(e, T, 2),                                                          \
                       la_buffer(e, T + 1, slice), la_buffer(e, T + 2, slice), la_buffer(e, T + 3, slice),             \
                       2 * e->L, e->n_groups, n_tc, e->blockcounter, block_age(e), block_age(e, 1), block_age(e, 2),   \
                       block_age(e, 3), slice, e->lstream, far)
    if (two) { if (head) BFHIP_LAUNCH_LA(7); else BFHIP_LAUNCH_LA(6); }
    else if (head) BFHIP_LAUNCH_LA(3); else BFHIP_LAUNCH_LA(2);
#undef BFHIP_LAUNCH_LA
    *err = hipGetLastError();
    if (*err != hipSuccess) return;
    e->n_mac_launches++;
    for (int k = 1; k <= 3; k++) {
        e->la_for[(T + k) & 3ull][slice] = T + k;
        e->la_at[(T + k) & 3ull][slice] = e->la_epoch;
    }
    if (two)
        for (int k = 1; k <= LA_FAR; k++) {
            e->far_for[(T + k) % 7ull][far.slice] = T + k;
            e->far_at[(T + k) % 7ull][far.slice] = e->la_epoch;
        }
}

// No block has been processed (or prewarm has just declared the zero-initialised rings N blocks of
// silence): every window the tails of the next three blocks read is silence, so their ahead buffers
// are zeros.  Store that instead of running three full MACs first.
int la_prime(bfhip_engine *e) {
    if (!e->la_active || e->b_ahead.p == nullptr) return BFHIP_OK;
    HIPCHK(hipMemsetAsync(e->b_ahead.p, 0, e->b_ahead.cap, e->stream));
    for (unsigned long long T = e->blocks_done; T < e->blocks_done + 3; T++)
        for (int j = 0; j < 3; j++) { e->la_for[T & 3ull][j] = T; e->la_at[T & 3ull][j] = e->la_epoch; }
    if (!e->far_active || e->b_far.p == nullptr) return BFHIP_OK;
    // the far tails of the next six blocks read silence alone as well
    HIPCHK(hipMemsetAsync(e->b_far.p, 0, e->b_far.cap, e->stream));
    for (unsigned long long T = e->blocks_done; T < e->blocks_done + LA_FAR; T++)
        for (int j = 0; j < LA_FAR; j++) { e->far_for[T % 7ull][j] = T; e->far_at[T % 7ull][j] = e->la_epoch; }
    return BFHIP_OK;
}

// are the three ahead buffers of the block about to run current?
static bool la_block_valid(const bfhip_engine *e) {
    const unsigned long long T = e->blocks_done;
    for (int j = 0; j < 3; j++)
        if (e->la_for[T & 3ull][j] != T || e->la_at[T & 3ull][j] != e->la_epoch) return false;
    if (e->far_active && e->b_far.p != nullptr)
        for (int j = 0; j < LA_FAR; j++)
            if (e->far_for[T % 7ull][j] != T || e->far_at[T % 7ull][j] != e->la_epoch) return false;
    return true;
}

// [long K3 of `count` outputs from the long partial sums Zp | long K1 of this block's inputs (inputs)]
static void launch_io_long(bfhip_engine *e, const void *Zp, int count, uint8_t *rawout, bool inputs, hipError_t *err) {
    constexpr int NT = fft_threads<float>(LW_LOG2);
    const int n_in = inputs ? e->n_ch[0] : 0;
    if (count + n_in == 0) return;
    const size_t lds = lds_fft_bytes(LW_LOG2, sizeof(c2<float>));
    auto k = io_long_kernel<float, LW_LOG2>;
    *err = allow_lds(k, lds);
    if (*err != hipSuccess) return;
    hipLaunchKernelGGL(k, dim3(count + n_in), dim3(NT), lds, e->ls, count, (const c2<float> *)Zp,
                       (size_t)e->n_out_padded * 2 * e->L, e->lw_chunks, 0, e->d_fmt[1], e->d_over,
                       e->ch.skip_quant(), rawout, e->safety_limit, e->d_status,
                       (const float *)e->d_prev, (float *)e->d_hist, (c2<float> *)e->d_lring, e->R, e->blockcounter,
                       (const c2<float> *)e->d_tw14, (const BlockState *)e->bs_arg);
    *err = hipGetLastError();
}

// which of the engine's partial-sum buffers Zp is (-1: a caller's buffer) and whether it holds long spectra
static int zp_index(const bfhip_engine *e, const void *Zp) {
    for (int i = 0; i < 3; i++) if (Zp != nullptr && Zp == e->d_Zp[i]) return i;
    return -1;
}
static bool zp_is_long(const bfhip_engine *e, const void *Zp) {
    const int i = zp_index(e, Zp);
    return i >= 0 && e->zp_long[i];
}

// ---------------------------------------------------------------- level kernels

// The per-filter kernels of every level in order: ring fills (N-way mixes, cascades), filter MACs,
// cross-fades.  fill(jobs, sources, n) and fade(jobs, n) launch the path's transforms for one level.
template <typename T, typename Fill, typename Fade>
void launch_levels(bfhip_engine *e, Fill fill, Fade fade, hipError_t *err) {
    const int age = block_age(e);
    const unsigned char *base = (const unsigned char *)e->b_jobs.p;
    const int V = 16 / (int)sizeof(c2<T>);
    const int threads = e->mac_threads;
    const int tiles = (e->L + threads * V - 1) / (threads * V);
    for (auto &lj : e->level_jobs) {
        if (lj.n_fill > 0) {
            fill((const FillJob<T> *)(base + lj.fill_off), (const MixSrc<T> *)(base + e->src_off), lj.n_fill);
            if (*err != hipSuccess) return;
        }
        if (lj.n_filt > 0) {
            hipLaunchKernelGGL(mac_filter_kernel<T>, dim3(tiles, lj.n_filt), dim3(threads), 0, e->ls,
                               (const FilterJob<T> *)(base + lj.filt_off), e->L, e->blockcounter, age,
                               (const BlockState *)e->bs_arg);
        }
        if (lj.n_fade > 0) {
            fade((const FadeJob<T> *)(base + lj.fade_off), lj.n_fade);
            if (*err != hipSuccess) return;
        }
        if ((*err = hipGetLastError()) != hipSuccess) return;
    }
}

template <typename P>
void launch_levels_lds(bfhip_engine *e, hipError_t *err) {
    using T = typename P::real;
    const size_t lds = lds_fft_bytes(P::LOG2, sizeof(c2<T>));
    auto kf = ring_fill_kernel<T, P::LOG2>;
    auto kx = crossfade_kernel<T, P::LOG2>;
    launch_levels<T>(e,
        [&](const FillJob<T> *jobs, const MixSrc<T> *src, int n) {
            if ((*err = allow_lds(kf, lds)) != hipSuccess) return;
            hipLaunchKernelGGL(kf, dim3(n), dim3(P::NT), lds, e->ls, jobs, src, P::tw(e),
                               e->N, e->blockcounter, (const BlockState *)e->bs_arg);
        },
        [&](const FadeJob<T> *jobs, int n) {
            if ((*err = allow_lds(kx, lds)) != hipSuccess) return;
            hipLaunchKernelGGL(kx, dim3(n), dim3(P::NT), lds, e->ls, jobs, P::tw(e));
        }, err);
}

// ---------------------------------------------------------------- block lengths above 8192 (bigfft.h)

// scratch for n_tr transforms of L complex points each (zin, zmid, zout)
int big_reserve(bfhip_engine *e, size_t n_tr) {
    if (n_tr <= e->big_cap) return BFHIP_OK;
    { int r = sync_all(e); if (r != BFHIP_OK) return r; }
    for (DevBuf &b : e->b_big) HIPCHK(b.grow(n_tr * (size_t)e->L * e->csize()));
    e->big_cap = n_tr;
    return BFHIP_OK;
}

// zin -> zout: complex FFT of L points for n_tr transforms on `st`
template <typename T>
void big_fft(bfhip_engine *e, int n_tr, bool inv, hipStream_t st, hipError_t *err) {
    const c2<T> *zin = (const c2<T> *)e->b_big[0].p;
    c2<T> *zmid = (c2<T> *)e->b_big[1].p, *zout = (c2<T> *)e->b_big[2].p;
    const c2<T> *tw13 = (const c2<T> *)e->d_tw13, *twL = (const c2<T> *)e->d_tw;
    *err = inv ? big_fft_run<T, true>(zin, zmid, zout, e->log2L, n_tr, tw13, twL, st)
               : big_fft_run<T, false>(zin, zmid, zout, e->log2L, n_tr, tw13, twL, st);
}

static inline dim3 big_grid_half(const bfhip_engine *e, int n_tr) { return dim3((unsigned)(e->L / 2 / 256 + 1), (unsigned)n_tr); }

template <typename T>
void launch_fft_in_big(bfhip_engine *e, const uint8_t *raw, int slot, hipError_t *err) {
    const int n = e->n_ch[0];
    const int parity = (int)(e->blocks_done & 1);
    const bool ps_on = e->d_ps_flags != nullptr;
    hipLaunchKernelGGL(big_in_pre<T>, big_grid_half(e, n), dim3(256), 0, e->ls, raw, e->d_fmt[0], (T *)e->d_prev,
                       (c2<T> *)e->b_big[0].p, e->L, ps_on ? e->d_ps_acc : (unsigned long long *)nullptr, n, parity,
                       e->powersave >= 1.0 ? 1 : 0);
    big_fft<T>(e, n, false, e->ls, err);
    if (*err != hipSuccess) return;
    hipLaunchKernelGGL(big_untangle<T>, big_grid_half(e, n), dim3(256), 0, e->ls, (const c2<T> *)e->b_big[2].p,
                       (c2<T> *)e->d_ring + (size_t)slot * e->L, (size_t)e->R * e->L, (const c2<T> *)e->d_tw, e->L, (T)1);
    if (ps_on)
        hipLaunchKernelGGL(big_ps_finish<T>, dim3((unsigned)(e->L / 256), (unsigned)n), dim3(256), 0, e->ls,
                           (const unsigned long long *)e->d_ps_acc, n, parity, ps_arg(e), (c2<T> *)e->d_ring, e->R, slot, e->L);
    *err = hipGetLastError();
}

template <typename T>
void launch_coeff_prep_big(bfhip_engine *e, const void *taps, int n_taps, double scale, void *H,
                           int n_blocks, hipError_t *err) {
    hipStream_t keep = e->ls;
    e->ls = e->stream;
    hipLaunchKernelGGL(big_coeff_pre<T>, big_grid_half(e, n_blocks), dim3(256), 0, e->stream, (const T *)taps, n_taps,
                       (T)scale, (c2<T> *)e->b_big[0].p, e->L, e->d_bad);
    big_fft<T>(e, n_blocks, false, e->stream, err);
    if (*err == hipSuccess) {
        hipLaunchKernelGGL(big_untangle<T>, big_grid_half(e, n_blocks), dim3(256), 0, e->stream, (const c2<T> *)e->b_big[2].p,
                           (c2<T> *)H, (size_t)e->L, (const c2<T> *)e->d_tw, e->L, (T)1.0 / (T)(2 * e->L));
        *err = hipGetLastError();
    }
    e->ls = keep;
}

template <typename T>
void launch_ifft_out_big(bfhip_engine *e, const void *Zp, size_t chunk_stride, int n_chunks,
                         int first, int count, uint8_t *raw, hipError_t *err) {
    hipLaunchKernelGGL(big_out_pre<T>, big_grid_half(e, count), dim3(256), 0, e->ls, (const c2<T> *)Zp, chunk_stride,
                       n_chunks, (c2<T> *)e->b_big[0].p, (const c2<T> *)e->d_tw, e->L);
    big_fft<T>(e, count, true, e->ls, err);
    if (*err != hipSuccess) return;
    hipLaunchKernelGGL(big_out_post<T>, dim3(count), dim3(1024), 0, e->ls, (const c2<T> *)e->b_big[2].p, first, e->d_fmt[1],
                       e->d_over, e->ch.skip_quant(), raw,
                       e->ch.timeout<T>(first, e->L), e->L, e->safety_limit,
                       e->d_status);
    *err = hipGetLastError();          // (the dither pass behind it: do_outputs)
}

template <typename T>
void launch_levels_big(bfhip_engine *e, hipError_t *err) {
    const c2<T> *twL = (const c2<T> *)e->d_tw;
    launch_levels<T>(e,
        [&](const FillJob<T> *jobs, const MixSrc<T> *src, int n) {
            hipLaunchKernelGGL(big_fill_pre<T>, big_grid_half(e, n), dim3(256), 0, e->ls, jobs, src,
                               (c2<T> *)e->b_big[0].p, twL, e->L);
            big_fft<T>(e, n, true, e->ls, err);
            if (*err != hipSuccess) return;
            hipLaunchKernelGGL(big_fill_slide<T>, big_grid_half(e, n), dim3(256), 0, e->ls, jobs,
                               (const c2<T> *)e->b_big[2].p, (c2<T> *)e->b_big[0].p, e->L);
            big_fft<T>(e, n, false, e->ls, err);
            if (*err != hipSuccess) return;
            hipLaunchKernelGGL(big_fill_post<T>, big_grid_half(e, n), dim3(256), 0, e->ls, jobs, src,
                               (const c2<T> *)e->b_big[2].p, twL, e->N, e->blockcounter, e->L, (const BlockState *)e->bs_arg);
        },
        [&](const FadeJob<T> *jobs, int n) {
            hipLaunchKernelGGL(big_fade_pre<T>, big_grid_half(e, 2 * n), dim3(256), 0, e->ls, jobs,
                               (c2<T> *)e->b_big[0].p, twL, e->L);
            big_fft<T>(e, 2 * n, true, e->ls, err);
            if (*err != hipSuccess) return;
            hipLaunchKernelGGL(big_fade_mix<T>, dim3((unsigned)(e->L / 256), (unsigned)n), dim3(256), 0, e->ls,
                               (const c2<T> *)e->b_big[2].p, (c2<T> *)e->b_big[0].p, e->L);
            big_fft<T>(e, n, false, e->ls, err);
            if (*err != hipSuccess) return;
            hipLaunchKernelGGL(big_fade_post<T>, big_grid_half(e, n), dim3(256), 0, e->ls, jobs,
                               (const c2<T> *)e->b_big[2].p, twL, e->L);
        }, err);
}

// ---------------------------------------------------------------- timing

static int record(bfhip_engine *e, int stage, bool end) {
    if (!e->timed_now) return BFHIP_OK;
    if (e->bs_arg != nullptr) return BFHIP_OK;           // a graph is being captured: replayed blocks are not timed
    HIPCHK(hipEventRecord(e->ev[(size_t)e->ev_used * EV_PER_BLOCK + 2 * stage + end], e->ls));
    if (end) e->timed_mask |= 1 << stage;
    return BFHIP_OK;
}
int record_begin(bfhip_engine *e, int stage) { return record(e, stage, false); }
int record_end(bfhip_engine *e, int stage) { return record(e, stage, true); }

// ---------------------------------------------------------------- the passes of a block

int do_inputs(bfhip_engine *e, const void *rawin_dev, unsigned int ahead) {
    { int rv = channels_before_k1(e, rawin_dev); if (rv != BFHIP_OK) return rv; }
    hipError_t err = hipSuccess;
    const uint8_t *raw = (const uint8_t *)rawin_dev;
    const int slot = (int)((e->blockcounter + ahead) % (unsigned int)e->R);
    if (e->big) { int rr = big_reserve(e, (size_t)e->n_ch[0]); if (rr != BFHIP_OK) return rr; }
    on_path(e, [&](auto p) { launch_fft_in<decltype(p)>(e, raw, slot, &err); },
               [&](auto t) { launch_fft_in_big<decltype(t)>(e, raw, slot, &err); });
    if (err != hipSuccess) return fail(BFHIP_EHIP, "fft_in launch: %s", hipGetErrorString(err));
    if (e->lw_struct) launch_io_long(e, nullptr, 0, nullptr, true, &err);       // behind it: it reads prev
    if (err != hipSuccess) return fail(BFHIP_EHIP, "long fft_in launch: %s", hipGetErrorString(err));
    return BFHIP_OK;
}

int do_levels(bfhip_engine *e) {
    bool any = false;
    for (auto &lj : e->level_jobs) any = any || lj.n_fill || lj.n_filt || lj.n_fade;
    if (!any) return BFHIP_OK;
    hipError_t err = hipSuccess;
    { const int rr = record_begin(e, T_LEVELS); if (rr != BFHIP_OK) return rr; }
    if (e->big) {
        size_t need = 1;
        for (auto &lj : e->level_jobs) need = std::max(need, std::max((size_t)lj.n_fill, (size_t)2 * lj.n_fade));
        int rr = big_reserve(e, need);
        if (rr != BFHIP_OK) return rr;
    }
    on_path<false>(e, [&](auto p) { launch_levels_lds<decltype(p)>(e, &err); },
                      [&](auto t) { launch_levels_big<decltype(t)>(e, &err); });
    if (err != hipSuccess) return fail(BFHIP_EHIP, "level kernels: %s", hipGetErrorString(err));
    return record_end(e, T_LEVELS);
}

int do_mac(bfhip_engine *e, void *Zp, bool may_long) {
    hipError_t err = hipSuccess;
    e->zp_is_sum = false;
    // the long plan covers blocks whose partial sums stay in the engine's own buffers and are converted
    // by its own output pass (not the phase calls, which hand standard spectra to the caller)
    const int zi = zp_index(e, Zp);
    const bool lng = e->lw_active && zi >= 0 && may_long;
    if (zi >= 0) e->zp_long[zi] = lng;
    // look-ahead (not under a captured graph or in real-time mode, whose launch arguments are frozen):
    // the head pass when the block's three ahead buffers are current, else the full long MAC; either way
    // the tail pass of this call's slice for the next three blocks behind it (in the head pass's launch)
    const bool la = lng && e->la_active && e->bs_arg == nullptr && !e->rt.on;
    if (la && la_block_valid(e)) {
        launch_mac_la(e, Zp, true, &err);
        if (err != hipSuccess) return fail(BFHIP_EHIP, "look-ahead mac launch: %s", hipGetErrorString(err));
        e->n_la_head++;
        return BFHIP_OK;
    }
    if (lng) { launch_mac_long(e, Zp, &err); if (la) e->n_la_full++; }
    else with_real(e, [&](auto t) { launch_mac<decltype(t)>(e, Zp, &err); });
    if (err != hipSuccess) return fail(BFHIP_EHIP, "mac launch: %s", hipGetErrorString(err));
    e->n_mac_launches++;
    if (la) {
        launch_mac_la(e, nullptr, false, &err);
        if (err != hipSuccess) return fail(BFHIP_EHIP, "look-ahead mac launch: %s", hipGetErrorString(err));
    } else {
        e->la_epoch++;             // a block without a tail pass: what is stored ahead no longer lines up
    }
    return BFHIP_OK;
}

int do_mac_pair(bfhip_engine *e, void *Zp0, void *Zp1) {
    const int n_tc = e->n_tiles * e->n_chunks;
    e->zp_is_sum = false;
    with_real(e, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((mac_xbar2_kernel<T, true>), dim3(mac_grid(n_tc, e->n_groups)), dim3(e->mac_threads), 0, e->ls,
                           (const MacEntry<T> *)e->b_entries.p, (const ChunkRange *)e->b_chunks.p, (c2<T> *)Zp0, (c2<T> *)Zp1,
                           e->L, e->n_out_padded, e->n_groups, e->n_chunks, n_tc, e->blockcounter, e->hstream);
    });
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(BFHIP_EHIP, "mac2 launch: %s", hipGetErrorString(err));
    return BFHIP_OK;
}

int sum_chunks(bfhip_engine *e, const void *Zp, void *Z) {
    const size_t n_per_chunk = (size_t)e->n_out_padded * e->L;
    const size_t n_valid = (size_t)e->n_ch[1] * e->L;
    const int grid = (int)((n_valid + 255) / 256);
    with_real(e, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(sum_partials_kernel<T>, dim3(grid), dim3(256), 0, e->ls,
                           (const c2<T> *)Zp, (c2<T> *)Z, n_per_chunk, n_valid, e->n_chunks);
    });
    if (Z == Zp) e->zp_is_sum = true;
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(BFHIP_EHIP, "sum_partials launch: %s", hipGetErrorString(err));
    return BFHIP_OK;
}

int do_outputs(bfhip_engine *e, const void *Zp, size_t chunk_stride, int n_chunks, int first,
               int count, void *rawout_dev) {
    hipError_t err = hipSuccess;
    if (count <= 0) return BFHIP_OK;
    if (e->ch.outputs_at_once() && (first != 0 || count != e->n_ch[1]))
        return fail(BFHIP_EINVAL, "outputs that share a physical channel cannot be split over several calls");
    const bool lng = zp_is_long(e, Zp);
    if (lng && (first != 0 || count != e->n_ch[1]))
        return fail(BFHIP_EINVAL, "a long-window block's outputs are converted all at once");
    if (!lng && n_chunks > 2 && n_chunks == e->n_chunks && first == 0 && count == e->n_ch[1] &&
        chunk_stride == (size_t)e->n_out_padded * e->L) {
        // many partials (few long filters): the one-workgroup-per-channel output pass would walk
        // them one dependent load after the other; add them up with the whole chip first
        // (in place, same order) and hand over a single spectrum per channel
        { const int rr = sum_chunks(e, Zp, const_cast<void *>(Zp)); if (rr != BFHIP_OK) return rr; }
        n_chunks = 1;
    }
    uint8_t *const raw = k3_target(e, rawout_dev);
    if (e->big) { int rr = big_reserve(e, (size_t)count); if (rr != BFHIP_OK) return rr; }
    if (lng) launch_io_long(e, Zp, count, raw, false, &err);
    else on_path(e, [&](auto p) { launch_ifft_out<decltype(p)>(e, Zp, chunk_stride, n_chunks, first, count, raw, &err); },
                    [&](auto t) { launch_ifft_out_big<decltype(t)>(e, Zp, chunk_stride, n_chunks, first, count, raw, &err); });
    if (err != hipSuccess) return fail(BFHIP_EHIP, "ifft_out launch: %s", hipGetErrorString(err));
    // what the channel stage launches behind the inverse transforms is timed apart: the reference's real2raw column
    const bool post = e->ch.follows_k3();
    if (post) { const int rr = record_begin(e, T_POST); if (rr != BFHIP_OK) return rr; }
    { int rv = channels_after_k3(e, rawout_dev, first, count); if (rv != BFHIP_OK) return rv; }
    return post ? record_end(e, T_POST) : BFHIP_OK;
}

int fused_outputs_inputs(bfhip_engine *e, const void *Zp, size_t chunk_stride, int n_chunks, int first, int count,
                         void *rawout_dev, const void *rawin_dev) {
    // the deferred and ping-pong schedules, whose owed blocks may hold two chunks, run on the wave FFT alone
    if (fft_path(e) == Fft::Lds && n_chunks != 1)
        return fail(BFHIP_EINVAL, "the fused output and input pass of the LDS transform takes one spectrum per output");
    int r;
    if ((r = channels_before_k1(e, rawin_dev)) != BFHIP_OK) return r;
    hipError_t err = hipSuccess;
    const int slot = (int)(e->blockcounter % (unsigned int)e->R);
    // an owed long-window block: its output pass rides with the long transforms of this block instead
    const bool lng = zp_is_long(e, Zp);
    if (lng && (first != 0 || count != e->n_ch[1]))
        return fail(BFHIP_EINVAL, "a long-window block's outputs are converted all at once");
    const int n_std = lng ? 0 : count;
    on_path(e, [&](auto p) {
                   launch_io<decltype(p)>(e, Zp, chunk_stride, n_chunks, first, n_std, k3_target(e, rawout_dev),
                                          (const uint8_t *)rawin_dev, slot, &err);
               },
               [](auto) {});           // (above 8192 points the callers keep the two passes apart)
    if (err != hipSuccess) return fail(BFHIP_EHIP, "io launch: %s", hipGetErrorString(err));
    if (e->lw_struct) launch_io_long(e, Zp, lng ? count : 0, k3_target(e, rawout_dev), true, &err);
    if (err != hipSuccess) return fail(BFHIP_EHIP, "long io launch: %s", hipGetErrorString(err));
    return channels_after_k3(e, rawout_dev, first, count);
}

// ---------------------------------------------------------------- coefficients

int coeff_prep(bfhip_engine *e, const void *taps_dev, int n_taps, double scale, void *H, int n_blocks) {
    if (e->big) { const int rr = big_reserve(e, (size_t)n_blocks); if (rr != BFHIP_OK) return rr; }
    hipError_t err = hipSuccess;
    on_path<false>(e, [&](auto p) { launch_coeff_prep<decltype(p)>(e, taps_dev, n_taps, scale, H, n_blocks, &err); },
                      [&](auto t) { launch_coeff_prep_big<decltype(t)>(e, taps_dev, n_taps, scale, H, n_blocks, &err); });
    if (err != hipSuccess) return fail(BFHIP_EHIP, "coeff_prep launch: %s", hipGetErrorString(err));
    return BFHIP_OK;
}

int coeff_reorder(bfhip_engine *e, void *taps, void *H, int n_blocks, bool to_packed) {
    const dim3 grid((e->L + 255) / 256, n_blocks);
    with_real(e, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(reorder_kernel<T>, grid, dim3(256), 0, e->stream, to_packed ? (const T *)taps : (const T *)nullptr,
                           (c2<T> *)H, e->L, to_packed ? 1 : 0, to_packed ? (T *)nullptr : (T *)taps);
    });
    HIPCHK(hipGetLastError());
    return BFHIP_OK;
}

int promote_ring(bfhip_engine *e, const void *src, void *ring, int delay, double scale, int n_valid) {
    const dim3 grid((e->L + 255) / 256, n_valid);
    with_real(e, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(promote_ring_kernel<T>, grid, dim3(256), 0, e->stream, (const c2<T> *)src, e->R,
                           (c2<T> *)ring, e->N, e->L, e->blockcounter, delay, (T)scale, n_valid);
    });
    HIPCHK(hipGetLastError());
    return BFHIP_OK;
}

// ---------------------------------------------------------------- real-time mode

int rt_copy_in(bfhip_engine *e, const RtCopy &in) {
    hipLaunchKernelGGL(rt_copy_in_kernel<0>, dim3((in.n16 + 255) / 256), dim3(256), 0, e->stream, in);
    HIPCHK(hipGetLastError());
    return BFHIP_OK;
}

int rt_tail(bfhip_engine *e, unsigned int grid, const RtCopy &out, int p) {
    hipLaunchKernelGGL(rt_tail_kernel<0>, dim3(grid), dim3(256), 0, e->stream, out, e->d_bs, e->N,
                       (const DevOverflow *)e->d_over, e->rt.h_over[p], e->n_ch[1], e->d_status, e->rt.h_status[p],
                       e->d_rt_arrive);
    HIPCHK(hipGetLastError());
    return BFHIP_OK;
}

}  // namespace bfhip_host
