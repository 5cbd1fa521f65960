// engine.h -- the engine's state, and the helpers that the host units of the engine use: bfhip.hip (the
// C ABI of include/bfhip.h, the block schedules), plan.hip (the plan builder), channels.hip (the channel
// stage, whose own state and interface are in channels.h) and passes.hip (every kernel launch; passes.h).
// Internal: nothing here is part of include/.
#pragma once
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/bfhip.h"
#include "alloc.h"
#include "kernels.h"

using namespace bfhip;

// Every device / pinned allocation of the engines goes through these (alloc.h), so that the tests
// can make the n-th one fail (bfhip_selftest_fail_alloc) and walk every out-of-memory path there is.
static inline hipError_t dev_alloc(void **p, size_t bytes) { return bfhip_internal_dev_alloc(p, bytes); }
template <typename P> static hipError_t dev_alloc(P **p, size_t bytes) { return bfhip_internal_dev_alloc((void **)p, bytes); }
static inline hipError_t pin_alloc(void **p, size_t bytes, unsigned int flags) { return bfhip_internal_pin_alloc(p, bytes, flags); }

// What the units share by name lives in this namespace: hidden, so that the dynamic symbols of
// the library stay those of the C ABI.
#define BFHIP_HOST_NS namespace bfhip_host __attribute__((visibility("hidden")))

BFHIP_HOST_NS {

// sets the calling thread's error text (bfhip_last_error) and returns `code` (bfhip.hip)
int fail(int code, const char *fmt, ...);

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(BFHIP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                              \
    } while (0)

// A device buffer that only grows: what a plan, a layout or a scratch area needs now, kept for the next
// one that fits.  No destructor: an engine deleted in a fork()ed child must not touch the device
// (bfhip_engine_destroy), so whoever owns the buffer calls release().
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;

    // at least `bytes`; the old contents are not kept.  On failure the buffer is empty.
    hipError_t grow(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t r = dev_alloc(&p, bytes);
        if (r == hipSuccess) cap = bytes; else p = nullptr;
        return r;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};

struct Coeff {
    int n_blocks = 0;
    void *d_H = nullptr;     // [n_blocks][L] packed spectra
    // a set the host keeps in (shared) memory in the reference's cbuf layout and that another
    // process may rewrite at run time (bflogic_eq through bfaccess->convolver_coeffs2cbuf):
    // where each block lives on the host, and the change-notice generation last uploaded
    std::vector<const void *> watch_src;
    std::vector<uint64_t> watch_gen;
    // BFHIP_COEFF_LAZY: the host blocks are remembered (watch_src) and go to the device the first
    // time an ACTIVE filter refers to the set -- a filter process of a multi-process host holds the
    // sets of its own filters, not the whole configuration's (d_H == nullptr until then)
    bool lazy = false, watched = false;
};

struct Filter {
    std::vector<int> in_ch, in_f, out_ch;
    std::vector<double> in_scale, in_fscale, out_scale;
    int coeff = -1, delayblocks = 0, crossfade = 0;
    int prevcoeff = -1;
    // false: another engine (another filter process of the host, bfrun.c:2312-2328) runs this filter.
    // It still takes part in the PLAN -- groups, entry order, chunk boundaries are those of the whole
    // configuration, so every output is summed in exactly the order a single engine would use --
    // but none of its work is launched here and its coefficients are not loaded.
    bool active = true;
    int name = -1;                     // the host's own number for the filter (intname); -1: its index here
};

constexpr int MAX_TIMED = 4096;
// event pairs of a timed block: T_IN K1 (input transforms), T_MAC K2 (MAC), T_OUT K3 (output pass,
// everything of it), T_POST the part of the output pass behind the inverse transforms (dither, N:1
// mix, sub-sample delay), T_LEVELS the per-filter level kernels in front of the MAC (N-way input
// mixes, cascades, cross-fades)
enum { T_IN, T_MAC, T_OUT, T_POST, T_LEVELS, EV_PAIRS };
constexpr int EV_PER_BLOCK = 2 * EV_PAIRS;

}  // namespace bfhip_host

#include "channels.h"

using namespace bfhip_host;

struct bfhip_engine {
    int device = 0;
    pid_t owner = 0;               // the process that created the engine (HIP state does not survive fork())
    int L = 0, N = 0, rs = 4, log2L = 0;
    int n_ch[2] = {0, 0};
    std::vector<bfhip_format> fmt[2];
    double safety_limit = 0.0;
    // `powersave:` (bfconf.c:1549-1561): 0 off, >= 1 exact-zero windows, < 1 linear noise floor
    double powersave = 0.0;
    int *d_ps_flags = nullptr, *d_ps_live = nullptr;
    unsigned long long *d_ps_acc = nullptr;    // partition lengths above 8192: [2][n_in] running maxima
    double *d_ps_scale = nullptr;
    std::vector<Coeff> coeffs;
    // Coefficient sets are carved out of a few large slabs instead of one hipMalloc each: the MAC
    // streams all of them at once (config C: 4096 sets, 8 GiB), and thousands of separate 2 MiB
    // allocations cost it 5-10 % (one hipMalloc per set: 0.79 - 0.86 of peak box to box, one slab
    // 0.886).  Where inside the slab a set starts matters as much -- the stream-ordered
    // copy below takes that out of the host's hands.
    struct Slab { void *base = nullptr; size_t cap = 0, used = 0; };
    std::vector<Slab> slabs;
    bool coeff_arena = true;               // BFHIP_COEFF_ARENA=0: one hipMalloc per set
    unsigned int skew_state = 12345u;
    // Stream-ordered copy of the coefficients for uniform crossbar plans (StreamLayout, kernels.h):
    // every MAC workgroup reads one sequential slice.  Built / refreshed by build_plan.
    int stream_wanted = 1;                 // BFHIP_COEFF_STREAM: 0 off, 1 from 64 MiB of coefficients up, 2 always
    StreamLayout hstream = {nullptr, 0, 0, 0};
    DevBuf b_stream;
    DevBuf b_where;                        // StreamWhere per entry | d_which: the entries to lay out
    int *d_which = nullptr;
    std::vector<std::array<const void *, OG>> stream_keys;     // per flat entry: the sets laid out there
    int stream_geom[5] = {0, 0, 0, 0, 0};                          // entries, E_c, P, n_tc, n_groups
    bool any_watched = false;
    unsigned long long watch_seq = 0;       // bfhip_coeff_dirty_sequence() at the last poll
    unsigned long long watch_lost = 0;      // bfhip_dirty_lost() at the last poll
    std::vector<Filter> filters;
    // shard of a configuration (multi-process host): which outputs this engine converts and writes.
    // -1 = derive at finalize (fed by an active filter, or by no filter at all), 0 / 1 = set by the host
    std::vector<signed char> out_active_set;
    std::vector<char> out_active;          // after finalize
    bool sharded = false;                  // some output belongs to another engine
    struct OwnedRun { size_t offset, len, stride; };       // bytes: per frame `len` at `offset`, frames `stride` apart
    std::vector<OwnedRun> owned_runs;      // the raw output samples this engine owns (merged channel runs)
    std::vector<unsigned char> h_stage;    // host staging for bfhip_engine_block of a sharded engine
    bool finalized = false, finalize_failed = false, plan_dirty = true;
    unsigned int blockcounter = 0;
    // ... which wraps by a multiple of every ring depth (N, and N + 1 when a spare slot exists)
    // long before 2^32, so that `blockcounter mod depth` never jumps (BlockState, kernels.h)
    unsigned int wrap_at = 0, wrap_by = 0;
    unsigned long long blocks_done = 0;      // since creation (procblocks analogue)

    hipStream_t stream = nullptr;      // main stream: per-filter kernels and the crossbar MAC
    bool own_stream = false;
    hipStream_t ls = nullptr;          // stream the next launch goes to
    // How bfhip_engine_block[_dev] schedules a block (BFHIP_MODE_*, choose_mode at finalize):
    //  - PIPELINED: the input FFT of block t+1 and the inverse FFT / requantiser of block t-1 run on
    //    their own streams beside the HBM-bound MAC of block t, the way the reference overlaps its
    //    input, filter and output processes (bfrun.c:2312-2616).  Needs one spare ring slot (R = N + 1).
    //  - DEFERRED (large crossbars on one stream): the inverse transforms of block t run in ONE launch
    //    with the forward transforms of block t+1 (io_wave_kernel) -- both are a handful of workgroups
    //    that would otherwise run back to back, each alone on the chip, in front of and behind the
    //    millisecond MAC.  The output of a block is therefore written during the NEXT
    //    bfhip_engine_block_dev call, or by bfhip_engine_sync (which flushes it).
    //  - PINGPONG (small crossbars with the wave FFT): [K3 of t-2 | K1 of t] in one launch on the side
    //    stream s_in while the MAC of t-1 runs on the main stream; the MAC of t waits for that launch.
    //    Two launches and four event calls per block instead of three launches and seven, and the two
    //    transforms run side by side.  Outputs are owed for two calls.
    int mode = BFHIP_MODE_SEQUENTIAL;
    int overlap_mode = -1;             // -1 auto, 0 off, 1 on (bfhip_engine_set_overlap)
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_mac[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    hipEvent_t ev_io[2] = {nullptr, nullptr}, ev_mac3[3] = {nullptr, nullptr, nullptr};
    int R = 0;                         // depth of the input rings
    struct Pending {
        void *Zp = nullptr; size_t chunk_stride = 0; int n_chunks = 0;
        void *rawout = nullptr; hipEvent_t out_done = nullptr;
        hipEvent_t mac_done = nullptr;     // ping-pong: the side stream waits for it before the inverse transforms
    };
    std::deque<Pending> pendq;         // outputs owed, oldest first (at most output_lag of them)

    // partition lengths above the LDS limit (bigfft.h): global scratch for [transform][L] complex
    bool big = false;
    int big_R = 1;                 // L / 8192
    DevBuf b_big[3];               // zin, zmid, zout
    size_t big_cap = 0;            // transforms the scratch holds
    void *d_tw13 = nullptr;        // twiddle table of the 8192-point LDS transform
    // K1 / K3 on the wave FFT (fft_wave.h: L = 1024 .. 8192, default from 4096 up; BFHIP_FFT_WAVE=0/1)
    bool wave = false;
    void *d_tww = nullptr;         // its twiddle table

    // device state
    void *d_tw = nullptr;          // [2L] complex
    void *d_prev = nullptr;        // [n_in][L] real
    void *d_ring = nullptr;        // [n_in][N][L] complex
    DevFormat *d_fmt[2] = {nullptr, nullptr};
    DevOverflow *d_over = nullptr;
    int *d_status = nullptr;
    int *d_status_own = nullptr;   // the engine's allocation while d_status points at a caller's word
    int *d_bad = nullptr;
    // partial-sum ring, [n_chunks][n_out_padded][L] complex each: a schedule's block t writes
    // d_Zp[t % zp_depth(e)]; zp_last is the buffer the last MAC (or paired MAC) wrote
    void *d_Zp[3] = {nullptr, nullptr, nullptr};
    int zp_last = 0;
    size_t zp_bytes = 0;
    DevBuf b_entries;                  // MacEntry per entry
    DevBuf b_chunks;                   // ChunkRange per (group, chunk) | d_diag_jobs
    bool zp_is_sum = false;            // chunk 0 of the last block's partial-sum buffer holds the sum over all chunks (sum_chunks in place)
    uint8_t *d_rawin = nullptr, *d_rawout = nullptr;
    size_t raw_bytes[2] = {0, 0};
    DevBuf b_taps;

    // filters that need more than the shared-ring fast path (SURVEY A3 N-way mix, A7, A8)
    std::vector<int> level, owner_index, y_index, sink_index, fade_index;
    std::vector<char> is_source;
    std::vector<void *> promoted;      // private ring given to a shared-ring filter at run time
    int n_levels = 0, n_owners = 0, n_y = 0, n_sinks = 0, n_fadeable = 0;
    void *d_fring = nullptr;       // [n_owners][N][L] complex: private rings
    void *d_Y = nullptr;           // [n_y][L] complex: materialised filter outputs
    void *d_Yold = nullptr;        // [n_fadeable][L] complex: old-coefficient result in a fade block
    void *d_evalprev = nullptr;    // [n_sinks][L] real: previous valid half (convolve_eval state)
    DevBuf b_jobs;                 // fill jobs | mix sources | filter jobs | fade jobs
    struct LevelJobs { size_t fill_off = 0; int n_fill = 0; size_t filt_off = 0; int n_filt = 0;
                       size_t fade_off = 0; int n_fade = 0; };
    std::vector<LevelJobs> level_jobs;
    size_t src_off = 0;
    bool any_fading = false;

    Channels ch;                   // the channel stage (channels.h)

    // plan geometry
    int n_groups = 0, n_out_padded = 0, n_chunks = 1, n_tiles = 1, mac_threads = 256;
    int n_entries = 0;
    bool mac_nt = true;            // non-temporal coefficient loads (BFHIP_MAC_NT=0 turns them off)
    int mac_unroll = 0;            // 0: rotating three-stage pipeline; 1..4: plain unroll (BFHIP_MAC_UNROLL, tools/tune_mac.py)
    // two blocks per pass over the coefficients (bfhip_engine_enable_pairs / bfhip_engine_block_pair_dev)
    bool pairs = false;
    unsigned long long n_pair_launches = 0;
    bool all_dense = false;        // every MAC entry takes the crossbar path
    // one-to-one plans (every output fed by at most one single-term entry per chunk): mac_diag_kernel,
    // one workgroup per (chunk, output) walking whole spectra (BFHIP_MAC_DIAG=0 keeps the crossbar kernel)
    bool mac_diag = false;
    const int *d_diag_jobs = nullptr;      // [n_chunks * n_out_padded] entry index or -1 (lives behind the chunks)
    double alg_bytes_total = 0, alg_bytes_mac = 0;
    // long-window overlap-save (kernels.h: windows of 4 blocks, partitions of 3 blocks of taps).
    // lw_struct: decided at finalize (f32, L = 8192, wave transforms, N >= 8, >= 1 GiB of coefficients in
    // the whole configuration, or BFHIP_LONG_WINDOW=1); then the long transforms run in every block and
    // keep the history and the long ring current.  lw_active: the plan built last covers its blocks with
    // the long MAC (a plain uniform crossbar without fades, private rings, powersave or dither); any
    // other block runs the standard MAC and output pass, which the standard transforms keep exact.
    bool lw_struct = false, lw_active = false;
    void *d_hist = nullptr;        // [n_in][R][L] real blocks
    void *d_lring = nullptr;       // [n_in][R][2L] long window spectra
    void *d_tw14 = nullptr;        // twiddles of the 2L-point complex transform
    DevBuf b_lentries, b_lchunks;
    int lw_chunks = 1, lw_P = 0, lw_tiles = 0, lw_Pstd = 0;     // chunks per group, long / standard partitions, bin tiles
    StreamLayout lstream = {nullptr, 0, 0, 0};
    DevBuf b_lstream;
    DevBuf b_lwhere;                   // StreamWhere per long entry | d_lwhich
    int *d_lwhich = nullptr;
    std::vector<std::array<const void *, OG + 1>> lkeys;     // per long entry: its sets and (delay, length)
    bool zp_long[3] = {false, false, false};                   // d_Zp[i] holds long partial spectra
    // look-ahead long MAC (kernels.h, mac_la_*): call t computes the tails (partitions >= 1) of one slice
    // of entries for blocks t+1 .. t+3 into the ahead buffers b_ahead[block mod 4][slice]; the block's own
    // MAC is then the head pass (partition 0 on top of its three ahead buffers).  la_active: the plan
    // built last may run it (build_long_layout).  The validity table names, per ahead buffer, the block
    // (blocks_done when it runs) it was computed for and the epoch; anything that can change a product
    // already stored bumps the epoch, and a block whose three buffers are not all current runs the full
    // long MAC instead.
    bool la_active = false;
    DevBuf b_ahead;                // [4][3][n_out_padded][2L] complex
    unsigned long long la_epoch = 1;
    unsigned long long la_for[4][3] = {};
    unsigned long long la_at[4][3] = {};       // epoch 0: never written
    // second tier (kernels.h, la_far_phase): partitions >= 2 of one sixth of the entries for blocks t+1 .. t+6
    // into b_far[block mod 7][slice]; the tail pass above is then p = 1 alone.  Same epoch, its own table.
    bool far_active = false;
    DevBuf b_far;                  // [7][6][n_out_padded][2L] complex
    unsigned long long far_for[7][LA_FAR] = {};
    unsigned long long far_at[7][LA_FAR] = {};
    unsigned long long n_la_head = 0, n_la_full = 0;
    unsigned long long n_mac_launches = 0;      // MAC kernels launched by do_mac, of every kind

    // real-time mode (bfhip_engine_rt_*): pinned host double buffer, the block's launch
    // sequence replayed from a HIP graph, completion signalled through pinned memory
    struct Rt {
        bool on = false;
        int flags = 0;
        void *h_in[2] = {nullptr, nullptr}, *h_out[2] = {nullptr, nullptr};
        DevOverflow *h_over[2] = {nullptr, nullptr};
        int *h_status[2] = {nullptr, nullptr};      // [0] status bits, [1] sequence number
        hipGraphExec_t exec[2] = {nullptr, nullptr};
        bool valid[2] = {false, false};
        bool primed = false;                        // one direct block ran since the last plan change
        hipEvent_t done[2] = {nullptr, nullptr};
        unsigned long long submitted = 0, waited = 0;
        unsigned int bs_t = 0;                      // what d_bs->t holds
        bool bs_synced = false;
        unsigned long long n_graph = 0, n_direct = 0, n_capture = 0;
        // what rt_wait last wrote into the caller's overflow array: an entry that differs from it
        // next time was changed by the HOST (bf_reset_peak, bfrun.c: the CLI's peak reset) and
        // becomes the device's state for that output
        std::vector<DevOverflow> last_over;
        std::vector<unsigned long long> over_from;
        bool last_valid = false;
        // BFHIP_RT_OVERLAP: copies of neighbouring periods run on the copy engines beside compute
        hipStream_t s_h2d = nullptr, s_d2h = nullptr;
        hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_cmp[2] = {nullptr, nullptr};
        uint8_t *d_in[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr};
    } rt;
    BlockState *d_bs = nullptr;
    unsigned int *d_rt_arrive = nullptr;
    BlockState *bs_arg = nullptr;      // non-null while a graph is being captured

    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;    // EV_PER_BLOCK per block: start/stop of the EV_PAIRS stages on their streams
    int ev_used = 0;
    int timing_stride = 1;         // time every n-th block (the event records cost ~3 us each)
    bool timed_now = false;
    int timed_mask = 0;            // which of the three kernel pairs of the block in progress were recorded
    unsigned long long timed_for = ~0ull;   // blocks_done the decision above was taken for
    std::vector<unsigned char> ev_mask;     // [MAX_TIMED] timed_mask of every timed block

    size_t csize() const { return (size_t)2 * rs; }     // bytes per complex
};

BFHIP_HOST_NS {

const void *const STREAM_KEY_STALE = (const void *)(uintptr_t)1;     // never a set's address
void *const PROMOTED_ELSEWHERE = (void *)(uintptr_t)1;               // promoted[] of an inactive filter: no ring here
constexpr int LW_LOG2 = 14;        // the 4B-point real transform of B = 8192: 2^14 complex points

// raise a kernel's dynamic-LDS limit once per (device, kernel, size): the attribute call costs a
// few microseconds, which is real money in a 35 us block
template <typename K> hipError_t allow_lds(K kernel, size_t bytes) {
    static std::mutex mu;
    static std::set<std::tuple<int, const void *, size_t>> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const auto key = std::make_tuple(dev, reinterpret_cast<const void *>(kernel), bytes);
    std::lock_guard<std::mutex> lock(mu);
    if (done.count(key)) return hipSuccess;
    const hipError_t r = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (r == hipSuccess) done.insert(key);
    return r;
}

// bfhip.hip
int sync_all(bfhip_engine *e);
int zp_depth(const bfhip_engine *e);
int coeff_make_resident(bfhip_engine *e, int ci);

// passes.hip (what the plan builder needs of it; the rest: passes.h)
int la_prime(bfhip_engine *e);

// plan.hip
int clamp_delay(const bfhip_engine *e, int d);
int cblocks_of(const bfhip_engine *e, int coeff, int delay);
int build_plan(bfhip_engine *e);
int long_refresh_block(bfhip_engine *e, const void *H, int block);
template <typename T> int stream_refresh_block(bfhip_engine *e, const void *H, int block);

}  // namespace bfhip_host
