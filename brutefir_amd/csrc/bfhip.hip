// bfhip.hip -- host side of the engine + the C ABI of include/bfhip.h (the plan builder: plan.hip; the
// channel stage around the transforms: channels.hip; every kernel launch: passes.hip -- this unit names no
// kernel and holds no device code).
//
// What the reference's filter_process() does with host buffers and a chain of convolver_*
// calls per filter (bfrun.c:1493-2008) is turned into a static device plan here:
//   * every input channel owns one ring of its last N spectra in HBM (the reference keeps one
//     ring per filter, bfrun.c:1273-1287; filters that only scale a single input share the
//     input's ring and carry their scale in the plan -> the ring is read once per output
//     group instead of once per filter);
//   * every output group owns a list of (ring, delay) entries with up to 8 filter terms each;
//   * a block is three launches: fft_in (K1), mac_xbar (K2), ifft_out (K3).
// The integer bookkeeping (slot = blockcounter mod N, delay clamp, cblocks truncation,
// warm-up count) follows bfrun.c:1566-1600,1745-1746 literally.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <deque>
#include <map>
#include <string>
#include <vector>
#include <mutex>
#include <set>
#include <tuple>
#include <type_traits>

#include "engine.h"
#include "passes.h"
#include "coeff_async.h"
#include "conv_shared.h"
#include "dither_init.h"
#include "subdelay_filter.h"
#include "bigfft.h"

// what the allocation wrappers of engine.h end in (alloc.h)
static int g_fail_alloc = 0;           // countdown: the allocation that takes it to zero fails
static inline bool alloc_injected() { return g_fail_alloc > 0 && --g_fail_alloc == 0; }
extern "C" hipError_t bfhip_internal_dev_alloc(void **p, size_t bytes) {
    if (alloc_injected()) { *p = nullptr; return hipErrorOutOfMemory; }
    return hipMalloc(p, bytes);
}
extern "C" hipError_t bfhip_internal_pin_alloc(void **p, size_t bytes, unsigned int flags) {
    if (alloc_injected()) { *p = nullptr; return hipErrorOutOfMemory; }
    return hipHostMalloc(p, bytes, flags);
}

namespace {
thread_local std::string g_err;
}  // namespace

BFHIP_HOST_NS {

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    // a failed runtime call (an allocation that did not fit, say) leaves its code behind as the
    // "last error"; reported here, it must not be found again by the launch check of a later,
    // unrelated call.  Only the two codes a runtime failure is reported under reach the runtime:
    // argument and state errors (a NULL handle, the fork()ed-child refusal of check_owner) return
    // without a single HIP call.
    if (code == BFHIP_EHIP || code == BFHIP_ENOMEM) (void)hipGetLastError();
    return code;
}

int sync_all(bfhip_engine *e) {
    if (e->s_in) HIPCHK(hipStreamSynchronize(e->s_in));
    if (e->stream) HIPCHK(hipStreamSynchronize(e->stream));
    if (e->s_out) HIPCHK(hipStreamSynchronize(e->s_out));
    return BFHIP_OK;
}

// partial-sum buffers a schedule cycles through: the MAC of block t writes one while the output passes
// of the blocks before it still read the others (a pair writes two at once)
int zp_depth(const bfhip_engine *e) {
    const int d = e->mode == BFHIP_MODE_PINGPONG ? 3 : e->mode == BFHIP_MODE_SEQUENTIAL ? 1 : 2;
    return e->pairs ? std::max(d, 2) : d;
}

}  // namespace bfhip_host

namespace {

int ilog2(int v) {
    int o = 0;
    while ((1 << o) < v) o++;
    return ((1 << o) == v) ? o : -1;
}

// the streams a block's input and output passes go to, and how many calls its output is owed for
hipStream_t in_stream(const bfhip_engine *e) {
    return e->mode == BFHIP_MODE_PIPELINED || e->mode == BFHIP_MODE_PINGPONG ? e->s_in : e->stream;
}
hipStream_t out_stream(const bfhip_engine *e) {
    return e->mode == BFHIP_MODE_PIPELINED ? e->s_out : e->mode == BFHIP_MODE_PINGPONG ? e->s_in : e->stream;
}
int output_lag(const bfhip_engine *e) {
    return e->mode == BFHIP_MODE_PINGPONG ? 2 : e->mode == BFHIP_MODE_DEFERRED ? 1 : 0;
}

// ---------------------------------------------------------------- coefficient memory

void *coeff_alloc(bfhip_engine *e, size_t bytes) {
    if (!e->coeff_arena) {
        void *p = nullptr;
        return dev_alloc(&p, bytes) == hipSuccess ? p : nullptr;
    }
    size_t need = (bytes + 65535) & ~(size_t)65535;                // sets start on 64 KiB
    size_t skew = 0;
    if (const char *env = getenv("BFHIP_COEFF_PAD_B")) {
        if (env[0] == 'r') {
            // pseudo-random start inside an extra 64 KiB (256-byte steps)
            e->skew_state = e->skew_state * 1664525u + 1013904223u;
            skew = (size_t)((e->skew_state >> 16) & 255u) * 256;
            need = ((bytes + 255) & ~(size_t)255) + 65536;
        } else need = (bytes + (size_t)atol(env) + 255) & ~(size_t)255;
    }
    if (!e->slabs.empty()) {
        auto &sl = e->slabs.back();
        if (sl.cap - sl.used >= need) { void *p = (unsigned char *)sl.base + sl.used + skew; sl.used += need; return p; }
    }
    // a first slab of 64 MiB keeps small engines small; whoever needs more gets 2 GiB pieces
    // (config C, MAC alone, one box: one hipMalloc per set 0.83 of peak, 512 MiB slabs 0.86,
    // >= 2 GiB slabs 0.883-0.886).  A host that knows the total calls bfhip_engine_reserve_coeffs.
    size_t cap = e->slabs.empty() ? ((size_t)64 << 20) : ((size_t)2 << 30);
    if (const char *env = getenv("BFHIP_COEFF_SLAB_MB")) cap = (size_t)std::max(1, atoi(env)) << 20;
    cap = std::max(cap, need);
    bfhip_engine::Slab sl;
    while (dev_alloc(&sl.base, cap) != hipSuccess) {
        (void)hipGetLastError();
        if (cap <= need) return nullptr;
        cap = std::max(need, cap / 2);
    }
    sl.cap = cap; sl.used = need;
    e->slabs.push_back(sl);
    return (unsigned char *)sl.base + skew;
}

// give back a set that was allocated last (error paths); anything else stays with its slab
void coeff_release(bfhip_engine *e, void *p, size_t bytes) {
    if (!p) return;
    if (!e->coeff_arena) { (void)hipFree(p); return; }
    if (e->slabs.empty()) return;
    auto &sl = e->slabs.back();
    const size_t need = (bytes + 65535) & ~(size_t)65535;
    if (sl.used >= need && (unsigned char *)sl.base + sl.used - need == (unsigned char *)p) sl.used -= need;
}

// the staging buffer for taps and processed blocks on their way to or from a set: `bytes` of it, and
// nothing on the device still reading the one it replaces
int taps_reserve(bfhip_engine *e, size_t bytes) {
    if (bytes <= e->b_taps.cap) return BFHIP_OK;
    if (e->b_taps.p) { const int r = sync_all(e); if (r != BFHIP_OK) return r; }
    HIPCHK(e->b_taps.grow(bytes));
    return BFHIP_OK;
}

size_t raw_extent(const std::vector<bfhip_format> &v, int n, int L) {
    size_t m = 0;
    for (int i = 0; i < n; i++) {
        const bfhip_format &f = v[i];
        const size_t end = (size_t)f.byte_offset + ((size_t)(L - 1) * f.sample_spacing + 1) * f.bytes;
        m = std::max(m, end);
    }
    return m;
}

double overflow_max(const bfhip_format &f) {             // bfrun.c:2270-2277
    return f.isfloat ? 1.0 : (double)((uint64_t)1 << ((f.sbytes << 3) - 1)) - 1;
}

int check_format(const bfhip_format *f) {
    if (f->isfloat) {
        if (f->bytes != 4 && f->bytes != 8) return 0;
    } else if (f->bytes < 1 || f->bytes > 4 || f->sbytes < 1 || f->sbytes > f->bytes) {
        return 0;
    }
    return f->sample_spacing >= 1 && f->byte_offset >= 0;
}

// is the block in progress one of the timed ones?  Decided once per block, by whichever entry
// point touches it first (block_dev, or the phase calls of a multi-GPU host).
void timing_begin(bfhip_engine *e) {
    if (e->timed_for == e->blocks_done) return;
    e->timed_for = e->blocks_done;
    e->timed_mask = 0;
    e->timed_now = e->timing && e->ev_used < MAX_TIMED && e->blocks_done % (unsigned long long)e->timing_stride == 0;
}

int poll_coeff_changes(bfhip_engine *e);

// restores "the next launch goes to the main stream" on every return path of a schedule that sends
// launches to a side stream (an error in the middle must not leave e->ls pointing there: the do_*
// helpers of the phase entry points launch on e->ls)
struct LsGuard {
    bfhip_engine *e;
    ~LsGuard() { e->ls = e->stream; }
};

// the inverse transforms of the blocks whose output is still owed (deferred output: one, ping-pong
// schedule: up to two), oldest first, each as a launch of its own
int flush_pending(bfhip_engine *e) {
    LsGuard guard{e};                  // every return path leaves the launch stream on the main stream
    const bool side = e->mode == BFHIP_MODE_PINGPONG && !e->pendq.empty();
    while (!e->pendq.empty()) {
        // (popped only once its launch is in the stream: a failed launch leaves the owed output
        // queued -- the caller sees the error, and the entry's event is never silently dropped)
        const bfhip_engine::Pending p = e->pendq.front();
        // the ping-pong schedule keeps every output pass on the side stream (their overflow state
        // and the dither chains are sequential), behind the MAC that produced the spectra
        e->ls = out_stream(e);
        if (p.mac_done) HIPCHK(hipStreamWaitEvent(e->ls, p.mac_done, 0));
        const int r = do_outputs(e, p.Zp, p.chunk_stride, p.n_chunks, 0, e->n_ch[1], p.rawout);
        if (r != BFHIP_OK) return r;
        e->pendq.pop_front();
        if (p.out_done) HIPCHK(hipEventRecord(p.out_done, e->ls));
    }
    e->ls = e->stream;
    if (side) {
        // whatever the main stream does next (a phase call's MAC writes the partial-sum buffer these
        // output passes read) comes behind them
        HIPCHK(hipEventRecord(e->ev_io[0], e->s_in));
        HIPCHK(hipStreamWaitEvent(e->stream, e->ev_io[0], 0));
    }
    return BFHIP_OK;
}

// An engine is usable in the process that created it only: a fork()ed child inherits the handle but
// not a working HIP runtime, and its first device call would hang.  Checked before anything else.
int check_owner(const bfhip_engine *e) {
    if (e->owner != getpid())
        return fail(BFHIP_ESTATE, "this engine belongs to process %d: HIP state does not survive fork(); create the "
                    "engine in the process that runs the blocks", (int)e->owner);
    return BFHIP_OK;
}

int ensure_ready(bfhip_engine *e) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    if (!e->finalized) return fail(BFHIP_ESTATE, "engine not finalized");
    HIPCHK(hipSetDevice(e->device));
    if (e->plan_dirty && !e->pendq.empty()) {
        // the owed output belongs to the old plan's geometry and buffers
        const int r = flush_pending(e);
        if (r != BFHIP_OK) return r;
    }
    if (e->any_watched) {
        // one load of a shared counter per block; a partition another process rewrote since the
        // last block is re-uploaded now, before this block's plan / coefficient switch is applied
        const int r = poll_coeff_changes(e);
        if (r < 0) return r;
    }
    if (e->plan_dirty) {
        e->rt.valid[0] = e->rt.valid[1] = false;     // captured launches point into the old plan
        e->rt.primed = false;
        return build_plan(e);
    }
    return BFHIP_OK;
}

// The three passes of a block with their timing records, each on e->ls: a schedule switches streams
// and adds its waits and event records between them.
int block_inputs(bfhip_engine *e, const void *rawin_dev) {
    int r;
    if ((r = record_begin(e, T_IN)) != BFHIP_OK) return r;
    if ((r = do_inputs(e, rawin_dev)) != BFHIP_OK) return r;
    return record_end(e, T_IN);
}
int block_mac(bfhip_engine *e, int zi) {
    int r;
    if ((r = do_levels(e)) != BFHIP_OK) return r;
    if ((r = record_begin(e, T_MAC)) != BFHIP_OK) return r;
    if ((r = do_mac(e, e->d_Zp[zi])) != BFHIP_OK) return r;
    e->zp_last = zi;
    return record_end(e, T_MAC);
}
int block_outputs(bfhip_engine *e, int zi, void *rawout_dev) {
    int r;
    if ((r = record_begin(e, T_OUT)) != BFHIP_OK) return r;
    if ((r = do_outputs(e, e->d_Zp[zi], (size_t)e->n_out_padded * e->L, e->n_chunks, 0, e->n_ch[1], rawout_dev)) != BFHIP_OK) return r;
    return record_end(e, T_OUT);
}
// inputs -> levels -> MAC -> outputs of one block, in order on e->ls
int block_in_order(bfhip_engine *e, const void *rawin_dev, int zi, void *rawout_dev) {
    int r;
    if ((r = block_inputs(e, rawin_dev)) != BFHIP_OK) return r;
    if ((r = block_mac(e, zi)) != BFHIP_OK) return r;
    return block_outputs(e, zi, rawout_dev);
}

void advance(bfhip_engine *e) {
    if (e->timed_now) {
        if (e->timed_mask) { e->ev_mask[e->ev_used] = (unsigned char)e->timed_mask; e->ev_used++; }
        e->timed_now = false;
    }
    e->blockcounter++;                                   // bfrun.c:2034
    if (e->wrap_by != 0u && e->blockcounter >= e->wrap_at) e->blockcounter -= e->wrap_by;
    e->blocks_done++;
    for (auto &f : e->filters) f.prevcoeff = f.coeff;    // bfrun.c:1838
    if (e->any_fading) e->plan_dirty = true;             // the fade lasts exactly one block
}

// Re-upload the watched partitions whose change notice moved (bfhip_coeff_mark_dirty, written by
// convolver_runtime_coeffs2cbuf in whichever process renders new coefficients).  Returns the
// number of partitions refreshed.
int poll_coeff_changes(bfhip_engine *e) {
    const unsigned long long seq = bfhip_coeff_dirty_sequence();
    if (seq == e->watch_seq) return 0;
    e->watch_seq = seq;
    const unsigned long long lost = bfhip_dirty_lost();
    const bool all = lost != e->watch_lost;             // a notice found no slot: trust nothing
    e->watch_lost = lost;
    int n = 0;
    for (size_t ci = 0; ci < e->coeffs.size(); ci++) {
        Coeff &c = e->coeffs[ci];
        if (c.lazy && !c.watched) continue;                     // host pointers kept for the first load only
        for (size_t b = 0; b < c.watch_src.size(); b++) {
            const uint64_t gen = bfhip_dirty_generation(c.watch_src[b]);
            if (gen == c.watch_gen[b] && !all) continue;
            c.watch_gen[b] = gen;
            const int r = bfhip_engine_refresh_coeff_processed(e, (int)ci, (int)b, c.watch_src[b]);
            if (r != BFHIP_OK) return r;
            n++;
        }
    }
    return n;
}

// ---------------------------------------------------------------- real-time mode

void rt_release(bfhip_engine *e) {
    auto &rt = e->rt;
    for (int p = 0; p < 2; p++) {
        if (rt.exec[p]) (void)hipGraphExecDestroy(rt.exec[p]);
        if (rt.done[p]) (void)hipEventDestroy(rt.done[p]);
        if (rt.h_in[p]) (void)hipHostFree(rt.h_in[p]);
        if (rt.h_out[p]) (void)hipHostFree(rt.h_out[p]);
        if (rt.h_over[p]) (void)hipHostFree(rt.h_over[p]);
        if (rt.h_status[p]) (void)hipHostFree(rt.h_status[p]);
        if (rt.ev_h2d[p]) (void)hipEventDestroy(rt.ev_h2d[p]);
        if (rt.ev_cmp[p]) (void)hipEventDestroy(rt.ev_cmp[p]);
        if (rt.d_in[p]) (void)hipFree(rt.d_in[p]);
        if (rt.d_out[p]) (void)hipFree(rt.d_out[p]);
    }
    if (rt.s_h2d) (void)hipStreamDestroy(rt.s_h2d);
    if (rt.s_d2h) (void)hipStreamDestroy(rt.s_d2h);
    if (e->d_bs) (void)hipFree(e->d_bs);
    if (e->d_rt_arrive) (void)hipFree(e->d_rt_arrive);
    e->d_bs = nullptr;
    e->d_rt_arrive = nullptr;
    rt = bfhip_engine::Rt();
}

// can this plan's launch sequence be replayed unchanged block after block?
bool rt_graphable(const bfhip_engine *e) {
    if ((e->rt.flags & (BFHIP_RT_NO_GRAPH | BFHIP_RT_OVERLAP)) || e->big) return false;
    // N:1 channels and sub-sample delays upload a per-block job table; a cross-fade lasts one block
    return !e->ch.has_vchan && !e->any_fading;
}

// Throughput with host buffers: upload of period t+1 and download of period t-1 on the copy
// engines (their own streams) while period t computes -- the reference's input / filter / output
// process pipeline over its two buffer halves (bfrun.c:2031, 2312-2616).  Two periods must be
// in flight for the overlap to happen (rt_submit before rt_wait of the previous one).
int rt_enqueue_overlap(bfhip_engine *e, int p) {
    auto &rt = e->rt;
    int r;
    HIPCHK(hipMemcpyAsync(rt.d_in[p], rt.h_in[p], e->raw_bytes[0], hipMemcpyHostToDevice, rt.s_h2d));
    HIPCHK(hipEventRecord(rt.ev_h2d[p], rt.s_h2d));
    e->ls = e->stream;
    HIPCHK(hipStreamWaitEvent(e->stream, rt.ev_h2d[p], 0));
    if ((r = block_in_order(e, rt.d_in[p], 0, rt.d_out[p])) != BFHIP_OK) return r;
    RtCopy none;
    none.dst = nullptr; none.src = nullptr; none.n16 = 0; none.pad = 0;
    if ((r = rt_tail(e, 1u, none, p)) != BFHIP_OK) return r;
    HIPCHK(hipEventRecord(rt.ev_cmp[p], e->stream));
    HIPCHK(hipStreamWaitEvent(rt.s_d2h, rt.ev_cmp[p], 0));
    HIPCHK(hipMemcpyAsync(rt.h_out[p], rt.d_out[p], e->raw_bytes[1], hipMemcpyDeviceToHost, rt.s_d2h));
    HIPCHK(hipEventRecord(rt.done[p], rt.s_d2h));
    return BFHIP_OK;
}

// the launch sequence of one block on the main stream: pinned in -> device -> pinned out
int rt_enqueue(bfhip_engine *e, int p) {
    auto &rt = e->rt;
    int r;
    if (rt.flags & BFHIP_RT_OVERLAP) return rt_enqueue_overlap(e, p);
    e->ls = e->stream;
    const bool nodes = (rt.flags & BFHIP_RT_COPY_ENGINE) != 0;
    RtCopy cin, cout;
    cin.dst = (uint4 *)e->d_rawin; cin.src = (const uint4 *)rt.h_in[p];
    cin.n16 = (unsigned int)((e->raw_bytes[0] + 15) / 16); cin.pad = 0;
    cout.dst = (uint4 *)rt.h_out[p]; cout.src = (const uint4 *)e->d_rawout;
    cout.n16 = nodes ? 0u : (unsigned int)((e->raw_bytes[1] + 15) / 16); cout.pad = 0;
    if (nodes) {
        HIPCHK(hipMemcpyAsync(e->d_rawin, rt.h_in[p], e->raw_bytes[0], hipMemcpyHostToDevice, e->stream));
    } else if ((r = rt_copy_in(e, cin)) != BFHIP_OK) {
        return r;
    }
    // (plain launches of a timed engine -- bfhip_engine_enable_timing; `benchmark: true` hosts ask for
    // BFHIP_RT_NO_GRAPH -- are bracketed by events like bfhip_engine_block_dev's; captured ones are not)
    if ((r = block_in_order(e, e->d_rawin, 0, e->d_rawout)) != BFHIP_OK) return r;
    if (nodes) HIPCHK(hipMemcpyAsync(rt.h_out[p], e->d_rawout, e->raw_bytes[1], hipMemcpyDeviceToHost, e->stream));
    return rt_tail(e, nodes ? 1u : (cout.n16 + 255) / 256, cout, p);
}

int rt_capture(bfhip_engine *e, int p) {
    auto &rt = e->rt;
    if (rt.exec[p]) { (void)hipGraphExecDestroy(rt.exec[p]); rt.exec[p] = nullptr; }
    HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeRelaxed));
    e->bs_arg = e->d_bs;
    const int r = rt_enqueue(e, p);
    e->bs_arg = nullptr;
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(e->stream, &g);
    if (r != BFHIP_OK) { if (g) (void)hipGraphDestroy(g); return r; }
    if (ce != hipSuccess) return fail(BFHIP_EHIP, "graph capture: %s", hipGetErrorString(ce));
    const hipError_t ie = hipGraphInstantiate(&rt.exec[p], g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess) { rt.exec[p] = nullptr; return fail(BFHIP_EHIP, "graph instantiate: %s", hipGetErrorString(ie)); }
    rt.valid[p] = true;
    rt.n_capture++;
    return BFHIP_OK;
}

}  // namespace

// ==================================================================== C ABI

extern "C" {

const char *bfhip_last_error(void) { return g_err.c_str(); }
const char *bfhip_version(void) { return "bfhip 0.1 (gfx950)"; }

int bfhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

bfhip_engine *bfhip_engine_create(int device, int length, int n_blocks, int realsize,
                                  int n_in, int n_out) {
    if (realsize != 4 && realsize != 8) { fail(BFHIP_EINVAL, "Invalid real size %d.", realsize); return nullptr; }
    const int lg = ilog2(length);
    if (lg < 2 || lg > 20) {
        fail(BFHIP_EINVAL, "Invalid length %d (power of two in 4..1048576 required).", length);
        return nullptr;
    }
    if (n_blocks < 1 || n_in < 1 || n_out < 1) { fail(BFHIP_EINVAL, "bad n_blocks/n_in/n_out"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fail(BFHIP_ENODEV, "no HIP device available (there is no CPU fallback)");
        return nullptr;
    }
    if (device < 0 || device >= ndev) { fail(BFHIP_ENODEV, "device %d out of range (%d devices)", device, ndev); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { fail(BFHIP_ENODEV, "hipSetDevice(%d) failed", device); return nullptr; }

    bfhip_engine *e = new bfhip_engine();
    e->device = device; e->L = length; e->N = n_blocks; e->rs = realsize; e->log2L = lg;
    e->owner = getpid();
    e->big = lg > BIG_LOG2M;
    e->big_R = e->big ? length / BIG_M : 1;
    e->n_ch[0] = n_in; e->n_ch[1] = n_out;
    for (int io = 0; io < 2; io++) {
        e->fmt[io].resize(e->n_ch[io]);
        for (int c = 0; c < e->n_ch[io]; c++) {
            bfhip_format &f = e->fmt[io][c];
            f.isfloat = 1; f.swap = 0; f.bytes = f.sbytes = realsize; f.scale = 1.0;
            f.sample_spacing = 1; f.byte_offset = c * length * realsize;
        }
    }
    e->ch.init(e->n_ch);
    bool ok = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) == hipSuccess;
    e->own_stream = ok;
    // twiddles exp(-2 pi i m / (2L)), computed in double, + their thread-ordered copy (fft_lds.h)
    int log2l = 0;
    while ((1 << log2l) < length) log2l++;
    const std::vector<unsigned char> tw = make_twiddle_table(log2l, realsize,
        realsize == 4 ? fft_threads<float>(log2l) : fft_threads<double>(log2l));
    ok = ok && dev_alloc(&e->d_tw, tw.size()) == hipSuccess;
    ok = ok && hipMemcpy(e->d_tw, tw.data(), tw.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (e->big) {
        const std::vector<unsigned char> tw13 = make_twiddle_table(BIG_LOG2M, realsize,
            realsize == 4 ? fft_threads<float>(BIG_LOG2M) : fft_threads<double>(BIG_LOG2M));
        ok = ok && dev_alloc(&e->d_tw13, tw13.size()) == hipSuccess;
        ok = ok && hipMemcpy(e->d_tw13, tw13.data(), tw13.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    // default from L = 4096 up: below that a workgroup of L/16 threads is one or two waves and the
    // plain LDS transform with twice the threads has the shorter critical path (tools/fft_probe:
    // L = 2048 5.6 vs 6.3 us, L = 1024 4.5 vs 5.4 us); BFHIP_FFT_WAVE=1 forces it on, =0 off
    if (const char *env = getenv("BFHIP_COEFF_ARENA")) e->coeff_arena = atoi(env) != 0;
    if (const char *env = getenv("BFHIP_COEFF_STREAM")) e->stream_wanted = atoi(env);
    e->wave = wave_fft_ok(lg, realsize) && lg >= 12;
    if (const char *env = getenv("BFHIP_FFT_WAVE")) e->wave = wave_fft_ok(lg, realsize) && atoi(env) != 0;
    if (e->wave) {
        const std::vector<unsigned char> tww = make_wave_twiddle_table(lg, realsize);
        ok = ok && dev_alloc(&e->d_tww, tww.size()) == hipSuccess;
        ok = ok && hipMemcpy(e->d_tww, tww.data(), tww.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && dev_alloc((void **)&e->d_bad, sizeof(int)) == hipSuccess;
    ok = ok && hipMemset(e->d_bad, 0, sizeof(int)) == hipSuccess;
    if (!ok) {
        const hipError_t le = hipGetLastError();
        fail(BFHIP_EHIP, "device set-up failed: %s", le == hipSuccess ? "out of device memory" : hipGetErrorString(le));
        bfhip_engine_destroy(e);
        return nullptr;
    }
    return e;
}

void bfhip_engine_destroy(bfhip_engine *e) {
    if (e == nullptr) return;
    if (e->owner != getpid()) { delete e; return; }     // a forked child: the device objects are the parent's
    (void)hipSetDevice(e->device);
    e->pendq.clear();
    (void)sync_all(e);
    if (e->coeff_arena) { for (auto &sl : e->slabs) if (sl.base) (void)hipFree(sl.base); }
    else { for (auto &c : e->coeffs) if (c.d_H) (void)hipFree(c.d_H); }
    for (void *p : e->promoted) if (p && p != PROMOTED_ELSEWHERE) (void)hipFree(p);
    e->ch.release();
    rt_release(e);
    for (void *z : e->d_Zp) if (z) (void)hipFree(z);
    for (int i = 0; i < 2; i++) {
        if (e->ev_in[i]) (void)hipEventDestroy(e->ev_in[i]);
        if (e->ev_mac[i]) (void)hipEventDestroy(e->ev_mac[i]);
        if (e->ev_out[i]) (void)hipEventDestroy(e->ev_out[i]);
        if (e->ev_io[i]) (void)hipEventDestroy(e->ev_io[i]);
    }
    for (int i = 0; i < 3; i++) if (e->ev_mac3[i]) (void)hipEventDestroy(e->ev_mac3[i]);
    if (e->s_in) (void)hipStreamDestroy(e->s_in);
    if (e->s_out) (void)hipStreamDestroy(e->s_out);
    if (e->d_status_own) e->d_status = e->d_status_own;
    void *ptrs[] = {e->d_tw, e->d_prev, e->d_ring, e->d_fmt[0], e->d_fmt[1], e->d_over, e->d_status,
                    e->d_bad, e->d_rawin, e->d_rawout,
                    e->d_fring, e->d_Y, e->d_Yold, e->d_evalprev,
                    e->d_tw13, e->d_tww,
                    e->d_ps_flags, e->d_ps_live, e->d_ps_scale, e->d_ps_acc,
                    e->d_hist, e->d_lring, e->d_tw14};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    for (DevBuf *b : {&e->b_entries, &e->b_chunks, &e->b_jobs, &e->b_stream, &e->b_where, &e->b_lentries, &e->b_lchunks,
                      &e->b_lstream, &e->b_lwhere, &e->b_ahead, &e->b_far, &e->b_taps, &e->b_big[0], &e->b_big[1], &e->b_big[2]})
        b->release();
    for (auto ev : e->ev) (void)hipEventDestroy(ev);
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int bfhip_engine_set_format(bfhip_engine *e, int io, int ch, const bfhip_format *bf) {
    if (!e || !bf || io < 0 || io > 1 || ch < 0 || ch >= e->ch.n_phys[io]) return fail(BFHIP_EINVAL, "set_format: bad argument");
    if (!check_format(bf)) return fail(BFHIP_EINVAL, "Sample byte size %d is not supported.", bf->bytes);
    if (e->finalized) return fail(BFHIP_ESTATE, "set_format after finalize");
    e->fmt[io][ch] = *bf;
    return BFHIP_OK;
}

int bfhip_engine_set_overlap(bfhip_engine *e, int mode) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    if (e->finalized) return fail(BFHIP_ESTATE, "set_overlap after finalize");
    e->overlap_mode = mode;
    return BFHIP_OK;
}

int bfhip_engine_set_safety_limit(bfhip_engine *e, double limit) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    e->safety_limit = limit;
    return BFHIP_OK;
}

int bfhip_engine_set_powersave(bfhip_engine *e, double analog_powersave) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    if (e->finalized) return fail(BFHIP_ESTATE, "set_powersave after finalize");
    if (analog_powersave < 0.0) return fail(BFHIP_EINVAL, "set_powersave: negative noise floor");
    e->powersave = analog_powersave;
    return BFHIP_OK;
}

int bfhip_engine_map_channels(bfhip_engine *e, int io, int n_phys, const int virt2phys[]) {
    if (!e || io < 0 || io > 1 || !virt2phys || n_phys < 1 || n_phys > e->n_ch[io]) return fail(BFHIP_EINVAL, "map_channels: bad argument");
    if (e->finalized) return fail(BFHIP_ESTATE, "map_channels after finalize");
    std::vector<int> cnt(n_phys, 0);
    for (int v = 0; v < e->n_ch[io]; v++) {
        if (virt2phys[v] < 0 || virt2phys[v] >= n_phys) return fail(BFHIP_EINVAL, "map_channels: physical channel %d", virt2phys[v]);
        cnt[virt2phys[v]]++;
    }
    for (int c = 0; c < n_phys; c++) if (cnt[c] == 0) return fail(BFHIP_EINVAL, "map_channels: physical channel %d unused", c);
    e->ch.n_phys[io] = n_phys;
    e->ch.v2p[io].assign(virt2phys, virt2phys + e->n_ch[io]);
    e->ch.n_vpp[io] = cnt;
    return BFHIP_OK;
}

// one value of one virtual channel; `fixed`: not after finalize
static int set_channel(bfhip_engine *e, int io, int ch, const char *what, bool fixed, std::vector<int> (Channels::*field)[2], int value) {
    if (!e || io < 0 || io > 1 || ch < 0 || ch >= e->n_ch[io]) return fail(BFHIP_EINVAL, "%s: bad argument", what);
    if (fixed && e->finalized) return fail(BFHIP_ESTATE, "%s after finalize", what);
    (e->ch.*field)[io][ch] = value;
    return BFHIP_OK;
}
int bfhip_engine_set_delay(bfhip_engine *e, int io, int ch, int delay) {
    if (delay < 0) return fail(BFHIP_EINVAL, "set_delay: bad argument");
    return set_channel(e, io, ch, "set_delay", false, &Channels::vdelay, delay);
}
int bfhip_engine_set_maxdelay(bfhip_engine *e, int io, int ch, int maxdelay) { return set_channel(e, io, ch, "set_maxdelay", true, &Channels::vmaxdelay, maxdelay); }
int bfhip_engine_set_mute(bfhip_engine *e, int io, int ch, int muted) { return set_channel(e, io, ch, "set_mute", false, &Channels::vmuted, muted != 0); }
int bfhip_engine_set_subdelay(bfhip_engine *e, int io, int ch, int subdelay) { return set_channel(e, io, ch, "set_subdelay", false, &Channels::subdelay, subdelay); }

int bfhip_engine_enable_subdelay(bfhip_engine *e, int sdf_length, double kaiser_beta) {
    (void)kaiser_beta;       // parsed by the reference (sdf_beta) but its filters are built with 9 (delay.c:73)
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    if (e->finalized) return fail(BFHIP_ESTATE, "enable_subdelay after finalize");
    if (sdf_length < 1) return fail(BFHIP_EINVAL, "Invalid half filter length %d.", sdf_length);
    if (2 * sdf_length + 1 > e->L) return fail(BFHIP_EINVAL, "The filter_length must be at least 2 x sdf_length + 1.");
    int bs = 1;
    while (bs < 2 * sdf_length + 1) bs <<= 1;
    if (e->L % bs != 0) return fail(BFHIP_EINVAL, "Incompatible fragment/filter sizes (%d/%d).", e->L, 2 * sdf_length + 1);
    // the FIR keeps bs frames of history in LDS beside the tile it filters (subdelay_fir_kernel)
    if (sd_tile_frames(e->L, bs, e->rs) == 0)
        return fail(BFHIP_EINVAL, "sdf_length %d is too long for the sub-sample delay filter: its %d-frame history "
                                  "leaves no room in %d KiB of LDS.", sdf_length, bs, SD_LDS_BYTES / 1024);
    e->ch.sdf_length = sdf_length; e->ch.sd_flen = 2 * sdf_length + 1; e->ch.sd_bs = bs;
    return BFHIP_OK;
}

int bfhip_engine_enable_dither(bfhip_engine *e, const int out_channels[], int n,
                               int sample_rate, int max_size) {
    if (!e || !out_channels || n < 1 || sample_rate < 1) return fail(BFHIP_EINVAL, "enable_dither: bad argument");
    if (e->finalized) return fail(BFHIP_ESTATE, "enable_dither after finalize");
    std::vector<int> chs(out_channels, out_channels + n);
    for (int i = 0; i < n; i++) {
        if (chs[i] < 0 || chs[i] >= e->ch.n_phys[1]) return fail(BFHIP_EINVAL, "enable_dither: output channel %d", chs[i]);
        if (i > 0 && chs[i] <= chs[i - 1]) return fail(BFHIP_EINVAL, "enable_dither: channels must be ascending");
        if (e->fmt[1][chs[i]].isfloat) return fail(BFHIP_EINVAL, "cannot dither floating point format (output %d)", chs[i]);
    }
    // dither_init (dither.c:75-139): table spacing, Tausworthe bytes
    const std::string msg = dither_make_table(n, sample_rate, max_size, e->L, &e->ch.dither_spacing, &e->ch.dither_table);
    if (!msg.empty()) return fail(BFHIP_EINVAL, "%s", msg.c_str());
    e->ch.dither_channels = chs;
    return BFHIP_OK;
}

static int add_coeff_common(bfhip_engine *e, const void *taps, bool on_device, int n_taps,
                            double scale, int n_blocks) {
    if (!e || (!taps && n_taps > 0) || n_taps < 0) return fail(BFHIP_EINVAL, "add_coeff: bad argument");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    const int L = e->L;
    if (n_blocks <= 0) n_blocks = (n_taps + L - 1) / L;
    if (n_blocks < 1) n_blocks = 1;
    if (n_blocks > e->N) return fail(BFHIP_EINVAL, "coefficient set needs %d blocks, engine has %d", n_blocks, e->N);
    if (n_taps > n_blocks * L) n_taps = n_blocks * L;
    const void *src = taps;
    // Device taps: whatever produced them ran on a stream this engine knows nothing about (its own
    // stream is non-blocking: not even the legacy default stream orders with it).  Loading is not
    // the hot path: wait for the device before reading them, and for this engine's kernel before
    // returning -- the buffer is the caller's again when the call returns.
    if (on_device) HIPCHK(hipDeviceSynchronize());
    if (!on_device && n_taps > 0) {
        const size_t bytes = (size_t)n_taps * e->rs;
        { const int rt = taps_reserve(e, bytes); if (rt != BFHIP_OK) return rt; }
        { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
        HIPCHK(hipMemcpy(e->b_taps.p, taps, bytes, hipMemcpyHostToDevice));
        src = e->b_taps.p;
    }
    Coeff c;
    c.n_blocks = n_blocks;
    const size_t h_bytes = (size_t)n_blocks * L * e->csize();
    if ((c.d_H = coeff_alloc(e, h_bytes)) == nullptr)
        return fail(BFHIP_ENOMEM, "out of device memory for coefficient set");
    { const int rp = coeff_prep(e, src, n_taps, scale, c.d_H, n_blocks); if (rp != BFHIP_OK) { coeff_release(e, c.d_H, h_bytes); return rp; } }
    if (on_device) { int _r = sync_all(e); if (_r != BFHIP_OK) { coeff_release(e, c.d_H, h_bytes); return _r; } }
    if (!on_device) {
        // host-taps path is synchronous, like convolver_coeffs2cbuf: report NaN/Inf now
        int bad = 0;
        { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
        HIPCHK(hipMemcpy(&bad, e->d_bad, sizeof(int), hipMemcpyDeviceToHost));
        if (bad) {
            HIPCHK(hipMemset(e->d_bad, 0, sizeof(int)));
            coeff_release(e, c.d_H, h_bytes);
            return fail(BFHIP_EINVAL, "NaN or Inf value among coefficients.");
        }
    }
    e->coeffs.push_back(c);
    return (int)e->coeffs.size() - 1;
}

int bfhip_engine_reserve_coeffs(bfhip_engine *e, double total_bytes) {
    if (!e || total_bytes < 0) return fail(BFHIP_EINVAL, "reserve_coeffs: bad argument");
    if (!e->coeff_arena || total_bytes == 0) return BFHIP_OK;
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    // every set is rounded up to 64 KiB: leave room for that
    const size_t want = ((size_t)(total_bytes * 1.05) + ((size_t)1 << 20) + 65535) & ~(size_t)65535;
    if (!e->slabs.empty() && e->slabs.back().cap - e->slabs.back().used >= want) return BFHIP_OK;
    bfhip_engine::Slab sl;
    if (dev_alloc(&sl.base, want) != hipSuccess) {
        (void)hipGetLastError();
        return fail(BFHIP_ENOMEM, "out of device memory reserving %.0f bytes of coefficient memory", total_bytes);
    }
    sl.cap = want; sl.used = 0;
    e->slabs.push_back(sl);
    return BFHIP_OK;
}

int bfhip_engine_add_coeff(bfhip_engine *e, const void *taps, int n_taps, double scale, int n_blocks) {
    return add_coeff_common(e, taps, false, n_taps, scale, n_blocks);
}

int bfhip_engine_add_coeff_dev(bfhip_engine *e, const void *taps_dev, int n_taps, double scale, int n_blocks) {
    return add_coeff_common(e, taps_dev, true, n_taps, scale, n_blocks);
}

// one cbuf (2L reals, the reference's "4 re / 4 im" layout) -> packed partition `block` of set c
static int upload_processed_block(bfhip_engine *e, Coeff &c, int block, const void *cbuf) {
    const size_t n = (size_t)2 * e->L;
    for (size_t i = 0; i < n; i++) {           // convolver_verify_cbuf (fftw_convolver.c:598-622)
        const double v = e->rs == 4 ? (double)((const float *)cbuf)[i] : ((const double *)cbuf)[i];
        if (!std::isfinite(v)) return fail(BFHIP_EINVAL, "NaN or Inf value among coefficients.");
    }
    const size_t bytes = n * e->rs;
    { const int rt = taps_reserve(e, bytes); if (rt != BFHIP_OK) return rt; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }      // d_taps is reused; nothing may still read H
    HIPCHK(hipMemcpy(e->b_taps.p, cbuf, bytes, hipMemcpyHostToDevice));
    void *H = (unsigned char *)c.d_H + (size_t)block * e->L * e->csize();
    { int _r = coeff_reorder(e, e->b_taps.p, H, 1, true); if (_r != BFHIP_OK) return _r; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    return e->rs == 4 ? stream_refresh_block<float>(e, c.d_H, block) : stream_refresh_block<double>(e, c.d_H, block);
}

extern "C++" {
BFHIP_HOST_NS {
// a lazily registered set goes to the device (the first time an active filter refers to it)
int coeff_make_resident(bfhip_engine *e, int ci) {
    Coeff &c = e->coeffs[ci];
    if (c.d_H != nullptr) return BFHIP_OK;
    if ((int)c.watch_src.size() != c.n_blocks) return fail(BFHIP_ESTATE, "coefficient set %d has no data", ci);
    const size_t h_bytes = (size_t)c.n_blocks * e->L * e->csize();
    if ((c.d_H = coeff_alloc(e, h_bytes)) == nullptr)
        return fail(BFHIP_ENOMEM, "out of device memory for coefficient set");
    for (int b = 0; b < c.n_blocks; b++) {
        // generation first, data second: a notice that arrives in between is seen by the next poll
        const uint64_t gen = c.watched ? bfhip_dirty_generation(c.watch_src[b]) : 0;
        const int r = upload_processed_block(e, c, b, c.watch_src[b]);
        if (r != BFHIP_OK) { coeff_release(e, c.d_H, h_bytes); c.d_H = nullptr; return r; }
        if (c.watched) c.watch_gen[b] = gen;
    }
    return BFHIP_OK;
}
}  // namespace bfhip_host
}  // extern "C++"

int bfhip_engine_add_coeff_processed_blocks(bfhip_engine *e, void *const cbufs[], int n_blocks, int flags) {
    if (!e || !cbufs || n_blocks < 1) return fail(BFHIP_EINVAL, "add_coeff_processed_blocks: bad argument");
    if (n_blocks > e->N) return fail(BFHIP_EINVAL, "coefficient set has %d blocks, engine has %d", n_blocks, e->N);
    for (int b = 0; b < n_blocks; b++) if (!cbufs[b]) return fail(BFHIP_EINVAL, "add_coeff_processed_blocks: block %d is NULL", b);
    if (flags & ~(BFHIP_COEFF_WATCH | BFHIP_COEFF_LAZY)) return fail(BFHIP_EINVAL, "add_coeff_processed_blocks: unknown flag");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    const bool watch = (flags & BFHIP_COEFF_WATCH) != 0, lazy = (flags & BFHIP_COEFF_LAZY) != 0;
    Coeff c;
    c.n_blocks = n_blocks;
    c.lazy = lazy; c.watched = watch;
    if (lazy) {
        // nothing goes to the device yet: the host blocks (which the host keeps for its whole life,
        // bfconf->coeffs_data) are loaded when a filter this engine runs first refers to the set
        for (int b = 0; b < n_blocks; b++) { c.watch_src.push_back(cbufs[b]); c.watch_gen.push_back(0); }
        if (watch) e->any_watched = true;
        e->coeffs.push_back(c);
        if (e->finalized) e->plan_dirty = true;
        return (int)e->coeffs.size() - 1;
    }
    HIPCHK(hipSetDevice(e->device));
    const size_t h_bytes = (size_t)n_blocks * e->L * e->csize();
    if ((c.d_H = coeff_alloc(e, h_bytes)) == nullptr)
        return fail(BFHIP_ENOMEM, "out of device memory for coefficient set");
    for (int b = 0; b < n_blocks; b++) {
        // generation first, data second: a notice that arrives in between is seen by the next poll
        const uint64_t gen = watch ? bfhip_dirty_generation(cbufs[b]) : 0;
        const int r = upload_processed_block(e, c, b, cbufs[b]);
        if (r != BFHIP_OK) { coeff_release(e, c.d_H, h_bytes); return r; }
        if (watch) { c.watch_src.push_back(cbufs[b]); c.watch_gen.push_back(gen); }
    }
    if (watch) {
        e->any_watched = true;
        // (watch_seq stays where it is: a notice older than this call costs one extra scan)
    }
    e->coeffs.push_back(c);
    return (int)e->coeffs.size() - 1;
}

int bfhip_engine_coeff_is_resident(const bfhip_engine *e, int coeff) {
    if (!e || coeff < 0 || coeff >= (int)e->coeffs.size()) return 0;
    return e->coeffs[coeff].d_H != nullptr ? 1 : 0;
}

int bfhip_engine_refresh_coeff_processed(bfhip_engine *e, int coeff, int block, const void *cbuf) {
    if (!e || coeff < 0 || coeff >= (int)e->coeffs.size() || block < 0 || block >= e->coeffs[coeff].n_blocks)
        return fail(BFHIP_EINVAL, "refresh_coeff_processed: bad argument");
    Coeff &c = e->coeffs[coeff];
    if (cbuf == nullptr) {
        if (c.watch_src.empty()) return fail(BFHIP_EINVAL, "refresh_coeff_processed: no host buffer known for this set");
        cbuf = c.watch_src[block];
    }
    if (c.d_H == nullptr) {
        // registered lazily and not loaded yet: its host block is read when the set is first needed
        if (cbuf != c.watch_src[block]) return fail(BFHIP_ESTATE, "refresh_coeff_processed: set %d is not on the device yet", coeff);
        return BFHIP_OK;
    }
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    return upload_processed_block(e, c, block, cbuf);
}

int bfhip_engine_poll_coeff_changes(bfhip_engine *e) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    return poll_coeff_changes(e);
}

int bfhip_engine_add_coeff_processed(bfhip_engine *e, const void *cbufs, int n_blocks) {
    if (!e || !cbufs || n_blocks < 1) return fail(BFHIP_EINVAL, "add_coeff_processed: bad argument");
    if (n_blocks > e->N) return fail(BFHIP_EINVAL, "coefficient set has %d blocks, engine has %d", n_blocks, e->N);
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    const size_t n = (size_t)n_blocks * 2 * e->L;
    // convolver_verify_cbuf (fftw_convolver.c:598-622) as load_coeff applies it (bfconf.c:1958)
    for (size_t i = 0; i < n; i++) {
        const double v = e->rs == 4 ? (double)((const float *)cbufs)[i] : ((const double *)cbufs)[i];
        if (!std::isfinite(v)) return fail(BFHIP_EINVAL, "NaN or Inf value among coefficients.");
    }
    const size_t bytes = n * e->rs;
    { const int rt = taps_reserve(e, bytes); if (rt != BFHIP_OK) return rt; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    HIPCHK(hipMemcpy(e->b_taps.p, cbufs, bytes, hipMemcpyHostToDevice));
    Coeff c;
    c.n_blocks = n_blocks;
    if ((c.d_H = coeff_alloc(e, (size_t)n_blocks * e->L * e->csize())) == nullptr)
        return fail(BFHIP_ENOMEM, "out of device memory for coefficient set");
    { int _r = coeff_reorder(e, e->b_taps.p, c.d_H, n_blocks, true); if (_r != BFHIP_OK) return _r; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    e->coeffs.push_back(c);
    return (int)e->coeffs.size() - 1;
}

int bfhip_engine_read_coeff_processed(bfhip_engine *e, int coeff, void *cbufs) {
    if (!e || !cbufs || coeff < 0 || coeff >= (int)e->coeffs.size()) return fail(BFHIP_EINVAL, "read_coeff_processed: bad argument");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { const int rr = coeff_make_resident(e, coeff); if (rr != BFHIP_OK) return rr; }
    const int nb = e->coeffs[coeff].n_blocks;
    const size_t bytes = (size_t)nb * 2 * e->L * e->rs;
    { const int rt = taps_reserve(e, bytes); if (rt != BFHIP_OK) return rt; }
    { int _r = coeff_reorder(e, e->b_taps.p, e->coeffs[coeff].d_H, nb, false); if (_r != BFHIP_OK) return _r; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    HIPCHK(hipMemcpy(cbufs, e->b_taps.p, bytes, hipMemcpyDeviceToHost));
    return nb;
}

int bfhip_engine_update_coeff_block(bfhip_engine *e, int coeff, int block, const void *taps) {
    if (!e || coeff < 0 || coeff >= (int)e->coeffs.size() || block < 0 ||
        block >= e->coeffs[coeff].n_blocks || !taps)
        return fail(BFHIP_EINVAL, "update_coeff_block: bad argument");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { const int rr = coeff_make_resident(e, coeff); if (rr != BFHIP_OK) return rr; }
    const size_t bytes = (size_t)e->L * e->rs;
    { const int rt = taps_reserve(e, bytes); if (rt != BFHIP_OK) return rt; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    HIPCHK(hipMemcpy(e->b_taps.p, taps, bytes, hipMemcpyHostToDevice));
    void *H = (unsigned char *)e->coeffs[coeff].d_H + (size_t)block * e->L * e->csize();
    { const int rp = coeff_prep(e, e->b_taps.p, e->L, 1.0, H, 1); if (rp != BFHIP_OK) return rp; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    return e->rs == 4 ? stream_refresh_block<float>(e, e->coeffs[coeff].d_H, block)
                      : stream_refresh_block<double>(e, e->coeffs[coeff].d_H, block);
}

// ---- rewrite of a whole resident set without a host wait (coeff_async.h; bfhip_nupc_update_coeff_async)

// scratch the asynchronous rewrite needs, allocated now instead of lazily: the big-FFT buffers for a
// whole set's partitions.  (The rewrite reads its taps straight from the caller's device buffer, so it
// needs no d_taps.)  May wait and allocate: not for the audio path.
int bfhip_internal_engine_reserve_update(bfhip_engine *e) {
    if (!e || !e->finalized) return fail(BFHIP_ESTATE, "reserve_update: engine not finalized");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    if (e->big) { int rr = big_reserve(e, (size_t)e->N); if (rr != BFHIP_OK) return rr; }
    return BFHIP_OK;
}

// Partitions [0, n_blocks) of resident set `coeff` from n_taps reals in device memory (zero-padded),
// prepared by K7 on the engine's own stream, in order with its blocks: no host wait, no allocation,
// no blocking copy.  The set must not be read by a block handed in after this call until a filter is
// pointed at it again (the caller's state rules see to that); the stream-ordered copy and the long-window
// layout forget that they hold it, as update_coeff_block makes them when no copy is in force, so the next
// plan build lays it out from the new data.  Behind the preparation the engine's non-finite flag is
// copied to *bad_host (pinned) and cleared; the caller records its own event behind this call.
int bfhip_internal_engine_update_coeff_dev_async(bfhip_engine *e, int coeff, const void *taps_dev, int n_taps,
                                                 int n_blocks, int *bad_host) {
    if (!e || coeff < 0 || coeff >= (int)e->coeffs.size() || !taps_dev || n_taps < 0 || n_blocks < 1 ||
        n_blocks > e->coeffs[coeff].n_blocks || !bad_host)
        return fail(BFHIP_EINVAL, "update_coeff_dev_async: bad argument");
    if (!e->finalized) return fail(BFHIP_ESTATE, "update_coeff_dev_async: engine not finalized");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    Coeff &c = e->coeffs[coeff];
    if (c.d_H == nullptr) return fail(BFHIP_ESTATE, "update_coeff_dev_async: set %d is not on the device", coeff);
    if (e->big && (size_t)n_blocks > e->big_cap)
        return fail(BFHIP_ESTATE, "update_coeff_dev_async: no scratch reserved for %d partitions", n_blocks);
    HIPCHK(hipSetDevice(e->device));
    if ((long)n_taps > (long)n_blocks * e->L) n_taps = n_blocks * e->L;
    HIPCHK(hipMemsetAsync(e->d_bad, 0, sizeof(int), e->stream));
    // (the scratch above 8192 points was checked above: nothing is reserved, nothing waits)
    { const int rp = coeff_prep(e, taps_dev, n_taps, 1.0, c.d_H, n_blocks); if (rp != BFHIP_OK) return rp; }
    HIPCHK(hipMemcpyAsync(bad_host, e->d_bad, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemsetAsync(e->d_bad, 0, sizeof(int), e->stream));
    // the layouts compare sets by pointer, which an in-place rewrite does not change
    bool held = false;
    for (auto &k : e->stream_keys)
        for (int j = 0; j < OG; j++) if (k[j] == c.d_H) { k[j] = STREAM_KEY_STALE; held = true; }
    for (auto &k : e->lkeys)
        for (int j = 0; j < OG; j++) if (k[j] == c.d_H) { k[j] = STREAM_KEY_STALE; held = true; }
    // a layout in force that holds the set: build the plan again before the next block reads it
    if (held && (e->hstream.base != nullptr || e->lw_active)) e->plan_dirty = true;
    return BFHIP_OK;
}

int bfhip_engine_add_filter(bfhip_engine *e,
                            int n_in_ch, const int in_ch[], const double in_scale[],
                            int n_in_f, const int in_f[], const double in_fscale[],
                            int n_out_ch, const int out_ch[], const double out_scale[],
                            int coeff, int delayblocks, int crossfade) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    if (e->finalized) return fail(BFHIP_ESTATE, "add_filter after finalize");
    if (n_in_ch < 0 || n_in_f < 0 || n_out_ch < 0) return fail(BFHIP_EINVAL, "add_filter: negative count");
    if ((n_in_ch > 0 && (!in_ch || !in_scale)) || (n_in_f > 0 && (!in_f || !in_fscale)) ||
        (n_out_ch > 0 && (!out_ch || !out_scale)))
        return fail(BFHIP_EINVAL, "add_filter: null array");
    if (coeff < -1) return fail(BFHIP_EINVAL, "add_filter: coeff %d (-1 = none)", coeff);
    Filter f;
    for (int i = 0; i < n_in_ch; i++) {
        if (in_ch[i] < 0 || in_ch[i] >= e->n_ch[0]) return fail(BFHIP_EINVAL, "add_filter: input channel %d", in_ch[i]);
        f.in_ch.push_back(in_ch[i]); f.in_scale.push_back(in_scale[i]);
    }
    for (int i = 0; i < n_in_f; i++) {
        if (in_f[i] < 0 || in_f[i] >= (int)e->filters.size()) return fail(BFHIP_EINVAL, "add_filter: from_filter %d not defined yet", in_f[i]);
        f.in_f.push_back(in_f[i]); f.in_fscale.push_back(in_fscale[i]);
    }
    for (int i = 0; i < n_out_ch; i++) {
        if (out_ch[i] < 0 || out_ch[i] >= e->n_ch[1]) return fail(BFHIP_EINVAL, "add_filter: output channel %d", out_ch[i]);
        f.out_ch.push_back(out_ch[i]); f.out_scale.push_back(out_scale[i]);
    }
    if (coeff >= (int)e->coeffs.size()) return fail(BFHIP_EINVAL, "add_filter: coeff %d not loaded", coeff);
    f.coeff = coeff; f.delayblocks = delayblocks; f.crossfade = crossfade; f.prevcoeff = coeff;
    e->filters.push_back(f);
    return (int)e->filters.size() - 1;
}

int bfhip_engine_set_filter_active(bfhip_engine *e, int filter, int active) {
    if (!e || filter < 0 || filter >= (int)e->filters.size()) return fail(BFHIP_EINVAL, "set_filter_active: bad argument");
    if (e->finalized) return fail(BFHIP_ESTATE, "set_filter_active after finalize");
    e->filters[filter].active = active != 0;
    return BFHIP_OK;
}

int bfhip_engine_set_filter_name(bfhip_engine *e, int filter, int name) {
    if (!e || filter < 0 || filter >= (int)e->filters.size() || name < 0) return fail(BFHIP_EINVAL, "set_filter_name: bad argument");
    if (e->finalized) return fail(BFHIP_ESTATE, "set_filter_name after finalize");
    for (size_t i = 0; i < e->filters.size(); i++)
        if ((int)i != filter && e->filters[i].name == name) return fail(BFHIP_EINVAL, "set_filter_name: %d is taken", name);
    e->filters[filter].name = name;
    return BFHIP_OK;
}

int bfhip_engine_set_output_active(bfhip_engine *e, int ch, int active) {
    if (!e || ch < 0 || ch >= e->n_ch[1]) return fail(BFHIP_EINVAL, "set_output_active: bad argument");
    if (e->finalized) return fail(BFHIP_ESTATE, "set_output_active after finalize");
    e->out_active_set.resize(e->n_ch[1], -1);
    e->out_active_set[ch] = active ? 1 : 0;
    return BFHIP_OK;
}

int bfhip_engine_output_is_active(const bfhip_engine *e, int ch) {
    if (!e || ch < 0 || ch >= e->n_ch[1]) return 0;
    return e->out_active.empty() ? 1 : (e->out_active[ch] ? 1 : 0);
}

static int finalize_impl(bfhip_engine *e);

int bfhip_engine_finalize(bfhip_engine *e) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    if (e->finalized) return BFHIP_OK;
    // a finalize that failed half way (out of device memory, a bad coefficient set) leaves partial
    // state behind that only bfhip_engine_destroy cleans up: it is not retried
    if (e->finalize_failed) return fail(BFHIP_ESTATE, "finalize failed before: destroy this engine");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    const int r = finalize_impl(e);
    if (r != BFHIP_OK) { e->finalize_failed = true; e->finalized = false; }
    return r;
}

// Which outputs does this engine convert and write?  (bfconf.c:2893-2931: every output is mixed
// inside one filter process, connected filters stay in one process -- the same rules, checked.)
static int resolve_shard(bfhip_engine *e) {
    const int O = e->n_ch[1], F = (int)e->filters.size();
    e->out_active_set.resize(O, -1);
    std::vector<char> fed(O, 0), fed_here(O, 0), fed_else(O, 0);
    for (int fi = 0; fi < F; fi++) {
        const Filter &f = e->filters[fi];
        for (int o : f.out_ch) { fed[o] = 1; (f.active ? fed_here : fed_else)[o] = 1; }
        for (int g : f.in_f)
            if (e->filters[g].active != f.active)
                return fail(BFHIP_EINVAL, "filters %d and %d are connected: they must be run by the same engine", g, fi);
    }
    e->out_active.assign(O, 1);
    e->sharded = false;
    for (int o = 0; o < O; o++) {
        if (fed_here[o] && fed_else[o]) return fail(BFHIP_EINVAL, "output %d is mixed from filters of two engines", o);
        const bool derived = fed[o] ? fed_here[o] != 0 : true;
        const bool act = e->out_active_set[o] < 0 ? derived : e->out_active_set[o] != 0;
        if (!act && fed_here[o]) return fail(BFHIP_EINVAL, "output %d is fed by this engine's filters but marked inactive", o);
        if (act && fed_else[o]) return fail(BFHIP_EINVAL, "output %d is fed by another engine's filters but marked active", o);
        e->out_active[o] = act ? 1 : 0;
        if (!act) e->sharded = true;
    }
    // virtual outputs that share a physical channel are mixed in the time domain by ONE engine
    for (int o = 0; o < O; o++)
        for (int q = o + 1; q < O; q++)
            if (e->ch.v2p[1][o] == e->ch.v2p[1][q] && e->out_active[o] != e->out_active[q])
                return fail(BFHIP_EINVAL, "outputs %d and %d share a physical channel: one engine must own both", o, q);
    return BFHIP_OK;
}

// the raw output samples a sharded engine owns, as byte runs per frame (neighbouring channels of an
// interleaved frame merge into one run)
static void build_owned_runs(bfhip_engine *e) {
    e->owned_runs.clear();
    if (!e->sharded) return;
    std::vector<bfhip_engine::OwnedRun> runs;
    std::vector<char> seen(e->ch.n_phys[1], 0);
    for (int o = 0; o < e->n_ch[1]; o++) {
        const int p = e->ch.v2p[1][o];
        if (!e->out_active[o] || seen[p]) continue;
        seen[p] = 1;
        const bfhip_format &f = e->fmt[1][p];
        runs.push_back({(size_t)f.byte_offset, (size_t)f.bytes, (size_t)f.sample_spacing * f.bytes});
    }
    std::sort(runs.begin(), runs.end(), [](const bfhip_engine::OwnedRun &a, const bfhip_engine::OwnedRun &b) { return a.offset < b.offset; });
    for (auto &r : runs) {
        if (!e->owned_runs.empty()) {
            auto &b = e->owned_runs.back();
            if (b.stride == r.stride && b.offset + b.len == r.offset && b.len + r.len <= b.stride) { b.len += r.len; continue; }
        }
        e->owned_runs.push_back(r);
    }
}

// dst <- src for the samples this engine owns; everything else in dst belongs to other engines
static void copy_owned(const bfhip_engine *e, void *dst, const void *src) {
    if (!e->sharded) { memcpy(dst, src, e->raw_bytes[1]); return; }
    for (auto &r : e->owned_runs) {
        unsigned char *d = (unsigned char *)dst + r.offset;
        const unsigned char *s = (const unsigned char *)src + r.offset;
        if (r.len == r.stride) { memcpy(d, s, r.len * (size_t)e->L); continue; }
        for (int n = 0; n < e->L; n++, d += r.stride, s += r.stride) memcpy(d, s, r.len);
    }
}

static void copy_owned_overflow(const bfhip_engine *e, bfhip_overflow dst[], const void *src) {
    const DevOverflow *s = (const DevOverflow *)src;
    for (int o = 0; o < e->n_ch[1]; o++)
        if (!e->sharded || e->out_active[o]) memcpy(&dst[o], &s[o], sizeof(DevOverflow));
}

// the block schedule (BFHIP_MODE_*), decided once at finalize
static int choose_mode(const bfhip_engine *e) {
    // Run the FFT kernels of neighbouring blocks beside the MAC?  Pays when the MAC is short
    // (small crossbars: config B 84 -> 58 us per block) and costs when it streams for a
    // millisecond (config C 1.40 -> 1.77 ms): decide from the coefficient bytes per block.
    double bytes = 0;
    for (auto &f : e->filters) {
        if (f.coeff < 0) continue;
        const int d = clamp_delay(e, f.delayblocks);
        bytes += (double)cblocks_of(e, f.coeff, d) * (double)e->L * (double)e->csize() * (double)std::max<size_t>(1, f.out_ch.size());
    }
    // ... and only while the transforms leave most CUs to the MAC: with hundreds of channels the
    // FFT workgroups fill the chip themselves (config D, 256 + 256: 0.178 ms piped, 0.168 plain)
    bool pipe = bytes / 6.4e12 < 100e-6 && e->n_ch[0] + e->n_ch[1] <= 128;
    // (Beside a long MAC the transforms only get in the way: a MAC workgroup takes 320 of a SIMD's
    // 512 registers per lane, no transform workgroup fits on the same CU, and on a side stream
    // they either wait for the MAC's tail or push its workgroups together on fewer CUs --
    // config C 1.40 -> 1.74 ms.  A 256-thread variant that did fit next to round 1's MAC hid
    // them but slowed the MAC by as much)
    if (e->overlap_mode >= 0) pipe = e->overlap_mode != 0;
    // (the environment only moves the AUTOMATIC choice: an explicit bfhip_engine_set_overlap wins --
    // the non-uniform convolver depends on its segment engines running strictly in order)
    if (const char *env = e->overlap_mode < 0 ? getenv("BFHIP_OVERLAP") : nullptr) pipe = atoi(env) != 0;
    if (!e->ch.one_to_one() || e->big) pipe = false;   // one job table per side; one FFT scratch
    // the fused [K3 | K1] launch of deferred output and ping-pong needs the plain 1:1 raw path
    const bool plain = e->wave && !e->big && e->ch.configured_plain();
    // one stream and a MAC that fills the chip for a long time: deferred output.  (An explicit
    // bfhip_engine_set_overlap(e, 0) -- "strictly in order" -- beats the environment.)
    bool defer = !pipe && plain && e->overlap_mode != 0;
    if (const char *env = getenv("BFHIP_DEFER")) defer = defer && atoi(env) != 0;
    if (e->pairs) pipe = false;                // block pairs run on the one main stream
    // small MACs with the wave FFT: the two-stream ping-pong instead of three streams
    if (pipe) return plain ? BFHIP_MODE_PINGPONG : BFHIP_MODE_PIPELINED;
    return defer ? BFHIP_MODE_DEFERRED : BFHIP_MODE_SEQUENTIAL;
}

static int finalize_impl(bfhip_engine *e) {
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    { const int rsh = resolve_shard(e); if (rsh != BFHIP_OK) return rsh; }
    HIPCHK(hipSetDevice(e->device));
    const size_t L = e->L;
    const size_t prev_b = (size_t)e->n_ch[0] * L * e->rs;
    e->mode = choose_mode(e);
    // (a pair needs the spare ring slot too: block t + 1 is transformed before the MAC reads block t - N + 1)
    e->R = (e->mode == BFHIP_MODE_PIPELINED || e->mode == BFHIP_MODE_PINGPONG || e->pairs) ? e->N + 1 : e->N;
    {
        // the shared rings are R deep, the private ones N: the counter wraps by a multiple of both
        const unsigned long long period = e->R == e->N ? (unsigned long long)e->N : (unsigned long long)e->N * e->R;
        if (period <= (1ull << 30)) {
            e->wrap_by = (unsigned int)((0x7fffffffull / period) * period);
            e->wrap_at = e->wrap_by + 2u * (unsigned int)e->R;           // t - p - delay stays >= 0
        }
        if (const char *env = getenv("BFHIP_TEST_WRAP_PERIODS")) {       // tests: wrap after a few ring periods
            e->wrap_by = (unsigned int)(std::max(1, atoi(env)) * period);
            // (... and BFHIP_TEST_WRAP_SKEW: by a few blocks more, i.e. NOT a multiple of the depths --
            // what a wrap at 2^32 is for such depths; the tests want to see that go wrong)
            if (const char *skew = getenv("BFHIP_TEST_WRAP_SKEW")) e->wrap_by += (unsigned int)atoi(skew);
            e->wrap_at = e->wrap_by + 2u * (unsigned int)e->R;
        }
    }
    // the MAC addresses a ring / a coefficient set with 32-bit byte offsets from its base
    if ((double)(e->N + 1) * (double)L * (double)e->csize() >= 4294967296.0)
        return fail(BFHIP_EINVAL, "%d partitions of %d taps: a coefficient set would exceed 4 GiB", e->N, e->L);
    const size_t ring_b = (size_t)e->n_ch[0] * e->R * L * e->csize();
    if (dev_alloc(&e->d_prev, prev_b) != hipSuccess || dev_alloc(&e->d_ring, ring_b) != hipSuccess)
        return fail(BFHIP_ENOMEM, "out of device memory for the spectrum rings");
    HIPCHK(hipMemset(e->d_prev, 0, prev_b));       // bfrun.c:1388: everything starts zeroed
    HIPCHK(hipMemset(e->d_ring, 0, ring_b));
    if (e->powersave > 0.0) {
        if (e->big) {
            HIPCHK(dev_alloc((void **)&e->d_ps_acc, 2 * e->n_ch[0] * sizeof(unsigned long long)));
            HIPCHK(hipMemset(e->d_ps_acc, 0, 2 * e->n_ch[0] * sizeof(unsigned long long)));
        }
        {
            std::vector<int> ones((size_t)e->n_ch[0] * e->R, 1);     // the zeroed rings are silence
            std::vector<double> sc(e->n_ch[0]);
            for (int c = 0; c < e->n_ch[0]; c++) sc[c] = e->fmt[0][e->ch.v2p[0][c]].scale;
            HIPCHK(dev_alloc((void **)&e->d_ps_flags, ones.size() * sizeof(int)));
            HIPCHK(hipMemcpy(e->d_ps_flags, ones.data(), ones.size() * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(dev_alloc((void **)&e->d_ps_live, e->n_ch[0] * sizeof(int)));
            HIPCHK(hipMemset(e->d_ps_live, 0, e->n_ch[0] * sizeof(int)));
            HIPCHK(dev_alloc((void **)&e->d_ps_scale, sc.size() * sizeof(double)));
            HIPCHK(hipMemcpy(e->d_ps_scale, sc.data(), sc.size() * sizeof(double), hipMemcpyHostToDevice));
        }
    }
    for (int io = 0; io < 2; io++) HIPCHK(dev_alloc((void **)&e->d_fmt[io], e->n_ch[io] * sizeof(DevFormat)));
    int r = channels_setup(e);
    if (r != BFHIP_OK) return r;
    HIPCHK(dev_alloc((void **)&e->d_over, e->n_ch[1] * sizeof(DevOverflow)));
    HIPCHK(dev_alloc((void **)&e->d_status, sizeof(int)));
    HIPCHK(hipMemset(e->d_status, 0, sizeof(int)));
    e->raw_bytes[0] = raw_extent(e->fmt[0], e->ch.n_phys[0], e->L);
    e->raw_bytes[1] = raw_extent(e->fmt[1], e->ch.n_phys[1], e->L);
    build_owned_runs(e);
    HIPCHK(dev_alloc((void **)&e->d_rawin, e->raw_bytes[0] + 16));       // +16: staged in 16-byte words
    HIPCHK(dev_alloc((void **)&e->d_rawout, e->raw_bytes[1] + 16));
    HIPCHK(hipMemset(e->d_rawout, 0, e->raw_bytes[1]));
    // classify filters: who owns a private ring, who must materialise its output
    {
        const int F = (int)e->filters.size();
        e->level.assign(F, 0); e->owner_index.assign(F, -1); e->y_index.assign(F, -1);
        e->sink_index.assign(F, -1); e->fade_index.assign(F, -1); e->is_source.assign(F, 0);
        e->promoted.assign(F, nullptr);
        e->n_owners = e->n_y = e->n_sinks = e->n_fadeable = 0;
        int maxlevel = 0;
        for (int fi = 0; fi < F; fi++) {
            const Filter &f = e->filters[fi];
            for (int g : f.in_f) { e->is_source[g] = 1; e->level[fi] = std::max(e->level[fi], e->level[g] + 1); }
            maxlevel = std::max(maxlevel, e->level[fi]);
            if (!f.active) continue;               // run by another engine: no ring, no buffers here
            if (f.in_ch.size() != 1 || !f.in_f.empty()) e->owner_index[fi] = e->n_owners++;
            if (!f.in_f.empty()) e->sink_index[fi] = e->n_sinks++;
            if (f.crossfade) e->fade_index[fi] = e->n_fadeable++;
        }
        for (int fi = 0; fi < F; fi++)
            if (e->filters[fi].active && (e->is_source[fi] || e->filters[fi].crossfade)) e->y_index[fi] = e->n_y++;
        e->n_levels = maxlevel + 1;
        auto zalloc = [&](void **p, size_t bytes) -> int {
            if (bytes == 0) return BFHIP_OK;
            if (dev_alloc(p, bytes) != hipSuccess) return fail(BFHIP_ENOMEM, "out of device memory (%zu bytes)", bytes);
            HIPCHK(hipMemset(*p, 0, bytes));
            return BFHIP_OK;
        };
        if ((r = zalloc(&e->d_fring, (size_t)e->n_owners * e->N * L * e->csize())) != BFHIP_OK) return r;
        if ((r = zalloc(&e->d_Y, (size_t)e->n_y * L * e->csize())) != BFHIP_OK) return r;
        if ((r = zalloc(&e->d_Yold, (size_t)e->n_fadeable * L * e->csize())) != BFHIP_OK) return r;
        if ((r = zalloc(&e->d_evalprev, (size_t)e->n_sinks * L * e->rs)) != BFHIP_OK) return r;
    }
    if ((r = channels_upload_dither(e)) != BFHIP_OK) return r;
    if (e->mode == BFHIP_MODE_PIPELINED || e->mode == BFHIP_MODE_PINGPONG) {
        HIPCHK(hipStreamCreateWithFlags(&e->s_in, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&e->s_out, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            HIPCHK(hipEventCreateWithFlags(&e->ev_in[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&e->ev_mac[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&e->ev_out[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&e->ev_io[i], hipEventDisableTiming));
        }
        for (int i = 0; i < 3; i++) HIPCHK(hipEventCreateWithFlags(&e->ev_mac3[i], hipEventDisableTiming));
    }
    e->ls = e->stream;
    e->finalized = true;
    r = bfhip_engine_reset_overflow(e);
    if (r != BFHIP_OK) return r;
    // coefficient sets loaded from device memory are checked here
    int bad = 0;
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    HIPCHK(hipMemcpy(&bad, e->d_bad, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return fail(BFHIP_EINVAL, "NaN or Inf value among coefficients.");
    {
        // long-window plan: structure here, the per-plan conditions in build_long_layout.  The size test
        // is on every set registered -- the whole configuration's, not a shard's share: a shard
        // engine takes the long plan exactly when the one-process engine does (plan_long_whole, plan.hip)
        int want = -1;
        if (const char *env = getenv("BFHIP_LONG_WINDOW")) want = atoi(env) != 0 ? 1 : 0;
        double vol = 0;
        for (auto &c : e->coeffs) vol += (double)c.n_blocks * (double)L * (double)e->csize();
        // (what the configuration fixes for good -- powersave, dither, wide / shared / sub-sample outputs --
        // is settled here: such an engine never runs the long transforms)
        e->lw_struct = want != 0 && e->rs == 4 && e->L == 8192 && e->wave && !e->big && e->N >= 8 && !e->pairs &&
                       e->powersave <= 0.0 && e->ch.k3_writes_raw() && (want == 1 || vol >= 1073741824.0);
        if (e->lw_struct) {
            const size_t hist_b = (size_t)e->n_ch[0] * e->R * L * sizeof(float);
            const size_t lring_b = (size_t)e->n_ch[0] * e->R * 2 * L * sizeof(c2<float>);
            const std::vector<unsigned char> tw = make_twiddle_table(LW_LOG2, 4, fft_threads<float>(LW_LOG2), true);
            if (dev_alloc(&e->d_hist, hist_b) != hipSuccess || dev_alloc(&e->d_lring, lring_b) != hipSuccess ||
                dev_alloc(&e->d_tw14, tw.size()) != hipSuccess)
                return fail(BFHIP_ENOMEM, "out of device memory for the long-window rings");
            HIPCHK(hipMemset(e->d_hist, 0, hist_b));
            HIPCHK(hipMemset(e->d_lring, 0, lring_b));
            HIPCHK(hipMemcpy(e->d_tw14, tw.data(), tw.size(), hipMemcpyHostToDevice));
        }
    }
    return build_plan(e);
}

// Exact history semantics for run-time changes (SURVEY 7 "hard parts"): the reference scales
// and delays a block when it ENTERS the filter's ring, so a change must not touch the blocks
// already in it.  A filter that shares its input's ring gets its own ring at that moment.
static int promote_filter(bfhip_engine *e, int fi) {
    if (!e->finalized || e->owner_index[fi] >= 0 || e->promoted[fi]) return BFHIP_OK;
    const Filter &f = e->filters[fi];
    if (!f.active) {
        // run by another engine, which gives it its private ring there; here only the plan's shape follows
        if (f.in_ch.size() == 1 && f.in_f.empty()) { e->promoted[fi] = PROMOTED_ELSEWHERE; e->plan_dirty = true; }
        return BFHIP_OK;
    }
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    const size_t bytes = (size_t)e->N * e->L * e->csize();
    void *ring = nullptr;
    if (dev_alloc(&ring, bytes) != hipSuccess) return fail(BFHIP_ENOMEM, "out of device memory for a private ring");
    HIPCHK(hipMemsetAsync(ring, 0, bytes, e->stream));
    const int ch = f.in_ch[0];
    const int delay = clamp_delay(e, f.delayblocks);
    const double sc = f.in_scale[0] * e->fmt[0][e->ch.v2p[0][ch]].scale;
    const int n_valid = (int)std::min<unsigned long long>(e->blocks_done, (unsigned long long)e->N);
    if (n_valid > 0) {
        const unsigned char *src = (const unsigned char *)e->d_ring + (size_t)ch * e->R * e->L * e->csize();
        const int r = promote_ring(e, src, ring, delay, sc, n_valid);
        if (r != BFHIP_OK) return r;
    }
    e->promoted[fi] = ring;
    e->plan_dirty = true;
    return BFHIP_OK;
}

int bfhip_engine_set_coeff(bfhip_engine *e, int filter, int coeff) {
    if (!e || filter < 0 || filter >= (int)e->filters.size() || coeff >= (int)e->coeffs.size())
        return fail(BFHIP_EINVAL, "set_coeff: bad argument");
    if (e->filters[filter].coeff != coeff) { e->filters[filter].coeff = coeff; e->plan_dirty = true; }
    return BFHIP_OK;
}

int bfhip_engine_set_delayblocks(bfhip_engine *e, int filter, int blocks) {
    if (!e || filter < 0 || filter >= (int)e->filters.size()) return fail(BFHIP_EINVAL, "set_delayblocks: bad argument");
    if (e->filters[filter].delayblocks != blocks) {
        int r = promote_filter(e, filter);
        if (r != BFHIP_OK) return r;
        e->filters[filter].delayblocks = blocks; e->plan_dirty = true;
    }
    return BFHIP_OK;
}

int bfhip_engine_set_scale(bfhip_engine *e, int filter, int io, int index, double scale) {
    if (!e || filter < 0 || filter >= (int)e->filters.size() || io < 0 || io > 1) return fail(BFHIP_EINVAL, "set_scale: bad argument");
    auto &v = io == 0 ? e->filters[filter].in_scale : e->filters[filter].out_scale;
    if (index < 0 || index >= (int)v.size()) return fail(BFHIP_EINVAL, "set_scale: bad index");
    if (v[index] != scale) {
        if (io == 0) {
            int r = promote_filter(e, filter);
            if (r != BFHIP_OK) return r;
        }
        v[index] = scale; e->plan_dirty = true;
    }
    return BFHIP_OK;
}

int bfhip_engine_set_fscale(bfhip_engine *e, int filter, int index, double scale) {
    if (!e || filter < 0 || filter >= (int)e->filters.size()) return fail(BFHIP_EINVAL, "set_fscale: bad argument");
    auto &v = e->filters[filter].in_fscale;
    if (index < 0 || index >= (int)v.size()) return fail(BFHIP_EINVAL, "set_fscale: bad index");
    if (v[index] != scale) { v[index] = scale; e->plan_dirty = true; }
    return BFHIP_OK;
}

// The phase calls (a host that mixes partial spectra of several engines, bench.py --gpus N) hand
// standard spectra to the caller: an engine driven through them runs the standard plan only, and
// from its first phase call on no longer pays for the long transforms or keeps their memory.
static int lw_drop(bfhip_engine *e) {
    if (!e->lw_struct) return BFHIP_OK;
    { const int r = sync_all(e); if (r != BFHIP_OK) return r; }
    e->lw_struct = e->lw_active = e->la_active = e->far_active = false;
    e->la_epoch++;
    for (void **p : {&e->d_hist, &e->d_lring}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    e->b_lstream.release(); e->b_ahead.release(); e->b_far.release();
    e->lstream = StreamLayout{nullptr, 0, 0, 0};
    e->lkeys.clear();
    for (bool &z : e->zp_long) z = false;
    return BFHIP_OK;
}

int bfhip_engine_inputs_dev(bfhip_engine *e, const void *rawin_dev) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if (!rawin_dev) return fail(BFHIP_EINVAL, "inputs: null buffer");
    if ((r = flush_pending(e)) != BFHIP_OK) return r;
    if ((r = lw_drop(e)) != BFHIP_OK) return r;
    e->ls = e->stream;
    timing_begin(e);
    return block_inputs(e, rawin_dev);
}

int bfhip_engine_mac_dev(bfhip_engine *e, void *z_dev) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if (!z_dev) return fail(BFHIP_EINVAL, "mac: null buffer");
    if ((r = flush_pending(e)) != BFHIP_OK) return r;      // an output owed by bfhip_engine_block_dev goes first
    if ((r = lw_drop(e)) != BFHIP_OK) return r;
    e->ls = e->stream;
    timing_begin(e);
    if ((r = do_levels(e)) != BFHIP_OK) return r;
    if ((r = record_begin(e, T_MAC)) != BFHIP_OK) return r;
    const bool direct = e->n_chunks == 1 && e->n_out_padded == e->n_ch[1];
    if ((r = do_mac(e, direct ? z_dev : e->d_Zp[0], false)) != BFHIP_OK) return r;
    e->zp_last = 0;
    if ((r = record_end(e, T_MAC)) != BFHIP_OK) return r;
    return direct ? BFHIP_OK : sum_chunks(e, e->d_Zp[0], z_dev);
}

int bfhip_engine_outputs_dev(bfhip_engine *e, const void *z_dev, int first, int count, void *rawout_dev) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if ((r = flush_pending(e)) != BFHIP_OK) return r;      // an output owed by bfhip_engine_block_dev goes first
    if ((r = lw_drop(e)) != BFHIP_OK) return r;
    if (first < 0 || count < 0 || first + count > e->n_ch[1]) return fail(BFHIP_EINVAL, "outputs: channel range");
    if (!z_dev || !rawout_dev) return fail(BFHIP_EINVAL, "outputs: null buffer");
    e->ls = e->stream;
    timing_begin(e);
    if ((r = record_begin(e, T_OUT)) != BFHIP_OK) return r;
    if ((r = do_outputs(e, z_dev, 0, 1, first, count, rawout_dev)) != BFHIP_OK) return r;
    return record_end(e, T_OUT);
}

int bfhip_engine_outputs_inputs_dev(bfhip_engine *e, const void *z_dev, int first, int count,
                                    void *rawout_dev, const void *rawin_dev) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if ((r = flush_pending(e)) != BFHIP_OK) return r;      // an output owed by bfhip_engine_block_dev goes first
    if ((r = lw_drop(e)) != BFHIP_OK) return r;
    if (first < 0 || count < 0 || first + count > e->n_ch[1]) return fail(BFHIP_EINVAL, "outputs: channel range");
    if (!z_dev || !rawout_dev || !rawin_dev) return fail(BFHIP_EINVAL, "outputs_inputs: null buffer");
    if (!e->ch.plain() || count == 0 || e->big) {
        // the dither pass follows the inverse transforms: keep the two launches apart
        if ((r = bfhip_engine_outputs_dev(e, z_dev, first, count, rawout_dev)) != BFHIP_OK) return r;
        return bfhip_engine_inputs_dev(e, rawin_dev);
    }
    e->ls = e->stream;
    timing_begin(e);
    if ((r = record_begin(e, T_IN)) != BFHIP_OK) return r;      // the fused launch is timed in the input slot
    if ((r = fused_outputs_inputs(e, z_dev, 0, 1, first, count, rawout_dev, rawin_dev)) != BFHIP_OK) return r;
    return record_end(e, T_IN);
}

int bfhip_engine_advance(bfhip_engine *e) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    advance(e);
    return BFHIP_OK;
}

// PIPELINED: the same passes on three streams
static int block_three_streams(bfhip_engine *e, const void *rawin_dev, void *rawout_dev,
                               hipEvent_t in_ready, hipEvent_t out_done) {
    int r;
    const int buf = (int)(e->blocks_done & 1);
    // K1 on the input stream.  It overwrites the ring slot of block t-R, last read by the MAC
    // of block t-2 (the MAC of t-1 reaches back only N = R-1 blocks).
    e->ls = e->s_in;
    if (e->blocks_done >= 2) HIPCHK(hipStreamWaitEvent(e->s_in, e->ev_mac[buf], 0));
    if (in_ready) HIPCHK(hipStreamWaitEvent(e->s_in, in_ready, 0));
    if ((r = block_inputs(e, rawin_dev)) != BFHIP_OK) return r;
    HIPCHK(hipEventRecord(e->ev_in[buf], e->s_in));

    // per-filter kernels and the crossbar MAC on the main stream; Zp[buf] is free once the
    // output pass of block t-2 has read it
    e->ls = e->stream;
    HIPCHK(hipStreamWaitEvent(e->stream, e->ev_in[buf], 0));
    if (e->blocks_done >= 2) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_out[buf], 0));
    if ((r = block_mac(e, buf)) != BFHIP_OK) return r;
    HIPCHK(hipEventRecord(e->ev_mac[buf], e->stream));

    // K3 (+ dither pass) on the output stream
    e->ls = e->s_out;
    HIPCHK(hipStreamWaitEvent(e->s_out, e->ev_mac[buf], 0));
    if ((r = block_outputs(e, buf, rawout_dev)) != BFHIP_OK) return r;
    HIPCHK(hipEventRecord(e->ev_out[buf], e->s_out));
    if (out_done) HIPCHK(hipEventRecord(out_done, e->s_out));
    return BFHIP_OK;
}

// DEFERRED (lag 1, main stream) and PINGPONG (lag 2, side stream): [K3 of block t-lag | K1 of block t]
// in one launch, then the MAC of block t on the main stream; K3 of block t is owed to a later call (or
// to flush / sync).  Same kernels, same order per channel: same bits.  With ping-pong the MAC of t-1
// (main) and the fused launch (side) overlap: K1 fills the spare ring slot, K3 reads the third Zp buffer.
static int block_owed(bfhip_engine *e, const void *rawin_dev, void *rawout_dev,
                      hipEvent_t in_ready, hipEvent_t out_done) {
    int r;
    const bool side = e->mode == BFHIP_MODE_PINGPONG;
    const int zi = (int)(e->blocks_done % (unsigned)zp_depth(e));
    e->ls = in_stream(e);
    if (in_ready) HIPCHK(hipStreamWaitEvent(e->ls, in_ready, 0));
    if ((r = record_begin(e, T_IN)) != BFHIP_OK) return r;
    if (e->pendq.size() >= (size_t)output_lag(e)) {
        const bfhip_engine::Pending p = e->pendq.front();     // popped once its launch is in the stream
        if (p.mac_done) HIPCHK(hipStreamWaitEvent(e->ls, p.mac_done, 0));
        if ((r = fused_outputs_inputs(e, p.Zp, p.chunk_stride, p.n_chunks, 0, e->n_ch[1], p.rawout, rawin_dev)) != BFHIP_OK) return r;
        e->pendq.pop_front();
        if (p.out_done) HIPCHK(hipEventRecord(p.out_done, e->ls));
    } else {
        if ((r = do_inputs(e, rawin_dev)) != BFHIP_OK) return r;
    }
    if ((r = record_end(e, T_IN)) != BFHIP_OK) return r;
    if (side) {
        const int par = (int)(e->blocks_done & 1ull);
        HIPCHK(hipEventRecord(e->ev_io[par], e->s_in));
        e->ls = e->stream;
        HIPCHK(hipStreamWaitEvent(e->stream, e->ev_io[par], 0));
    }
    if ((r = block_mac(e, zi)) != BFHIP_OK) return r;
    bfhip_engine::Pending np;
    np.Zp = e->d_Zp[zi]; np.chunk_stride = (size_t)e->n_out_padded * e->L; np.n_chunks = e->n_chunks;
    if (e->n_chunks > 2 && !e->zp_long[zi]) {
        // many partials (few outputs, many inputs: an output-sharded rank; few long filters): add them
        // up with the whole chip here, in place, same order -- the fused launch that owes this block's
        // output then reads one spectrum per channel (and exists: it takes at most two)
        if ((r = sum_chunks(e, np.Zp, np.Zp)) != BFHIP_OK) return r;
        np.n_chunks = 1;
    }
    if (side) {
        HIPCHK(hipEventRecord(e->ev_mac3[zi], e->stream));
        np.mac_done = e->ev_mac3[zi];
    }
    np.rawout = rawout_dev; np.out_done = out_done;
    e->pendq.push_back(np);
    return BFHIP_OK;
}

static int block_dev_impl(bfhip_engine *e, const void *rawin_dev, void *rawout_dev,
                          hipEvent_t in_ready, hipEvent_t out_done) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if (!rawin_dev || !rawout_dev) return fail(BFHIP_EINVAL, "block_dev: null buffer");
    timing_begin(e);
    LsGuard guard{e};
    switch (e->mode) {
    case BFHIP_MODE_PIPELINED: r = block_three_streams(e, rawin_dev, rawout_dev, in_ready, out_done); break;
    case BFHIP_MODE_DEFERRED:
    case BFHIP_MODE_PINGPONG: r = block_owed(e, rawin_dev, rawout_dev, in_ready, out_done); break;
    default:                           // the three passes in order on the main stream
        e->ls = e->stream;
        // the caller's producer of rawin_dev (any stream): K1 must not start before it is done
        if (in_ready) HIPCHK(hipStreamWaitEvent(e->stream, in_ready, 0));
        r = block_in_order(e, rawin_dev, (int)(e->blocks_done % (unsigned)zp_depth(e)), rawout_dev);
        // rawout_dev of THIS block is complete (and rawin_dev no longer needed) once this fires
        if (r == BFHIP_OK && out_done) HIPCHK(hipEventRecord(out_done, e->stream));
    }
    if (r != BFHIP_OK) return r;
    advance(e);
    return BFHIP_OK;
}

int bfhip_engine_block_dev(bfhip_engine *e, const void *rawin_dev, void *rawout_dev) {
    return block_dev_impl(e, rawin_dev, rawout_dev, nullptr, nullptr);
}

int bfhip_engine_block_dev_ev(bfhip_engine *e, const void *rawin_dev, void *rawout_dev,
                              void *in_ready_event, void *out_done_event) {
    return block_dev_impl(e, rawin_dev, rawout_dev, (hipEvent_t)in_ready_event, (hipEvent_t)out_done_event);
}

int bfhip_engine_enable_pairs(bfhip_engine *e, int on) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    if (e->finalized) return fail(BFHIP_ESTATE, "enable_pairs after finalize");
    e->pairs = on != 0;
    return BFHIP_OK;
}

// Two consecutive blocks, ONE pass over the coefficients (mac_xbar2_kernel).  Falls back to two
// single blocks whenever the plan is not a plain uniform crossbar or its rings are not full yet:
// the outputs are the same bits either way.
int bfhip_engine_block_pair_dev(bfhip_engine *e, const void *rawin0_dev, void *rawout0_dev,
                                const void *rawin1_dev, void *rawout1_dev) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if (!rawin0_dev || !rawout0_dev || !rawin1_dev || !rawout1_dev) return fail(BFHIP_EINVAL, "block_pair_dev: null buffer");
    bool plain = e->pairs && e->all_dense && !e->mac_diag && e->mac_nt && e->mac_unroll == 0 && !e->any_fading &&
                 !e->ch.has_vchan && !e->big && !e->rt.on && e->d_Zp[1] != nullptr && e->blocks_done >= (unsigned long long)e->N;
    for (auto &lj : e->level_jobs) plain = plain && !lj.n_fill && !lj.n_filt && !lj.n_fade;
    if (!plain) {
        if ((r = bfhip_engine_block_dev(e, rawin0_dev, rawout0_dev)) != BFHIP_OK) return r;
        return bfhip_engine_block_dev(e, rawin1_dev, rawout1_dev);
    }
    if ((r = flush_pending(e)) != BFHIP_OK) return r;          // an output owed by a single block goes first
    LsGuard guard{e};
    e->ls = e->stream;
    timing_begin(e);
    if ((r = record_begin(e, T_IN)) != BFHIP_OK) return r;
    if ((r = do_inputs(e, rawin0_dev, 0u)) != BFHIP_OK) return r;
    if ((r = do_inputs(e, rawin1_dev, 1u)) != BFHIP_OK) return r;
    if ((r = record_end(e, T_IN)) != BFHIP_OK) return r;
    if ((r = record_begin(e, T_MAC)) != BFHIP_OK) return r;
    if ((r = do_mac_pair(e, e->d_Zp[0], e->d_Zp[1])) != BFHIP_OK) return r;
    e->zp_last = 1;
    if ((r = record_end(e, T_MAC)) != BFHIP_OK) return r;
    if ((r = record_begin(e, T_OUT)) != BFHIP_OK) return r;
    const size_t stride = (size_t)e->n_out_padded * e->L;
    if ((r = do_outputs(e, e->d_Zp[0], stride, e->n_chunks, 0, e->n_ch[1], rawout0_dev)) != BFHIP_OK) return r;
    if ((r = do_outputs(e, e->d_Zp[1], stride, e->n_chunks, 0, e->n_ch[1], rawout1_dev)) != BFHIP_OK) return r;
    if ((r = record_end(e, T_OUT)) != BFHIP_OK) return r;
    e->n_pair_launches++;
    advance(e);
    advance(e);
    return BFHIP_OK;
}

unsigned long long bfhip_engine_pair_launches(const bfhip_engine *e) { return e ? e->n_pair_launches : 0ull; }

int bfhip_engine_flush(bfhip_engine *e) {
    if (!e || !e->finalized) return fail(BFHIP_ESTATE, "engine not finalized");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    return flush_pending(e);
}

int bfhip_engine_output_lag(const bfhip_engine *e) {
    if (!e || !e->finalized) return 0;
    return output_lag(e);
}

int bfhip_engine_sync(bfhip_engine *e) {
    if (!e || !e->finalized) return fail(BFHIP_ESTATE, "engine not finalized");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { int _r = flush_pending(e); if (_r != BFHIP_OK) return _r; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    int st = 0;
    HIPCHK(hipMemcpy(&st, e->d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) HIPCHK(hipMemset(e->d_status, 0, sizeof(int)));
    return st;
}

int bfhip_engine_block(bfhip_engine *e, const void *rawin, void *rawout, bfhip_overflow overflow[]) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if (!rawin || !rawout) return fail(BFHIP_EINVAL, "block: null buffer");
    static_assert(sizeof(bfhip_overflow) == sizeof(DevOverflow), "overflow struct layout");
    const hipStream_t sin = in_stream(e), sout = out_stream(e);
    if (overflow) HIPCHK(hipMemcpyAsync(e->d_over, overflow, e->n_ch[1] * sizeof(DevOverflow), hipMemcpyHostToDevice, sout));
    HIPCHK(hipMemcpyAsync(e->d_rawin, rawin, e->raw_bytes[0], hipMemcpyHostToDevice, sin));
    if ((r = bfhip_engine_block_dev(e, e->d_rawin, e->d_rawout)) != BFHIP_OK) return r;
    if ((r = flush_pending(e)) != BFHIP_OK) return r;          // host buffers: this block's output is due now
    if (e->sharded) {
        // rawout is shared with the engines of the other filter processes: only this engine's
        // samples (and overflow entries) may land in it
        e->h_stage.resize(e->raw_bytes[1] + (size_t)e->n_ch[1] * sizeof(DevOverflow));
        HIPCHK(hipMemcpyAsync(e->h_stage.data(), e->d_rawout, e->raw_bytes[1], hipMemcpyDeviceToHost, sout));
        if (overflow) HIPCHK(hipMemcpyAsync(e->h_stage.data() + e->raw_bytes[1], e->d_over, e->n_ch[1] * sizeof(DevOverflow), hipMemcpyDeviceToHost, sout));
        const int st = bfhip_engine_sync(e);
        if (st < 0) return st;
        copy_owned(e, rawout, e->h_stage.data());
        if (overflow) copy_owned_overflow(e, overflow, e->h_stage.data() + e->raw_bytes[1]);
        return st;
    }
    HIPCHK(hipMemcpyAsync(rawout, e->d_rawout, e->raw_bytes[1], hipMemcpyDeviceToHost, sout));
    if (overflow) HIPCHK(hipMemcpyAsync(overflow, e->d_over, e->n_ch[1] * sizeof(DevOverflow), hipMemcpyDeviceToHost, sout));
    return bfhip_engine_sync(e);
}

int bfhip_engine_rt_begin(bfhip_engine *e, int flags) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if ((r = flush_pending(e)) != BFHIP_OK) return r;
    if (e->rt.on) return fail(BFHIP_ESTATE, "rt_begin: already in real-time mode");
    if ((r = sync_all(e)) != BFHIP_OK) return r;
    // one stream: a period is needed back as soon as possible (deferred output stays what it was)
    if (e->mode == BFHIP_MODE_PIPELINED || e->mode == BFHIP_MODE_PINGPONG) e->mode = BFHIP_MODE_SEQUENTIAL;
    auto &rt = e->rt;
    rt.flags = flags;
    for (int p = 0; p < 2; p++) {
        HIPCHK(pin_alloc(&rt.h_in[p], e->raw_bytes[0] + 16, hipHostMallocDefault));
        HIPCHK(pin_alloc(&rt.h_out[p], e->raw_bytes[1] + 16, hipHostMallocDefault));
        HIPCHK(pin_alloc((void **)&rt.h_over[p], e->n_ch[1] * sizeof(DevOverflow), hipHostMallocDefault));
        HIPCHK(pin_alloc((void **)&rt.h_status[p], 2 * sizeof(int), hipHostMallocDefault));
        memset(rt.h_in[p], 0, e->raw_bytes[0]);
        memset(rt.h_out[p], 0, e->raw_bytes[1]);
        memset(rt.h_over[p], 0, e->n_ch[1] * sizeof(DevOverflow));
        rt.h_status[p][0] = rt.h_status[p][1] = 0;
        HIPCHK(hipEventCreateWithFlags(&rt.done[p], hipEventDisableTiming));
        if (flags & BFHIP_RT_OVERLAP) {
            HIPCHK(hipEventCreateWithFlags(&rt.ev_h2d[p], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&rt.ev_cmp[p], hipEventDisableTiming));
            HIPCHK(dev_alloc((void **)&rt.d_in[p], e->raw_bytes[0] + 16));
            HIPCHK(dev_alloc((void **)&rt.d_out[p], e->raw_bytes[1] + 16));
            HIPCHK(hipMemset(rt.d_out[p], 0, e->raw_bytes[1] + 16));
        }
    }
    if (flags & BFHIP_RT_OVERLAP) {
        HIPCHK(hipStreamCreateWithFlags(&rt.s_h2d, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&rt.s_d2h, hipStreamNonBlocking));
    }
    HIPCHK(dev_alloc((void **)&e->d_bs, sizeof(BlockState)));
    HIPCHK(dev_alloc((void **)&e->d_rt_arrive, sizeof(unsigned int)));
    HIPCHK(hipMemset(e->d_rt_arrive, 0, sizeof(unsigned int)));
    rt.on = true;
    rt.bs_synced = false;
    return BFHIP_OK;
}

int bfhip_engine_rt_end(bfhip_engine *e) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    if (!e->rt.on) return BFHIP_OK;
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { int r = sync_all(e); if (r != BFHIP_OK) return r; }
    rt_release(e);
    return BFHIP_OK;
}

void *bfhip_engine_rt_buffer(bfhip_engine *e, int io, int index) {
    if (!e || !e->rt.on || io < 0 || io > 1 || index < 0 || index > 1) return nullptr;
    return io == 0 ? e->rt.h_in[index] : e->rt.h_out[index];
}

int bfhip_engine_rt_submit(bfhip_engine *e, const void *rawin) {
    if (!e || !e->rt.on) return fail(BFHIP_ESTATE, "rt_submit: not in real-time mode");
    auto &rt = e->rt;
    if (rt.submitted - rt.waited >= 2) return fail(BFHIP_ESTATE, "rt_submit: two periods already in flight");
    int r = ensure_ready(e);                   // control changes since the last block rebuild the plan
    if (r != BFHIP_OK) return r;
    const int p = (int)(rt.submitted & 1);
    if (rawin && rawin != rt.h_in[p]) memcpy(rt.h_in[p], rawin, e->raw_bytes[0]);
    if (!rt.bs_synced || rt.bs_t != e->blockcounter) {
        // blocks went through the other entry points (or this is the first period)
        BlockState bs;
        bs.t = e->blockcounter;
        bs.age = block_age(e);
        bs.n_blocks = 0; bs.pad = 0;
        bs.wrap_at = e->wrap_at; bs.wrap_by = e->wrap_by;
        HIPCHK(hipMemcpyAsync(e->d_bs, &bs, sizeof(bs), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        rt.bs_synced = true;
    }
    rt.h_status[p][1] = 0;
    if (rt_graphable(e) && rt.primed) {
        if (!rt.valid[p] && (r = rt_capture(e, p)) != BFHIP_OK) return r;
        HIPCHK(hipGraphLaunch(rt.exec[p], e->stream));
        rt.n_graph++;
    } else {
        // first block after a plan change (also sets the kernels' LDS attributes outside any
        // capture), cross-fade blocks, per-block job tables: plain launches
        timing_begin(e);
        if ((r = rt_enqueue(e, p)) != BFHIP_OK) return r;
        rt.primed = true;
        rt.n_direct++;
    }
    if (!(rt.flags & BFHIP_RT_OVERLAP)) HIPCHK(hipEventRecord(rt.done[p], e->stream));   // else: after the download
    rt.submitted++;
    advance(e);
    rt.bs_t = e->blockcounter;
    return BFHIP_OK;
}

int bfhip_engine_rt_wait(bfhip_engine *e, void *rawout, bfhip_overflow overflow[]) {
    if (!e || !e->rt.on) return fail(BFHIP_ESTATE, "rt_wait: not in real-time mode");
    auto &rt = e->rt;
    if (rt.submitted == rt.waited) return fail(BFHIP_ESTATE, "rt_wait: nothing in flight");
    const int p = (int)(rt.waited & 1);
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    if ((rt.flags & BFHIP_RT_SPIN) && !(rt.flags & BFHIP_RT_OVERLAP)) {
        // the tail kernel's last store is the sequence word: watch it from the CPU; after 2 ms
        // by the clock (checked every 256 polls) fall back to the runtime, so that a device
        // error cannot hang the caller and a long block does not burn the core for its whole length
        volatile int *seq = rt.h_status[p] + 1;
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (unsigned spin = 1; *seq == 0; spin++) {
            __builtin_ia32_pause();
            if ((spin & 255u) == 0) {
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1000000000L + (t1.tv_nsec - t0.tv_nsec) > 2000000L) break;
            }
        }
        // seen: every store of the block (the tail kernel's copy-out included) is visible
        if (*seq == 0 || (rt.flags & BFHIP_RT_COPY_ENGINE)) HIPCHK(hipEventSynchronize(rt.done[p]));
    } else {
        HIPCHK(hipEventSynchronize(rt.done[p]));
    }
    rt.waited++;
    if (rawout && rawout != rt.h_out[p]) copy_owned(e, rawout, rt.h_out[p]);      // (a sharded engine: its own samples only)
    if (overflow) {
        // The reference reads icomm->overflow[ch] at every block and writes it back (bfrun.c:1929-1936),
        // so a reset by another process (bf_reset_peak: the CLI's peak reset) is picked up by the next
        // block.  Here the structs live on the device between periods: an entry the HOST changed since
        // this engine last wrote it becomes the device's state (queued behind whatever is in flight),
        // and the host's value stands until a period that started after the change reports.
        const int O = e->n_ch[1];
        const DevOverflow *dev = rt.h_over[p];
        const unsigned long long period = rt.waited - 1;                 // the period this call collected
        if ((int)rt.last_over.size() != O) { rt.last_over.assign(O, DevOverflow()); rt.over_from.assign(O, 0ull); rt.last_valid = false; }
        for (int o = 0; o < O; o++) {
            if (e->sharded && !e->out_active[o]) continue;
            DevOverflow &seen = rt.last_over[o];
            if (rt.last_valid && memcmp(&overflow[o], &seen, sizeof(DevOverflow)) != 0) {
                HIPCHK(hipMemcpyAsync(&e->d_over[o], &overflow[o], sizeof(DevOverflow), hipMemcpyHostToDevice, e->stream));
                memcpy(&seen, &overflow[o], sizeof(DevOverflow));
                rt.over_from[o] = rt.submitted;                           // periods submitted from now on count on the new state
                continue;
            }
            if (period < rt.over_from[o]) continue;                       // still a period from before the host's change
            memcpy(&overflow[o], &dev[o], sizeof(DevOverflow));
            memcpy(&seen, &dev[o], sizeof(DevOverflow));
        }
        rt.last_valid = true;
    }
    return rt.h_status[p][0];
}

int bfhip_engine_rt_block(bfhip_engine *e, const void *rawin, void *rawout, bfhip_overflow overflow[]) {
    int r = bfhip_engine_rt_submit(e, rawin);
    if (r != BFHIP_OK) return r;
    return bfhip_engine_rt_wait(e, rawout, overflow);
}

int bfhip_engine_rt_stats(const bfhip_engine *e, unsigned long long *graph_blocks,
                          unsigned long long *direct_blocks, unsigned long long *captures) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    if (graph_blocks) *graph_blocks = e->rt.n_graph;
    if (direct_blocks) *direct_blocks = e->rt.n_direct;
    if (captures) *captures = e->rt.n_capture;
    return BFHIP_OK;
}

// ---- self test of the wave FFT's host half: its per-thread twiddle table, no device involved ----
int bfhip_selftest_fail_alloc(int nth) {
    const int left = g_fail_alloc;             // > 0: the allocation armed before was never reached
    g_fail_alloc = nth > 0 ? nth : 0;
    return left;
}

int bfhip_selftest_wave_twiddles(int log2l, int realsize, void *out, int out_bytes) {
    if (!wave_fft_ok(log2l, realsize)) return fail(BFHIP_EINVAL, "selftest_wave_twiddles: length / precision not covered");
    const std::vector<unsigned char> t = make_wave_twiddle_table(log2l, realsize);
    if (out == nullptr) return (int)t.size();
    if ((size_t)out_bytes < t.size()) return fail(BFHIP_EINVAL, "selftest_wave_twiddles: buffer too small");
    memcpy(out, t.data(), t.size());
    return (int)t.size();
}

// ---- self test of the host-side delay machine: no device involved ---------------------------
struct bfhip_selftest_delay { DelayLine dl; };

bfhip_selftest_delay *bfhip_selftest_delay_new(int fragment, int initdelay, int maxdelay, int sample_size) {
    if (fragment < 1 || sample_size < 1 || initdelay < 0) { fail(BFHIP_EINVAL, "selftest_delay_new: bad argument"); return nullptr; }
    bfhip_selftest_delay *d = new bfhip_selftest_delay();
    d->dl.host = true;
    if (d->dl.init(fragment, initdelay, maxdelay, sample_size) != BFHIP_OK) { delete d; fail(BFHIP_ENOMEM, "selftest_delay_new: out of memory"); return nullptr; }
    return d;
}

int bfhip_selftest_delay_update(bfhip_selftest_delay *d, void *buf, int delay) {
    if (!d || !buf) return fail(BFHIP_EINVAL, "selftest_delay_update: bad argument");
    std::vector<ByteOp> ops;
    d->dl.update((uint8_t *)buf, delay, ops);
    for (const ByteOp &o : ops) {
        // the device runs every move with one thread per byte: source and destination of a move
        // must not overlap
        if (o.src && !(o.src + o.n <= o.dst || o.dst + o.n <= o.src)) return fail(BFHIP_ESTATE, "delay machine emitted an overlapping move");
        if (o.src) memcpy(o.dst, o.src, o.n); else memset(o.dst, 0, o.n);
    }
    return (int)ops.size();
}

void bfhip_selftest_delay_free(bfhip_selftest_delay *d) {
    if (!d) return;
    free(d->dl.arena);
    delete d;
}

int bfhip_engine_prewarm(bfhip_engine *e) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if (e->blocks_done != 0) return fail(BFHIP_ESTATE, "prewarm: blocks have been processed already");
    // N blocks of silence are what the zero-initialised rings hold: count them as processed, and
    // move the block counter past the point where (blockcounter - p - delay) would wrap
    e->blocks_done = (unsigned long long)e->N;
    e->blockcounter = (unsigned int)e->R;
    e->la_epoch++;
    { const int rp = la_prime(e); if (rp != BFHIP_OK) return rp; }
    e->rt.bs_synced = false;
    return BFHIP_OK;
}

int bfhip_engine_set_status_dev(bfhip_engine *e, int *status_dev) {
    if (!e || !e->finalized) return fail(BFHIP_ESTATE, "set_status_dev: engine not finalized");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    if (!e->d_status_own) e->d_status_own = e->d_status;
    e->d_status = status_dev ? status_dev : e->d_status_own;
    e->rt.valid[0] = e->rt.valid[1] = false;
    return BFHIP_OK;
}

int bfhip_engine_set_stream(bfhip_engine *e, void *hip_stream) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    if (e->finalized) { int _r = flush_pending(e); if (_r != BFHIP_OK) return _r; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    e->stream = (hipStream_t)hip_stream;
    e->ls = e->stream;
    e->own_stream = false;
    return BFHIP_OK;
}

int bfhip_engine_get_overflow(bfhip_engine *e, int ch, bfhip_overflow *of) {
    if (!e || !e->finalized || ch < 0 || ch >= e->n_ch[1] || !of) return fail(BFHIP_EINVAL, "get_overflow: bad argument");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { int _r = flush_pending(e); if (_r != BFHIP_OK) return _r; }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    HIPCHK(hipMemcpy(of, e->d_over + ch, sizeof(DevOverflow), hipMemcpyDeviceToHost));
    return BFHIP_OK;
}

int bfhip_engine_reset_overflow(bfhip_engine *e) {
    if (!e || !e->finalized) return fail(BFHIP_ESTATE, "engine not finalized");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    std::vector<DevOverflow> v(e->n_ch[1]);
    for (int c = 0; c < e->n_ch[1]; c++) {
        memset(&v[c], 0, sizeof(DevOverflow));
        v[c].max = overflow_max(e->fmt[1][e->ch.v2p[1][c]]);
    }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    HIPCHK(hipMemcpy(e->d_over, v.data(), v.size() * sizeof(DevOverflow), hipMemcpyHostToDevice));
    return BFHIP_OK;
}

unsigned int bfhip_engine_blockcounter(const bfhip_engine *e) { return e ? e->blockcounter : 0; }
int bfhip_engine_block_mode(const bfhip_engine *e) {
    if (!e || !e->finalized) return -1;
    return e->mode;
}
int bfhip_engine_uses_wave_fft(const bfhip_engine *e) { return e && e->wave ? 1 : 0; }
int bfhip_engine_uses_stream_layout(const bfhip_engine *e) { return e && e->hstream.base ? 1 : 0; }
int bfhip_engine_uses_diag_mac(const bfhip_engine *e) { return e && e->mac_diag ? 1 : 0; }
int bfhip_engine_window_blocks(const bfhip_engine *e) {
    if (!e) return fail(BFHIP_EINVAL, "window_blocks: null engine");
    return e->lw_active ? 4 : 2;
}
int bfhip_engine_lookahead_blocks(const bfhip_engine *e) {
    if (!e) return fail(BFHIP_EINVAL, "lookahead_blocks: null engine");
    return e->lw_active && e->la_active && !e->rt.on ? 3 : 0;
}
int bfhip_engine_lookahead_far_blocks(const bfhip_engine *e) {
    if (!e) return fail(BFHIP_EINVAL, "lookahead_far_blocks: null engine");
    return e->lw_active && e->la_active && e->far_active && !e->rt.on ? LA_FAR : 0;
}
int bfhip_engine_ring_depth(const bfhip_engine *e) { return e ? e->R : 0; }
int bfhip_engine_mac_counts(const bfhip_engine *e, unsigned long long *counts) {
    if (!e || !counts) return fail(BFHIP_EINVAL, "mac_counts: null %s", e ? "array" : "engine");
    counts[0] = e->n_mac_launches;
    counts[1] = e->n_la_head;
    counts[2] = e->n_la_full;
    return BFHIP_OK;
}

int bfhip_engine_enable_timing(bfhip_engine *e, int on) {
    if (!e) return fail(BFHIP_EINVAL, "null engine");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    if (on && e->ev.empty()) {
        e->ev.resize((size_t)MAX_TIMED * EV_PER_BLOCK);
        for (auto &x : e->ev) HIPCHK(hipEventCreate(&x));
        e->ev_mask.assign(MAX_TIMED, 0);
    }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    e->timing = on != 0;
    e->timing_stride = on > 1 ? on : 1;
    e->ev_used = 0;
    e->timed_for = ~0ull;
    e->timed_now = false;
    return BFHIP_OK;
}

int bfhip_engine_get_timing(bfhip_engine *e, double ms[4]) {
    if (!e || !ms) return fail(BFHIP_EINVAL, "get_timing: bad argument");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    ms[0] = ms[1] = ms[2] = ms[3] = 0;                      // T_IN, T_MAC, T_OUT, blocks with a MAC
    int cnt[3] = {0, 0, 0};
    for (int i = 0; i < e->ev_used; i++) {
        for (int k = T_IN; k <= T_OUT; k++) {
            if (!(e->ev_mask[i] & (1 << k))) continue;      // phase not launched through a timed entry point
            float t = 0;
            HIPCHK(hipEventElapsedTime(&t, e->ev[(size_t)i * EV_PER_BLOCK + 2 * k], e->ev[(size_t)i * EV_PER_BLOCK + 2 * k + 1]));
            ms[k] += t;
            cnt[k]++;
        }
    }
    for (int k = T_IN; k <= T_OUT; k++) if (cnt[k] > 0) ms[k] /= cnt[k];
    ms[3] = cnt[T_MAC];
    e->ev_used = 0;
    return BFHIP_OK;
}

// The reference's `benchmark: true` table (bfrun.c:2035-2078), device side.
int bfhip_engine_stage_times(bfhip_engine *e, double ms[8]) {
    if (!e || !ms) return fail(BFHIP_EINVAL, "stage_times: bad argument");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    for (int k = 0; k < 8; k++) ms[k] = 0;
    double sum[EV_PAIRS] = {0, 0, 0, 0, 0};
    int n_blocks = 0;
    for (int i = 0; i < e->ev_used; i++) {
        if (!(e->ev_mask[i] & (1 << T_MAC))) continue;      // no MAC timed: not a whole block
        n_blocks++;
        for (int k = 0; k < EV_PAIRS; k++) {
            if (!(e->ev_mask[i] & (1 << k))) continue;
            float t = 0;
            HIPCHK(hipEventElapsedTime(&t, e->ev[(size_t)i * EV_PER_BLOCK + 2 * k], e->ev[(size_t)i * EV_PER_BLOCK + 2 * k + 1]));
            sum[k] += t;
        }
    }
    e->ev_used = 0;
    if (n_blocks == 0) return 0;
    const double post = sum[T_POST] / n_blocks, out = sum[T_OUT] / n_blocks;
    ms[1] = sum[T_IN] / n_blocks;                           // time2freq (+ raw2real, fused)
    ms[2] = sum[T_LEVELS] / n_blocks;                       // mixscale1: the per-filter input mixes / cascades
    ms[3] = sum[T_MAC] / n_blocks;                          // convolve (+ mixscale1 of plain filters, mixscale2: fused)
    ms[5] = out > post ? out - post : 0.0;                  // freq2time (+ real2raw of undithered 1:1 outputs, fused)
    ms[6] = post;                                           // real2raw: dither, N:1 mix, sub-sample delay passes
    ms[7] = ms[1] + ms[2] + ms[3] + ms[5] + ms[6];
    return n_blocks;
}

int bfhip_engine_algorithmic_bytes(bfhip_engine *e, double bytes[2]) {
    int r = ensure_ready(e);
    if (r != BFHIP_OK) return r;
    if (!bytes) return fail(BFHIP_EINVAL, "algorithmic_bytes: null array");
    bytes[0] = e->alg_bytes_total;
    bytes[1] = e->alg_bytes_mac;
    return BFHIP_OK;
}

int bfhip_engine_read_output_spectrum(bfhip_engine *e, int ch, void *dst) {
    if (!e || !e->finalized || ch < 0 || ch >= e->n_ch[1] || !dst) return fail(BFHIP_EINVAL, "read_output_spectrum: bad argument");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    if (e->zp_long[e->zp_last])
        return fail(BFHIP_ESTATE, "read_output_spectrum: the last block ran the long-window plan, whose output spectra "
                    "have 2L bins of a 4L-point transform; set BFHIP_LONG_WINDOW=0 to read standard spectra");
    const size_t row = (size_t)e->L * e->csize();
    std::vector<unsigned char> tmp(row);
    memset(dst, 0, row);
    const unsigned char *zp = (const unsigned char *)e->d_Zp[e->zp_last];
    for (int c = 0; c < (e->zp_is_sum ? 1 : e->n_chunks); c++) {
        HIPCHK(hipMemcpy(tmp.data(), zp + ((size_t)c * e->n_out_padded + ch) * row, row, hipMemcpyDeviceToHost));
        const size_t n = (size_t)2 * e->L;
        if (e->rs == 4) for (size_t i = 0; i < n; i++) ((float *)dst)[i] += ((float *)tmp.data())[i];
        else for (size_t i = 0; i < n; i++) ((double *)dst)[i] += ((double *)tmp.data())[i];
    }
    return BFHIP_OK;
}

int bfhip_engine_read_ring_slot(bfhip_engine *e, int ch, int slot, void *dst) {
    if (!e || !e->finalized || ch < 0 || ch >= e->n_ch[0] || slot < 0 || slot >= e->R || !dst) return fail(BFHIP_EINVAL, "read_ring_slot: bad argument");
    { const int ro = check_owner(e); if (ro != BFHIP_OK) return ro; }
    HIPCHK(hipSetDevice(e->device));
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    const size_t row = (size_t)e->L * e->csize();
    HIPCHK(hipMemcpy(dst, (unsigned char *)e->d_ring + ((size_t)ch * e->R + slot) * row, row, hipMemcpyDeviceToHost));
    return BFHIP_OK;
}

}  // extern "C"
