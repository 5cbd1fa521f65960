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
//
// This unit: create / destroy, the configuration setters, finalize, the audio path (block_dev, block,
// sync, overflow) and the run-time control of switches, gains, delays and sub-delays.  block_dev stages
// the period's input, asks the schedule (nupc_sched.h) what every due segment block runs as, launches
// (nupc_kernels.h), and tells the schedule that the period is over.  Set rewrites and equaliser renders
// are nupc_update.hip; the state of all of it is nupc.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dither_init.h"
#include "nupc_kernels.h"
#include "nupc_loudness.h"
#include "subdelay_filter.h"

static thread_local std::string n_err;

int nupc_host::nfail(int code, const std::string &msg) { n_err = msg; if (code == BFHIP_EHIP || code == BFHIP_ENOMEM) (void)hipGetLastError(); return code; }

namespace {

// an output's overflow struct before its first sample (bf_reset_peak)
DevOverflow over_initial(const bfhip_format &f) {
    DevOverflow o;
    memset(&o, 0, sizeof(o));
    o.max = f.isfloat ? 1.0 : (double)((uint64_t)1 << ((f.sbytes << 3) - 1)) - 1;
    return o;
}

// what the kernels keep of a channel's format
DevFormat dev_format(const bfhip_format &f) {
    DevFormat d;
    d.isfloat = f.isfloat; d.swap = f.swap; d.bytes = f.bytes; d.sbytes = f.sbytes;
    d.sample_spacing = f.sample_spacing; d.byte_offset = f.byte_offset; d.alt = nullptr;
    return d;
}

// channel ch of `c` interleaved reals, the layout of the segment engines' outputs and of d_in_real
bfhip_format real_format(int rs, int c, int ch, double scale) {
    bfhip_format f;
    f.isfloat = 1; f.swap = 0; f.bytes = f.sbytes = rs; f.scale = scale;
    f.sample_spacing = c; f.byte_offset = ch * rs;
    return f;
}

// the slice of `taps` (n_taps reals) that segment s covers, as bfhip_engine_add_coeff takes it: a segment
// past the end of the taps gets one zero -> taps taken (0: the zero)
long seg_slice(const bfhip_nupc *n, const Seg &s, const void *taps, long n_taps, std::vector<unsigned char> &zero,
               const void **src) {
    const long avail = n_taps - s.off, cap = (long)s.L * s.N;
    const long take = avail < 0 ? 0 : (avail > cap ? cap : avail);
    *src = (const unsigned char *)taps + (size_t)s.off * n->rs;
    if (take == 0) { zero.assign((size_t)n->rs, 0); *src = zero.data(); }
    return take;
}

}  // namespace

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
        n->sets.sched.seg.push_back({s.L, s.off});
    }
    for (auto &s : n->seg) {
        s.eng = bfhip_engine_create(device, s.L, s.N, realsize, n_in, n_out);
        if (!s.eng) { nfail(BFHIP_EINVAL, std::string("nupc_create: ") + bfhip_last_error()); bfhip_nupc_destroy(n); return nullptr; }
    }
    for (int io = 0; io < 2; io++) {
        const int c = io ? n_out : n_in;
        n->io.fmt[io].resize(c);
        for (int ch = 0; ch < c; ch++) n->io.fmt[io][ch] = real_format(realsize, c, ch, 1.0);   // interleaved frames
    }
    n->sets.sched.crossfade = seg_length[0];          // the reference's one-block fade
    n->og.mirror.gain.assign(n_out, 1.0);
    n->og.mirror.gain_len.assign(n_out, 0);
    n->dl[0].resize(n_in);
    n->dl[1].resize(n_out);
    n->sd.val[0].assign(n_in, BFHIP_UNDEFINED_SUBDELAY);
    n->sd.val[1].assign(n_out, BFHIP_UNDEFINED_SUBDELAY);
    return n;
}

void bfhip_nupc_destroy(bfhip_nupc *n) {
    if (!n) return;
    if (n->owner != getpid()) { for (auto &sg : n->seg) if (sg.eng) bfhip_engine_destroy(sg.eng); delete n; return; }   // a forked child
    (void)hipSetDevice(n->device);
    if (n->stream) (void)hipStreamSynchronize(n->stream);
    for (auto &s : n->seg) if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (n->upd.stream) (void)hipStreamSynchronize(n->upd.stream);
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
    void *p[] = {n->d_acc[0], n->d_acc[1], n->d_in, n->d_rawout, n->io.d_fmt[1], n->og.d, n->st.d_over, n->st.d_status,
                 n->st.d_arrive, n->dither.d_slot, n->dither.d_state, n->dither.d_table, n->dither.d_randmap,
                 n->dither.d_stage, n->sd.d_bank, n->sd.d_hist[0], n->sd.d_hist[1], n->io.d_fmt[0], n->d_in_real, n->d_stage,
                 n->lim.d_ring, n->lim.d_group_of, n->lim.d_groups, n->lim.d_state,
                 n->loud.d_groups, n->loud.d_state, n->loud.d_open, n->loud.d_ring};
    for (void *q : p) if (q) (void)hipFree(q);
    for (auto &side : n->dl) for (auto &d : side) if (d.arena) (void)hipFree(d.arena);
    void *h[] = {n->st.h_status, n->io.h_in, n->io.h_out, n->st.h_over, n->og.h};
    for (void *q : h) if (q) (void)hipHostFree(q);
    upd_release(n);
    if (n->og.ev) (void)hipEventDestroy(n->og.ev);
    if (n->ev_in) (void)hipEventDestroy(n->ev_in);
    if (n->stream) (void)hipStreamDestroy(n->stream);
    delete n;
}

long bfhip_nupc_taps(const bfhip_nupc *n) { return n ? n->taps() : 0; }
int bfhip_nupc_latency(const bfhip_nupc *n) { return n ? n->L0() : 0; }

// raw formats of the L0-frame I/O buffers.  On a side that does not declare its buffer
// (bfhip_nupc_set_buffer_bytes) frames must be interleaved (every channel of the side has the same
// sample_spacing = frame size in samples), the way dai.c lays out one interleaved device, because
// segment k reads L_k consecutive frames of the raw input ring; on one that does, every channel is
// laid out on its own
int bfhip_nupc_set_format(bfhip_nupc *n, int io, int ch, const bfhip_format *f) {
    if (!n || !f || io < 0 || io > 1 || ch < 0 || ch >= (io ? n->n_out : n->n_in)) return nfail(BFHIP_EINVAL, "nupc_set_format: bad argument");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_format after finalize");
    n->io.fmt[io][ch] = *f;
    return BFHIP_OK;
}

int bfhip_nupc_set_buffer_bytes(bfhip_nupc *n, int io, long bytes) {
    if (!n || io < 0 || io > 1 || bytes < 1) return nfail(BFHIP_EINVAL, "nupc_set_buffer_bytes: bad argument");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_buffer_bytes after finalize");
    n->io.buf_bytes[io] = bytes;
    return BFHIP_OK;
}

long bfhip_nupc_buffer_bytes(const bfhip_nupc *n, int io) {
    if (!n || io < 0 || io > 1) return nfail(BFHIP_EINVAL, "nupc_buffer_bytes: bad argument");
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc_buffer_bytes before finalize");
    return (long)n->io.period_bytes[io];
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
        if (n->io.fmt[1][chs[i]].isfloat)
            return nfail(BFHIP_EINVAL, "cannot dither floating point format (output " + std::to_string(chs[i]) + ")");
    }
    int spacing = 0;
    std::vector<int8_t> table;
    const std::string msg = dither_make_table(n_ch, sample_rate, max_size, n->L0(), &spacing, &table);
    if (!msg.empty()) return nfail(BFHIP_EINVAL, msg);
    n->dither.spacing = spacing;
    n->dither.table.swap(table);
    n->dither.ch = chs;
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
        std::vector<unsigned char> zero;
        const void *src;
        const long take = seg_slice(n, s, taps, n_taps, zero, &src);
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
    n->sets.coeff.push_back({set0});
    n->sets.out_scale.push_back(out_scale);
    n->sets.sched.add_filter();
    // kept until finalize: the base of a filter that bfhip_nupc_reserve_eq_base names later
    const size_t keep = (size_t)std::min(n_taps, n->taps()) * n->rs;
    n->eq.taps0.emplace_back((const unsigned char *)taps, (const unsigned char *)taps + keep);
    return BFHIP_OK;
}

// another impulse response for a filter (before finalize): loaded into every segment engine as a
// set of its own with the segment's full partition count, so that update_coeff can rewrite all of it
int bfhip_nupc_add_coeff(bfhip_nupc *n, int filter, const void *taps, long n_taps) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_add_coeff after finalize");
    if (filter < 0 || filter >= (int)n->sets.coeff.size() || !taps || n_taps < 1 || n_taps > n->taps())
        return nfail(BFHIP_EINVAL, "nupc_add_coeff: bad argument");
    OWNER(n);
    int c0 = -1;
    for (auto &s : n->seg) {
        std::vector<unsigned char> zero;
        const void *src;
        const long take = seg_slice(n, s, taps, n_taps, zero, &src);
        const int c = bfhip_engine_add_coeff(s.eng, src, take == 0 ? 1 : (int)take, 1.0, s.N);
        if (c < 0) return nfail(c, std::string("nupc_add_coeff: ") + bfhip_last_error());
        if (c0 >= 0 && c != c0) return nfail(BFHIP_EINVAL, "nupc_add_coeff: the segment engines disagree on coefficient numbering");
        c0 = c;
    }
    for (auto &s : n->seg) s.n_blocks[filter].push_back(s.N);
    n->sets.coeff[filter].push_back(c0);
    return (int)n->sets.coeff[filter].size() - 1;
}

// (C linkage: `seg_assign` is one of the library's dynamic symbols, and the set of those does not change here)
namespace { int seg_assign(Seg &s, const bfhip_nupc *n, const std::vector<Asg> &asg); }

}  // extern "C"

namespace {

// point a segment engine's filters at an assignment (a plan rebuild at its next call if any moved)
int seg_assign(Seg &s, const bfhip_nupc *n, const std::vector<Asg> &asg) {
    for (size_t f = 0; f < asg.size(); f++) {
        if (s.eng_set[f] == asg[f]) continue;
        if (s.eng_set[f].set != asg[f].set) ECHK(bfhip_engine_set_coeff(s.eng, (int)f, n->sets.coeff[f][asg[f].set]));
        // an output scale dirties the plan only (no private ring); out_scale * 1.0 is out_scale
        if (s.eng_set[f].gain != asg[f].gain)
            ECHK(bfhip_engine_set_scale(s.eng, (int)f, BFHIP_OUT, 0, n->sets.out_scale[f] * asg[f].gain));
        s.eng_set[f] = asg[f];
    }
    return BFHIP_OK;
}

// one block of a segment: under one assignment into d_out, or (dual) the input transform once and
// the MAC + inverse transform under the old assignment into d_out and under the new one into
// d_out2.  The engine keeps whichever assignment it ran last, so a run of dual blocks costs one
// plan rebuild each, not two.
int seg_run(bfhip_nupc *n, Seg &s, const uint8_t *in, int mode /* 0 old, 1 new, 2 both */) {
    const std::vector<Asg> &old_asg = n->sets.sched.old_asg(), &live = n->sets.sched.live;
    if (mode != 2) {
        { const int r = seg_assign(s, n, mode == 0 ? old_asg : live); if (r < 0) return r; }
        ECHK(bfhip_engine_block_dev(s.eng, in, s.d_out));
        return BFHIP_OK;
    }
    const bool new_first = s.eng_set == live;
    ECHK(bfhip_engine_inputs_dev(s.eng, in));
    for (int k = 0; k < 2; k++) {
        const bool is_new = (k == 0) == new_first;
        { const int r = seg_assign(s, n, is_new ? live : old_asg); if (r < 0) return r; }
        ECHK(bfhip_engine_mac_dev(s.eng, s.d_z));
        ECHK(bfhip_engine_outputs_dev(s.eng, s.d_z, 0, n->n_out, is_new ? s.d_out2 : s.d_out));
    }
    ECHK(bfhip_engine_advance(s.eng));
    return BFHIP_OK;
}

// ---- finalize, step by step.  The order of the allocations is part of the contract with the tests
// that make the n-th one fail (bfhip_selftest_fail_alloc).

// a zeroed device buffer
template <typename P> int dev_zeroed(P **p, size_t bytes) {
    NCHK(bfhip_internal_dev_alloc((void **)p, bytes));
    NCHK(hipMemset(*p, 0, bytes));
    return BFHIP_OK;
}
// a device copy of a host array
template <typename P> int dev_copy(P **p, const std::vector<P> &v) {
    NCHK(bfhip_internal_dev_alloc((void **)p, v.size() * sizeof(P)));
    NCHK(hipMemcpy(*p, v.data(), v.size() * sizeof(P), hipMemcpyHostToDevice));
    return BFHIP_OK;
}
#define STEP(expr) do { const int _s = (expr); if (_s < 0) return _s; } while (0)

// which sides use sub-delay; a channel without a filter on such a side follows the filtered ones
// sdf_length whole frames later, through its integer delay line (dai.c:205-215, 230-243); a fixed line
// stays fixed
int fin_subdelay_sides(bfhip_nupc *n) {
    for (int io = 0; io < 2; io++) {
        const std::vector<int> &val = n->sd.val[io];
        for (size_t ch = 0; ch < val.size(); ch++) {
            if (val[ch] == BFHIP_UNDEFINED_SUBDELAY) continue;
            if (n->sd.sdf_length <= 0)
                return nfail(BFHIP_EINVAL, std::string("nupc: ") + (io ? "output " : "input ") + std::to_string(ch) +
                             " has a sub-sample delay but bfhip_nupc_enable_subdelay was not called");
            n->sd.use[io] = true;
        }
        if (n->sd.use[io] && val.size() > (size_t)kSdChannels)
            return nfail(BFHIP_EINVAL, "nupc: a side that uses sub-sample delay can have at most " + std::to_string(kSdChannels) + " channels");
        if (!n->sd.use[io]) continue;
        for (size_t ch = 0; ch < val.size(); ch++) {
            if (val[ch] != BFHIP_UNDEFINED_SUBDELAY) continue;
            NupcDelay &d = n->dl[io][ch];
            d.extra = n->sd.sdf_length;
            if (d.maxdelay > 0 && d.req > d.maxdelay) d.req = d.maxdelay;
            if (d.maxdelay == 0) d.req = 0;
            d.req += d.extra;
            if (d.maxdelay >= 0) d.maxdelay += d.extra;
        }
    }
    return BFHIP_OK;
}

// a side that declared its buffer: every channel's L0 samples lie inside it and no byte belongs to
// two channels (a byte map of the buffer)
int check_layout(const bfhip_nupc *n, int io) {
    const size_t total = (size_t)n->io.buf_bytes[io], L0 = (size_t)n->L0();
    std::vector<unsigned char> owned(total, 0);
    for (size_t ch = 0; ch < n->io.fmt[io].size(); ch++) {
        const bfhip_format &f = n->io.fmt[io][ch];
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

// the period buffers' sizes, per side: declared, or L0 interleaved frames
int fin_layout(bfhip_nupc *n) {
    for (int io = 0; io < 2; io++) {
        const int c = io ? n->n_out : n->n_in;
        const std::vector<bfhip_format> &fmt = n->io.fmt[io];
        if (n->io.buf_bytes[io]) {
            // the input side goes through the conversion kernel's argument block (NupcSdVals)
            if (io == BFHIP_IN && c > kSdChannels)
                return nfail(BFHIP_EINVAL, "nupc: an input side that declares its buffer can have at most " + std::to_string(kSdChannels) + " channels");
            STEP(check_layout(n, io));
            n->io.period_bytes[io] = (size_t)n->io.buf_bytes[io];
            continue;
        }
        for (int ch = 0; ch < c; ch++)
            if (fmt[ch].sample_spacing != fmt[0].sample_spacing || fmt[ch].bytes != fmt[0].bytes)
                return nfail(BFHIP_EINVAL, "nupc: all channels of a side must share one interleaved frame layout");
        n->io.frame_bytes[io] = (size_t)fmt[0].sample_spacing * fmt[0].bytes;
        n->io.period_bytes[io] = (size_t)n->L0() * n->io.frame_bytes[io];
    }
    n->io.in_real = n->sd.use[0] || n->io.buf_bytes[0];
    return BFHIP_OK;
}

// the accumulator ring, the raw input ring (or the stage) and the raw output period
int fin_rings(bfhip_nupc *n) {
    long reach = 0;
    for (auto &s : n->seg) reach = std::max(reach, s.off + 2L * s.L);
    int A = 1;
    while (A < reach + n->L0()) A <<= 1;
    n->A = A;
    STEP(dev_zeroed(&n->d_acc[0], (size_t)A * n->n_out * n->rs));
    // two periods of the longest segment: its forward transform may still be reading one while
    // the next is being filled
    n->in_frames = 2 * n->seg.back().L;
    if (n->io.buf_bytes[0]) STEP(dev_zeroed(&n->d_stage, n->io.period_bytes[0]));
    else STEP(dev_zeroed(&n->d_in, (size_t)n->in_frames * n->io.frame_bytes[0]));
    // bytes no output channel owns are never written: they stay zero
    STEP(dev_zeroed(&n->d_rawout, n->io.period_bytes[1]));
    return BFHIP_OK;
}

// what the emit step reads and writes per output (formats, gain records, overflow structs), the status
// words, and the pinned staging of bfhip_nupc_block and of the gain uploads
int fin_emit_state(bfhip_nupc *n) {
    std::vector<DevFormat> df(n->n_out);
    std::vector<DevOverflow> ov(n->n_out);
    GainMirror &g = n->og.mirror;
    g.ramp.resize(n->n_out);
    for (int ch = 0; ch < n->n_out; ch++) {
        const bfhip_format &f = n->io.fmt[1][ch];
        df[ch] = dev_format(f);
        g.ramp[ch] = NupcGain{1.0 / f.scale, g.gain[ch], g.gain[ch], 0, 0};   // bfrun.c:1850: inv * g
        ov[ch] = over_initial(f);
    }
    STEP(dev_copy(&n->io.d_fmt[1], df));
    STEP(dev_copy(&n->og.d, g.ramp));
    STEP(dev_copy(&n->st.d_over, ov));
    STEP(dev_zeroed(&n->st.d_status, sizeof(int)));
    STEP(dev_zeroed(&n->st.d_arrive, sizeof(unsigned int)));
    NCHK(bfhip_internal_pin_alloc((void **)&n->st.h_status, sizeof(int), hipHostMallocDefault));
    NCHK(bfhip_internal_pin_alloc((void **)&n->io.h_in, n->io.period_bytes[0], hipHostMallocDefault));
    NCHK(bfhip_internal_pin_alloc((void **)&n->io.h_out, n->io.period_bytes[1], hipHostMallocDefault));
    NCHK(bfhip_internal_pin_alloc((void **)&n->st.h_over, (size_t)n->n_out * sizeof(DevOverflow), hipHostMallocDefault));
    *n->st.h_status = 0;
    NCHK(bfhip_internal_pin_alloc((void **)&n->og.h, (size_t)n->n_out * sizeof(NupcGain), hipHostMallocDefault));
    NCHK(hipEventCreateWithFlags(&n->og.ev, hipEventDisableTiming));
    NCHK(hipEventRecord(n->og.ev, n->stream));
    g.dirty = false;
    return BFHIP_OK;
}

int fin_dither(bfhip_nupc *n) {
    NupcDither &d = n->dither;
    if (d.ch.empty()) return BFHIP_OK;
    std::vector<int> slot(n->n_out, -1), rank(d.ch.size());
    for (size_t i = 0; i < d.ch.size(); i++) {
        if (n->io.fmt[1][d.ch[i]].isfloat)
            return nfail(BFHIP_EINVAL, "cannot dither floating point format (output " + std::to_string(d.ch[i]) + ")");
        slot[d.ch[i]] = (int)i;
        rank[i] = (int)i;
    }
    STEP(dev_copy(&d.d_slot, slot));
    NCHK(dither_upload_tables(d.table, d.spacing, rank, n->rs, &d.d_table, &d.d_randmap, &d.d_state));
    NCHK(bfhip_internal_dev_alloc(&d.d_stage, d.ch.size() * n->L0() * n->rs));
    return BFHIP_OK;
}

// delay_allocate_buffer per channel, with the channel's own sample size
int fin_delay(bfhip_nupc *n) {
    for (int io = 0; io < 2; io++)
        for (size_t ch = 0; ch < n->dl[io].size(); ch++) {
            NupcDelay &d = n->dl[io][ch];
            const size_t bytes = d.init(n->L0(), n->io.fmt[io][ch].bytes);
            if (bytes) STEP(dev_zeroed(&d.arena, bytes));
        }
    return BFHIP_OK;
}

// the filter bank and the histories of the sides that use sub-delay; the formats and the ring of reals of
// an input side that is converted in front of the segments
int fin_subdelay(bfhip_nupc *n) {
    NupcSubdelay &sd = n->sd;
    if (sd.use[0] || sd.use[1]) {
        const std::vector<unsigned char> bank = sd_make_bank(sd.sdf_length, n->rs);
        NCHK(bfhip_internal_dev_alloc(&sd.d_bank, bank.size()));
        NCHK(hipMemcpy(sd.d_bank, bank.data(), bank.size(), hipMemcpyHostToDevice));
        for (int io = 0; io < 2; io++)
            if (sd.use[io]) STEP(dev_zeroed(&sd.d_hist[io], sd.val[io].size() * sd.bs * n->rs));
    }
    if (!n->io.in_real) return BFHIP_OK;
    std::vector<DevFormat> dfi(n->n_in);
    for (int ch = 0; ch < n->n_in; ch++) {
        const bfhip_format &f = n->io.fmt[0][ch];
        if (!n->io.buf_bytes[0] && (f.byte_offset < 0 || (size_t)f.byte_offset + f.bytes > n->io.frame_bytes[0]))
            return nfail(BFHIP_EINVAL, "nupc: sub-sample delay on a side with a channel whose samples lie outside the raw frame");
        dfi[ch] = dev_format(f);
    }
    STEP(dev_copy(&n->io.d_fmt[0], dfi));
    STEP(dev_zeroed(&n->d_in_real, (size_t)n->in_frames * n->n_in * n->rs));
    return BFHIP_OK;
}

// the spare ring of the switches, if any can happen
int fin_spare_ring(bfhip_nupc *n) {
    n->sets.can_switch = n->sets.gain_reserve;
    for (auto &c : n->sets.coeff) n->sets.can_switch = n->sets.can_switch || c.size() > 1;
    if (n->sets.can_switch) STEP(dev_zeroed(&n->d_acc[1], (size_t)n->A * n->n_out * n->rs));
    return BFHIP_OK;
}

// the segment engines: formats, the initial assignment, their streams and output buffers
int fin_segments(bfhip_nupc *n, int prio_least) {
    const int L0 = n->L0();
    for (auto &s : n->seg) {
        for (int ch = 0; ch < n->n_in; ch++) {
            // in_real: the ring of converted (and filtered) reals; the format's scale stays where it is
            // applied today, in the engines' filter scales
            const bfhip_format raw = n->io.fmt[0][ch], f = n->io.in_real ? real_format(n->rs, n->n_in, ch, raw.scale) : raw;
            ECHK(bfhip_engine_set_format(s.eng, BFHIP_IN, ch, &f));
        }
        for (int ch = 0; ch < n->n_out; ch++) {
            const bfhip_format f = real_format(n->rs, n->n_out, ch, 1.0);
            ECHK(bfhip_engine_set_format(s.eng, BFHIP_OUT, ch, &f));
        }
        STEP(seg_assign(s, n, n->sets.sched.live));          // initial gains other than 1
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
        ECHK(bfhip_engine_set_status_dev(s.eng, n->st.d_status));
        NCHK(bfhip_internal_dev_alloc((void **)&s.d_out, (size_t)s.L * n->n_out * n->rs));
        if (n->sets.can_switch) {
            NCHK(bfhip_internal_dev_alloc((void **)&s.d_out2, (size_t)s.L * n->n_out * n->rs));
            // n_out spectra of L complex numbers (rounded up to the MAC's output groups)
            NCHK(bfhip_internal_dev_alloc((void **)&s.d_z, (size_t)((n->n_out + 7) / 8 * 8) * s.L * 2 * n->rs));
        }
    }
    return BFHIP_OK;
}

// the limiter's rings, state and group table: only under bfhip_nupc_enable_limiter, behind everything else
int fin_limiter(bfhip_nupc *n) {
    NupcLimiter &lm = n->lim;
    if (!lm.on) return BFHIP_OK;
    for (auto &g : lm.groups)
        for (int k = 0; k < g.n_ch; k++) g.scale[k] = n->io.fmt[1][g.ch[k]].scale;
    STEP(dev_zeroed(&lm.d_ring, (size_t)n->n_out * (lm.D + n->L0()) * n->rs));      // x[t < 0] = 0
    STEP(dev_copy(&lm.d_group_of, lm.group_of));
    if (lm.groups.empty()) return BFHIP_OK;              // a pure delay of every output
    STEP(dev_copy(&lm.d_groups, lm.groups));
    std::vector<double> fresh(lm.groups.size() * 2 * lm.state_stride(), 1.0);        // r = e = 1 before frame 0
    if (lm.true_peak())                                  // and nothing detected yet
        for (size_t row = 0; row < lm.groups.size() * 2; row++) fresh[(row + 1) * lm.state_stride() - 1] = 0.0;
    STEP(dev_copy(&lm.d_state, fresh));
    return BFHIP_OK;
}

// the meter's group table, filter states, open partials and rings: only under bfhip_nupc_enable_loudness, behind
// everything else.  The chunk length of the kernel's scan and the transition-matrix powers are fixed here.
int fin_loudness(bfhip_nupc *n) {
    NupcLoudness &ld = n->loud;
    if (!ld.on || ld.groups.empty()) return BFHIP_OK;    // a meter without a group: nothing to launch
    for (auto &g : ld.groups)
        for (int k = 0; k < g.n_ch; k++) g.scale[k] = n->io.fmt[1][g.ch[k]].scale;
    ld.chunk = n->L0() <= kLoudSerialMax ? n->L0() : kLoudChunk;
    kweighting_transition(ld.coef.c, ld.chunk, ld.coef.mp[0]);
    for (int i = 1; i < 8; i++) loudness_mat_mul(ld.coef.mp[i - 1], ld.coef.mp[i - 1], ld.coef.mp[i]);
    STEP(dev_copy(&ld.d_groups, ld.groups));
    STEP(dev_zeroed(&ld.d_state, ld.groups.size() * kLoudGroupMax * 4 * sizeof(double)));
    STEP(dev_zeroed(&ld.d_open, ld.groups.size() * sizeof(double)));
    STEP(dev_zeroed(&ld.d_ring, ld.groups.size() * (size_t)ld.history * sizeof(double)));
    return BFHIP_OK;
}

int finalize_impl(bfhip_nupc *n) {
    OWNER(n);
    STEP(fin_subdelay_sides(n));
    NCHK(hipSetDevice(n->device));
    int prio_least = 0, prio_greatest = 0;
    NCHK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    NCHK(hipStreamCreateWithPriority(&n->stream, hipStreamNonBlocking, prio_greatest));
    NCHK(hipEventCreateWithFlags(&n->ev_in, hipEventDisableTiming));
    if (const char *bg = getenv("BFHIP_NUPC_BACKGROUND")) n->background = atoi(bg) != 0;
    STEP(fin_layout(n));
    STEP(fin_rings(n));
    STEP(fin_emit_state(n));
    STEP(fin_dither(n));
    STEP(fin_delay(n));
    STEP(fin_subdelay(n));
    STEP(fin_spare_ring(n));
    STEP(fin_segments(n, prio_least));
    STEP(upd_finalize(n, prio_least));
    STEP(fin_limiter(n));
    STEP(fin_loudness(n));
    n->finalized = true;
    return BFHIP_OK;
}

}  // namespace

extern "C" {

int bfhip_nupc_finalize(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return BFHIP_OK;
    // half-built state is cleaned up by bfhip_nupc_destroy only: a failed finalize is not retried
    if (n->finalize_failed) return nfail(BFHIP_ESTATE, "nupc_finalize failed before: destroy this convolver");
    const int r = finalize_impl(n);
    if (r != BFHIP_OK) { n->finalize_failed = true; n->finalized = false; }
    return r;
}

// one I/O block of L_0 frames, device-resident raw buffers, asynchronous on the nupc's stream
int bfhip_nupc_block_dev(bfhip_nupc *n, const void *rawin_dev, void *rawout_dev) {
    if (!n || !n->finalized) return nfail(BFHIP_ESTATE, "nupc not finalized");
    if (!rawin_dev || !rawout_dev) return nfail(BFHIP_EINVAL, "nupc_block_dev: null buffer");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    const int L0 = n->L0();
    const unsigned long long opos = n->block * (unsigned long long)L0;            // first frame emitted
    const unsigned long long end = opos + (unsigned long long)L0;                 // samples received
    // ---- stage the input: append to the input ring (segment blocks are aligned: never split by the wrap)
    const size_t wpos = n->in_slot();
    uint8_t *slot = n->in_slot_raw();
    if ((const uint8_t *)rawin_dev != slot)                                   // block() uploads straight into the slot
        NCHK(hipMemcpyAsync(slot, rawin_dev, n->io.period_bytes[0], hipMemcpyDeviceToDevice, n->stream));
    // input delay and mute on the slot, before any segment (or ev_in, which the background
    // segment streams wait on) reads it
    STEP(nupc_delay_side(n, BFHIP_IN, slot));
    // sub-delay or a declared buffer on the input side: convert (and filter) the period once, in
    // front of all segments
    if (n->io.in_real) STEP(nupc_subdelay_in(n, slot, wpos));
    // ---- output gains set since the last block: the records go up when a target changed
    if (n->og.mirror.start()) {
        NCHK(hipEventSynchronize(n->og.ev));                      // the previous upload has read the staging
        std::copy(n->og.mirror.ramp.begin(), n->og.mirror.ramp.end(), n->og.h);
        NCHK(hipMemcpyAsync(n->og.d, n->og.h, (size_t)n->n_out * sizeof(NupcGain), hipMemcpyHostToDevice, n->stream));
        NCHK(hipEventRecord(n->og.ev, n->stream));
    }
    // ---- the segment blocks that are due, each as the schedule says
    Switcher &sched = n->sets.sched;
    sched.commit(opos);
    bool ev_in_recorded = false;
    for (size_t k = 0; k < n->seg.size(); k++) {
        Seg &s = n->seg[k];
        if (end % (unsigned long long)s.L != 0) continue;
        const BlockPlan plan = sched.block(k, end);
        const size_t rpos = (size_t)((end - s.L) % (unsigned long long)n->in_frames);
        const uint8_t *in = n->io.in_real ? n->d_in_real + rpos * (size_t)n->n_in * n->rs : n->d_in + rpos * n->io.frame_bytes[0];
        if (s.delay_steps == 0) {
            STEP(seg_run(n, s, in, plan.mode));
            STEP(nupc_accumulate(n, s, plan));
            continue;
        }
        if (s.pending) return nfail(BFHIP_ESTATE, "nupc: a background segment block was never collected");
        if (!ev_in_recorded) { NCHK(hipEventRecord(n->ev_in, n->stream)); ev_in_recorded = true; }
        NCHK(hipStreamWaitEvent(s.stream, n->ev_in, 0));
        if (s.consumed_once) NCHK(hipStreamWaitEvent(s.stream, s.ev_consumed, 0));   // d_out is free again
        STEP(seg_run(n, s, in, plan.mode));
        NCHK(hipEventRecord(s.ev_done, s.stream));
        s.pending = true;
        s.pending_plan = plan;
        s.due_block = n->block + (unsigned long long)s.delay_steps;
    }
    // ---- the background blocks whose first frame is due in this period
    for (auto &s : n->seg) {
        if (!s.pending || s.due_block != n->block) continue;
        NCHK(hipStreamWaitEvent(n->stream, s.ev_done, 0));
        STEP(nupc_accumulate(n, s, s.pending_plan));
        NCHK(hipEventRecord(s.ev_consumed, n->stream));
        s.pending = false;
        s.consumed_once = true;
    }
    // ---- emit; output delay and mute on the quantised block (block() copies it out behind this)
    if (n->lim.on) STEP(nupc_limit_emit(n, opos, rawout_dev));
    else STEP(nupc_emit(n, opos, rawout_dev));
    n->og.mirror.advance(L0);
    STEP(nupc_delay_side(n, BFHIP_OUT, (uint8_t *)rawout_dev));
    // ---- the loudness meter reads what leaves
    if (n->loud.d_groups) STEP(nupc_loudness(n, opos, rawout_dev));
    n->block++;
    sched.end_period(end);
    return BFHIP_OK;
}

// waits for the periods handed in so far (NOT for background segment blocks that are not due
// yet) and returns the status bits collected since the last call
int bfhip_nupc_sync(bfhip_nupc *n) {
    if (!n || !n->finalized) return nfail(BFHIP_ESTATE, "nupc not finalized");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    NCHK(hipStreamSynchronize(n->stream));
    const int st = *(volatile int *)n->st.h_status;
    *n->st.h_status = 0;
    return st;
}

// host buffers: copies in, runs, copies out, waits; returns status bits
int bfhip_nupc_block(bfhip_nupc *n, const void *rawin, void *rawout, bfhip_overflow overflow[]) {
    if (!n || !n->finalized || !rawin || !rawout) return nfail(BFHIP_ESTATE, "nupc_block: bad state or argument");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    const size_t over_bytes = (size_t)n->n_out * sizeof(DevOverflow);
    // upload straight into this block's slot of the input ring,
    // through pinned staging buffers: copies from pageable memory stall in the runtime every so often
    uint8_t *slot = n->in_slot_raw();
    memcpy(n->io.h_in, rawin, n->io.period_bytes[0]);
    NCHK(hipMemcpyAsync(slot, n->io.h_in, n->io.period_bytes[0], hipMemcpyHostToDevice, n->stream));
    if (overflow) {
        memcpy(n->st.h_over, overflow, over_bytes);
        NCHK(hipMemcpyAsync(n->st.d_over, n->st.h_over, over_bytes, hipMemcpyHostToDevice, n->stream));
    }
    int r = bfhip_nupc_block_dev(n, slot, n->d_rawout);
    if (r < 0) return r;
    NCHK(hipMemcpyAsync(n->io.h_out, n->d_rawout, n->io.period_bytes[1], hipMemcpyDeviceToHost, n->stream));
    if (overflow) NCHK(hipMemcpyAsync(n->st.h_over, n->st.d_over, over_bytes, hipMemcpyDeviceToHost, n->stream));
    r = bfhip_nupc_sync(n);
    if (r < 0) return r;
    memcpy(rawout, n->io.h_out, n->io.period_bytes[1]);
    if (overflow) memcpy(overflow, n->st.h_over, over_bytes);
    return r;
}

int bfhip_nupc_get_overflow(bfhip_nupc *n, int ch, bfhip_overflow *of) {
    if (!n || !n->finalized || !of || ch < 0 || ch >= n->n_out) return nfail(BFHIP_EINVAL, "nupc_get_overflow: bad argument");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    NCHK(hipStreamSynchronize(n->stream));
    NCHK(hipMemcpy(of, n->st.d_over + ch, sizeof(DevOverflow), hipMemcpyDeviceToHost));
    return BFHIP_OK;
}

// bf_reset_peak(): the initial structs go up behind the periods handed in so far and in front of
// the next one, through block()'s pinned staging (idle between block() calls; a second reset
// writes the same bytes into it); no host wait
int bfhip_nupc_reset_overflow(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc not finalized");
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    for (int ch = 0; ch < n->n_out; ch++) n->st.h_over[ch] = over_initial(n->io.fmt[1][ch]);
    NCHK(hipMemcpyAsync(n->st.d_over, n->st.h_over, (size_t)n->n_out * sizeof(DevOverflow), hipMemcpyHostToDevice, n->stream));
    return BFHIP_OK;
}

// ---- run-time control: coefficient switches -------------------------------------------------

static bool filter_ok(const bfhip_nupc *n, int filter) { return filter >= 0 && filter < (int)n->sets.coeff.size(); }

int bfhip_nupc_set_crossfade(bfhip_nupc *n, int frames) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (frames < 0 || frames == 1 || frames > 1048576) return nfail(BFHIP_EINVAL, "nupc_set_crossfade: 0 (hard switch) or 2 .. 1048576 frames");
    n->sets.sched.crossfade = frames;
    return BFHIP_OK;
}

int bfhip_nupc_set_coeff(bfhip_nupc *n, int filter, int coeff) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!filter_ok(n, filter) || coeff < 0 || coeff >= (int)n->sets.coeff[filter].size())
        return nfail(BFHIP_EINVAL, "nupc_set_coeff: bad filter or set");
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_coeff before finalize");
    if (n->sets.sched.busy()) return nfail(BFHIP_ESTATE, "nupc_set_coeff: the previous switch is still in flight (bfhip_nupc_switch_busy)");
    if (n->upd.reserve) {
        STEP(upd_poll(n));
        if (n->upd.inflight && n->upd.rewrites(filter, coeff))
            return nfail(BFHIP_ESTATE, "nupc_set_coeff: a rewrite of this set is in flight (bfhip_nupc_update_busy)");
        if (n->upd.bad[filter][coeff])
            return nfail(BFHIP_ESTATE, "nupc_set_coeff: the last rewrite of this set found a NaN or Inf value among its coefficients");
    }
    n->sets.sched.queued[filter].set = coeff;
    return BFHIP_OK;
}

long bfhip_nupc_switch_frame(const bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_ESTATE, "null");                 // not BFHIP_EINVAL: -1 means "no switch yet"
    return n->sets.sched.t_sw;
}

int bfhip_nupc_switch_busy(const bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    return n->sets.sched.busy() ? 1 : 0;
}

int bfhip_nupc_set_switch_mode(bfhip_nupc *n, int mode) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (mode != BFHIP_NUPC_SWITCH_ALIGNED && mode != BFHIP_NUPC_SWITCH_STAGGERED)
        return nfail(BFHIP_EINVAL, "nupc_set_switch_mode: BFHIP_NUPC_SWITCH_ALIGNED or BFHIP_NUPC_SWITCH_STAGGERED");
    if (n->sets.sched.busy()) return nfail(BFHIP_ESTATE, "nupc_set_switch_mode: the previous switch is still in flight (bfhip_nupc_switch_busy)");
    if (n->sets.sched.has_request())
        return nfail(BFHIP_ESTATE, "nupc_set_switch_mode: a set_coeff / set_filter_gain request is queued");
    n->sets.sched.switch_mode = mode;
    return BFHIP_OK;
}

int bfhip_nupc_get_switch_mode(const bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    return n->sets.sched.switch_mode;
}

long bfhip_nupc_switch_frame_segment(const bfhip_nupc *n, int segment) {
    if (!n) return nfail(BFHIP_ESTATE, "null");                 // not -1: that means "no switch yet"
    if (segment < 0 || segment >= (int)n->seg.size()) return nfail(BFHIP_ESTATE, "nupc_switch_frame_segment: bad segment");
    return (long)n->sets.sched.segment_frame(segment);
}

// ---- run-time control: per-filter gain as part of a switch ----------------------------------

int bfhip_nupc_reserve_filter_gain(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_filter_gain after finalize");
    n->sets.gain_reserve = true;
    return BFHIP_OK;
}

int bfhip_nupc_set_filter_gain(bfhip_nupc *n, int filter, double gain) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!filter_ok(n, filter) || !std::isfinite(gain))
        return nfail(BFHIP_EINVAL, "nupc_set_filter_gain: bad filter, or a gain that is not finite");
    if (!n->finalized) { n->sets.sched.live[filter].gain = gain; return BFHIP_OK; }     // the initial gain
    if (!n->sets.gain_reserve) return nfail(BFHIP_ESTATE, "nupc_set_filter_gain: needs bfhip_nupc_reserve_filter_gain before finalize");
    if (n->sets.sched.busy()) return nfail(BFHIP_ESTATE, "nupc_set_filter_gain: the previous switch is still in flight (bfhip_nupc_switch_busy)");
    n->sets.sched.queued[filter].gain = gain;
    return BFHIP_OK;
}

double bfhip_nupc_get_filter_gain(const bfhip_nupc *n, int filter) {
    if (!n || !filter_ok(n, filter)) { nfail(BFHIP_EINVAL, "nupc_get_filter_gain: bad argument"); return NAN; }
    return n->sets.sched.live[filter].gain;
}

// ---- run-time control: output gain ----------------------------------------------------------

int bfhip_nupc_set_output_gain(bfhip_nupc *n, int out_ch, double gain) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (out_ch < 0 || out_ch >= n->n_out || !std::isfinite(gain)) return nfail(BFHIP_EINVAL, "nupc_set_output_gain: bad argument");
    n->og.mirror.request(out_ch, gain);
    return BFHIP_OK;
}

int bfhip_nupc_set_gain_ramp(bfhip_nupc *n, int frames) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (frames < 0 || frames > 1048576) return nfail(BFHIP_EINVAL, "nupc_set_gain_ramp: 0 (step) or 1 .. 1048576 frames");
    n->og.mirror.gain_ramp = frames;
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
    (void)d.init(n->L0(), 1);
    return d.curdelay;
}

// ---- run-time control: per-channel sub-sample delay -----------------------------------------

int bfhip_nupc_enable_subdelay(bfhip_nupc *n, int sdf_length, double kaiser_beta) {
    (void)kaiser_beta;       // parsed by the reference (sdf_beta) but its filters are built with 9 (delay.c:73)
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_enable_subdelay after finalize");
    const int L0 = n->L0();
    if (sdf_length < 1) return nfail(BFHIP_EINVAL, "Invalid half filter length " + std::to_string(sdf_length) + ".");
    if (2 * sdf_length + 1 > L0) return nfail(BFHIP_EINVAL, "The filter_length must be at least 2 x sdf_length + 1.");
    int bs = 1;
    while (bs < 2 * sdf_length + 1) bs <<= 1;
    if (L0 % bs != 0)
        return nfail(BFHIP_EINVAL, "Incompatible fragment/filter sizes (" + std::to_string(L0) + "/" + std::to_string(2 * sdf_length + 1) + ").");
    if (bs > kSdMaxBs)
        return nfail(BFHIP_EINVAL, "nupc_enable_subdelay: sdf_length above " + std::to_string(kSdMaxBs / 2 - 1) + " is not supported");
    n->sd.sdf_length = sdf_length; n->sd.flen = 2 * sdf_length + 1; n->sd.bs = bs;
    return BFHIP_OK;
}

int bfhip_nupc_set_subdelay(bfhip_nupc *n, int io, int ch, int subdelay) {
    if (!delay_channel_ok(n, io, ch)) return nfail(BFHIP_EINVAL, "nupc_set_subdelay: bad argument");
    const bool in_range = subdelay > -100 && subdelay < 100;
    if (!n->finalized) {
        if (!in_range && subdelay != BFHIP_UNDEFINED_SUBDELAY) return nfail(BFHIP_EINVAL, "nupc_set_subdelay: value out of range (-100, 100)");
        n->sd.val[io][ch] = subdelay;
        return BFHIP_OK;
    }
    // set_subdelay, bfrun.c:520-541
    if (n->sd.val[io][ch] == BFHIP_UNDEFINED_SUBDELAY) return nfail(BFHIP_EINVAL, "nupc_set_subdelay: the channel has no sub-sample delay filter");
    if (!in_range) return nfail(BFHIP_EINVAL, "nupc_set_subdelay: value out of range (-100, 100)");
    n->sd.val[io][ch] = subdelay;               // read by the next block call
    return BFHIP_OK;
}

int bfhip_nupc_get_subdelay(const bfhip_nupc *n, int io, int ch) {
    if (!delay_channel_ok(n, io, ch)) return nfail(BFHIP_EINVAL, "nupc_get_subdelay: bad argument");
    return n->sd.val[io][ch];
}

// ---- look-ahead peak limiter (checks and the definition: limiter_host.h) ---------------------

int bfhip_nupc_enable_limiter(bfhip_nupc *n, int lookahead_frames, double release_frames) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_enable_limiter after finalize");
    if (n->lim.on) return nfail(BFHIP_ESTATE, "nupc_enable_limiter: the limiter is enabled already");
    std::string why;
    if (!limiter_check(lookahead_frames, release_frames, &why)) return nfail(BFHIP_EINVAL, "nupc_enable_limiter: " + why);
    n->lim.on = true;
    n->lim.D = lookahead_frames;
    n->lim.release = release_frames;
    n->lim.a = limiter_release_coef(release_frames);
    n->lim.group_of.assign(n->n_out, -1);
    return BFHIP_OK;
}

int bfhip_nupc_add_limiter_group(bfhip_nupc *n, const int out_channels[], int n_ch, double threshold) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_add_limiter_group after finalize");
    if (!n->lim.on) return nfail(BFHIP_ESTATE, "nupc_add_limiter_group: needs bfhip_nupc_enable_limiter first");
    std::string why;
    if (!limiter_check_group(n->lim.group_of, (int)n->lim.groups.size(), out_channels, n_ch, threshold, &why))
        return nfail(BFHIP_EINVAL, "nupc_add_limiter_group: " + why);
    NupcLimGroup g;
    memset(&g, 0, sizeof(g));
    g.n_ch = n_ch;
    const int index = (int)n->lim.groups.size();
    for (int k = 0; k < n_ch; k++) { g.ch[k] = out_channels[k]; g.scale[k] = 1.0; n->lim.group_of[out_channels[k]] = index; }
    n->lim.groups.push_back(g);
    n->lim.thr.push_back(threshold);
    return index;
}

int bfhip_nupc_set_limiter_threshold(bfhip_nupc *n, int group, double threshold) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (group < 0 || group >= (int)n->lim.groups.size()) return nfail(BFHIP_EINVAL, "nupc_set_limiter_threshold: bad group");
    if (!limiter_threshold_ok(threshold))
        return nfail(BFHIP_EINVAL, "nupc_set_limiter_threshold: the threshold must be > 0 (finite or +INFINITY)");
    n->lim.thr[group] = threshold;                      // read by the next block call
    return BFHIP_OK;
}

double bfhip_nupc_get_limiter_threshold(const bfhip_nupc *n, int group) {
    if (!n || group < 0 || group >= (int)n->lim.groups.size()) { nfail(BFHIP_EINVAL, "nupc_get_limiter_threshold: bad argument"); return NAN; }
    return n->lim.thr[group];
}

int bfhip_nupc_limiter_delay(const bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    return n->lim.on ? n->lim.D : 0;
}

int bfhip_nupc_get_limiter_reduction(bfhip_nupc *n, int group, double *min_gain) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!min_gain || group < 0 || group >= (int)n->lim.groups.size()) return nfail(BFHIP_EINVAL, "nupc_get_limiter_reduction: bad argument");
    *min_gain = 1.0;
    // nothing emitted since the previous call (or ever): the meter on the device is stale or fresh
    if (!n->finalized || n->block == 0 || ((n->lim.meter_reset >> group) & 1u)) return BFHIP_OK;
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    NCHK(hipStreamSynchronize(n->stream));
    // the parity the next block call reads
    const double *cell = n->lim.d_state + ((size_t)group * 2 + (n->block & 1)) * n->lim.state_stride() + 2 * n->lim.De();
    NCHK(hipMemcpy(min_gain, cell, sizeof(double), hipMemcpyDeviceToHost));
    n->lim.meter_reset |= 1u << group;                  // travels with the next block call
    return BFHIP_OK;
}

// ---- true-peak detection for the limiter (taps, checks and the definition: truepeak_host.h) ----

int bfhip_nupc_set_limiter_detector(bfhip_nupc *n, int detector) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_limiter_detector after finalize");
    if (!n->lim.on) return nfail(BFHIP_ESTATE, "nupc_set_limiter_detector: needs bfhip_nupc_enable_limiter first");
    std::string why;
    if (!truepeak_check(detector, n->lim.D, &why)) return nfail(BFHIP_EINVAL, "nupc_set_limiter_detector: " + why);
    n->lim.detector = detector;
    if (n->lim.true_peak()) truepeak_filter(&n->lim.taps);
    return BFHIP_OK;
}

int bfhip_nupc_get_limiter_detector(const bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    return n->lim.detector;
}

int bfhip_nupc_get_limiter_true_peak(bfhip_nupc *n, int group, double *max_peak) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!max_peak || group < 0 || group >= (int)n->lim.groups.size()) return nfail(BFHIP_EINVAL, "nupc_get_limiter_true_peak: bad argument");
    if (!n->lim.true_peak()) return nfail(BFHIP_ESTATE, "nupc_get_limiter_true_peak: the detector is BFHIP_NUPC_LIMIT_SAMPLE_PEAK");
    *max_peak = 0.0;
    // nothing detected since the previous call (or ever): the meter on the device is stale or fresh
    if (!n->finalized || n->block == 0 || ((n->lim.tp_reset >> group) & 1u)) return BFHIP_OK;
    OWNER(n);
    NCHK(hipSetDevice(n->device));
    NCHK(hipStreamSynchronize(n->stream));
    // the parity the next block call reads
    const double *cell = n->lim.d_state + ((size_t)group * 2 + (n->block & 1)) * n->lim.state_stride() + 2 * n->lim.De() + 1;
    NCHK(hipMemcpy(max_peak, cell, sizeof(double), hipMemcpyDeviceToHost));
    n->lim.tp_reset |= 1u << group;                     // travels with the next block call
    return BFHIP_OK;
}

int bfhip_selftest_truepeak_filter(double g_out[]) {
    if (!g_out) return nfail(BFHIP_EINVAL, "selftest_truepeak_filter: bad argument");
    TruepeakTaps taps;
    truepeak_filter(&taps);
    memcpy(g_out, taps.g, sizeof(taps.g));
    return BFHIP_OK;
}

int bfhip_selftest_truepeak(long n, const double x[], double tp_out[]) {
    if (!truepeak_detect(n, x, tp_out)) return nfail(BFHIP_EINVAL, "selftest_truepeak: bad argument");
    return BFHIP_OK;
}

int bfhip_selftest_limiter_envelope(int lookahead_frames, double release_frames, long n, const double p[], double s_out[]) {
    if (!limiter_envelope(lookahead_frames, release_frames, n, p, s_out))
        return nfail(BFHIP_EINVAL, "selftest_limiter_envelope: bad argument");
    return BFHIP_OK;
}

// ---- BS.1770 loudness meter (checks, design, definition and read-outs: loudness_host.h) ------

static_assert(sizeof(bfhip_loudness) == sizeof(LoudnessReadout), "bfhip_loudness is LoudnessReadout");
static_assert(BFHIP_NUPC_LOUD_GROUPS_MAX == kLoudGroupsMax && BFHIP_NUPC_LOUD_GROUP_MAX == kLoudGroupMax, "loudness limits");

int bfhip_nupc_enable_loudness(bfhip_nupc *n, int sample_rate, int history_subblocks) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_enable_loudness after finalize");
    if (n->loud.on) return nfail(BFHIP_ESTATE, "nupc_enable_loudness: the meter is enabled already");
    std::string why;
    if (!loudness_check(sample_rate, history_subblocks, &why)) return nfail(BFHIP_EINVAL, "nupc_enable_loudness: " + why);
    n->loud.on = true;
    n->loud.rate = sample_rate;
    n->loud.S = sample_rate / 10;
    n->loud.history = history_subblocks;
    kweighting_design(sample_rate, n->loud.coef.c);
    return BFHIP_OK;
}

int bfhip_nupc_add_loudness_group(bfhip_nupc *n, const int out_channels[], const double weight[], int n_ch) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_add_loudness_group after finalize");
    if (!n->loud.on) return nfail(BFHIP_ESTATE, "nupc_add_loudness_group: needs bfhip_nupc_enable_loudness first");
    std::string why;
    if (!loudness_check_group(n->n_out, (int)n->loud.groups.size(), out_channels, weight, n_ch, &why))
        return nfail(BFHIP_EINVAL, "nupc_add_loudness_group: " + why);
    NupcLoudGroup g;
    memset(&g, 0, sizeof(g));
    g.n_ch = n_ch;
    for (int k = 0; k < n_ch; k++) { g.ch[k] = out_channels[k]; g.weight[k] = weight ? weight[k] : 1.0; g.scale[k] = 1.0; }
    n->loud.groups.push_back(g);
    n->loud.reset.push_back(0);
    return (int)n->loud.groups.size() - 1;
}

}  // extern "C"

namespace {

// what the three calls below share: the handle, the meter, the group
int loud_group_ok(const bfhip_nupc *n, int group, const char *who) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->loud.on) return nfail(BFHIP_ESTATE, std::string(who) + ": needs bfhip_nupc_enable_loudness before finalize");
    if (group < 0 || group >= (int)n->loud.groups.size()) return nfail(BFHIP_EINVAL, std::string(who) + ": bad group");
    return BFHIP_OK;
}

// waits for the main stream and downloads cells [lo, hi) of the group's ring, sub-block j into h_ring[j mod history]
int loud_download(bfhip_nupc *n, int group, long long lo, long long hi) {
    NupcLoudness &ld = n->loud;
    NCHK(hipSetDevice(n->device));
    NCHK(hipStreamSynchronize(n->stream));
    ld.h_ring.resize((size_t)ld.history);
    const double *ring = ld.d_ring + (size_t)group * ld.history;
    const long long H = ld.history, a = lo % H, cnt = hi - lo;
    const long long first = std::min(cnt, H - a);
    if (first > 0) NCHK(hipMemcpy(ld.h_ring.data() + a, ring + a, (size_t)first * sizeof(double), hipMemcpyDeviceToHost));
    if (cnt > first) NCHK(hipMemcpy(ld.h_ring.data(), ring, (size_t)(cnt - first) * sizeof(double), hipMemcpyDeviceToHost));
    return BFHIP_OK;
}

}  // namespace

extern "C" {

int bfhip_nupc_get_loudness(bfhip_nupc *n, int group, bfhip_loudness *out) {
    STEP(loud_group_ok(n, group, "nupc_get_loudness"));
    if (!out) return nfail(BFHIP_EINVAL, "nupc_get_loudness: bad argument");
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc_get_loudness before finalize");
    OWNER(n);
    NupcLoudness &ld = n->loud;
    const long long done = (long long)(n->block * (unsigned long long)n->L0() / (unsigned long long)ld.S);
    STEP(loud_download(n, group, std::max(0LL, done - ld.history), done));
    LoudnessReadout r;
    loudness_readout(ld.rate, done, ld.history, ld.reset[group],
                     [&](long long j) { return ld.h_ring[(size_t)(j % ld.history)]; }, &r);
    memcpy(out, &r, sizeof(r));
    return BFHIP_OK;
}

int bfhip_nupc_get_loudness_energy(bfhip_nupc *n, int group, long long first, int count, double E_out[]) {
    STEP(loud_group_ok(n, group, "nupc_get_loudness_energy"));
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc_get_loudness_energy before finalize");
    NupcLoudness &ld = n->loud;
    const long long done = (long long)(n->block * (unsigned long long)n->L0() / (unsigned long long)ld.S);
    if (first < 0 || count < 0 || (count > 0 && !E_out)) return nfail(BFHIP_EINVAL, "nupc_get_loudness_energy: bad argument");
    if (first + count > done)
        return nfail(BFHIP_EINVAL, "nupc_get_loudness_energy: sub-block " + std::to_string(first + count - 1) + " is not complete yet (" +
                     std::to_string(done) + " are)");
    if (first < done - ld.history)
        return nfail(BFHIP_EINVAL, "nupc_get_loudness_energy: sub-block " + std::to_string(first) + " has left the history ring of " +
                     std::to_string(ld.history));
    if (count == 0) return BFHIP_OK;
    OWNER(n);
    STEP(loud_download(n, group, first, first + count));
    for (int i = 0; i < count; i++) E_out[i] = ld.h_ring[(size_t)((first + i) % ld.history)];
    return BFHIP_OK;
}

// host bookkeeping only: the first sub-block whose first frame is at or behind the next block call's
int bfhip_nupc_reset_loudness(bfhip_nupc *n, int group) {
    STEP(loud_group_ok(n, group, "nupc_reset_loudness"));
    const unsigned long long frames = n->block * (unsigned long long)n->L0(), S = (unsigned long long)n->loud.S;
    n->loud.reset[group] = (long long)((frames + S - 1) / S);
    return BFHIP_OK;
}

int bfhip_selftest_kweighting(int sample_rate, double coef_out[10]) {
    std::string why;
    if (!coef_out) return nfail(BFHIP_EINVAL, "selftest_kweighting: bad argument");
    if (!loudness_rate_ok(sample_rate, &why)) return nfail(BFHIP_EINVAL, "selftest_kweighting: " + why);
    kweighting_design(sample_rate, coef_out);
    return BFHIP_OK;
}

int bfhip_selftest_loudness_energy(int sample_rate, long n, const double v[], double E_out[]) {
    const long r = loudness_energy(sample_rate, n, v, E_out);
    if (r < 0) return nfail(BFHIP_EINVAL, "selftest_loudness_energy: bad argument");
    return (int)r;
}

int bfhip_selftest_loudness_gate(int sample_rate, long n_sub, const double E[], bfhip_loudness *out) {
    LoudnessReadout r;
    if (!loudness_gate(sample_rate, n_sub, E, out ? &r : nullptr)) return nfail(BFHIP_EINVAL, "selftest_loudness_gate: bad argument");
    memcpy(out, &r, sizeof(r));
    return BFHIP_OK;
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
