// nupc.h -- the non-uniform convolver's state, and what its two host units share: nupc.hip (the C ABI of
// include/bfhip_nupc.h but for the rewrites: create, finalize, the audio path, switches, gains, delays) and
// nupc_update.hip (set rewrites and equaliser renders).  The period schedule -- every decision that depends
// on the calls made only -- is nupc_sched.h, which has no HIP in it; the kernels and their launches are
// nupc_kernels.h, included by nupc.hip alone.  Internal: nothing here is part of include/.
#pragma once
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/bfhip_nupc.h"
#include "alloc.h"
#include "eq_apply.h"
#include "eq_minphase.h"
#include "eq_render.h"
#include "kernels.h"
#include "limiter_host.h"
#include "loudness_host.h"
#include "nupc_sched.h"
#include "truepeak_host.h"

using namespace bfhip;
using namespace nupc_sched;

// What the units share by name lives in this namespace: hidden, so that the dynamic symbols of the
// library stay those of the C ABI.
#define NUPC_HOST_NS namespace nupc_host __attribute__((visibility("hidden")))

NUPC_HOST_NS {

// one segment: a uniform partitioned convolver over taps [off, off + N L)
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
    unsigned long long due_block = 0;
    // the plan of the pending block: its rings, and the fade of a staggered switch, which by the time the
    // block is accumulated may have left busy with another one committed
    BlockPlan pending_plan;
    // coefficient switches (only allocated when some filter has more than one set)
    void *d_out2 = nullptr;     // [L][n_out]: the second assignment's output of a block run under both
    void *d_z = nullptr;        // spectra between the split-phase MAC and output calls
    std::vector<Asg> eng_set;   // per filter: the set and gain the engine's filter runs now
    std::vector<std::vector<int>> n_blocks;   // [filter][set]: partitions the set has in this engine
    hipEvent_t ev_upd = nullptr;   // background segment with a reservation: its share of a rewrite is done
};

// raw formats and layout of the period buffers, [0] in / [1] out, and their staging
struct NupcIo {
    std::vector<bfhip_format> fmt[2];
    size_t frame_bytes[2] = {0, 0};        // interleaved raw frame size (no meaning on a side with a declared buffer)
    // bfhip_nupc_set_buffer_bytes: > 0 = the side declared its period buffer, every channel laid out
    // on its own (planes, several devices).  Such an input side stages the period in d_stage, runs
    // delay and mute in place there and converts it into d_in_real: per-period planes are not
    // contiguous across periods, so no raw ring could give segment k its L_k consecutive frames.
    long buf_bytes[2] = {0, 0};
    size_t period_bytes[2] = {0, 0};       // bytes of one period buffer, whichever way it was declared
    bool in_real = false;                  // the segment engines read d_in_real (fixed at finalize)
    DevFormat *d_fmt[2] = {nullptr, nullptr};   // in: for the conversion kernel (in_real only); out: for the emit step
    uint8_t *h_in = nullptr, *h_out = nullptr;  // pinned staging of one period (bfhip_nupc_block)
};

// what the emit step reports: overflow structs, status bits and their hand-off to the host
struct NupcStatus {
    DevOverflow *d_over = nullptr, *h_over = nullptr;   // h_over pinned
    int *d_status = nullptr, *h_status = nullptr;       // h_status pinned
    unsigned int *d_arrive = nullptr;
};

// coefficient sets and switches (filters numbered in add_filter order; set j of filter f is engine
// coefficient coeff[f][j] in every segment engine)
struct NupcSets {
    std::vector<std::vector<int>> coeff;
    std::vector<double> out_scale;         // per filter: add_filter's, multiplied by the assignment's gain
    bool gain_reserve = false;             // bfhip_nupc_reserve_filter_gain: gain-only switches need the spare ring
    bool can_switch = false;               // some filter has a second set, or gain_reserve: the spare ring exists
    Switcher sched;
};

// output gain: a block call that finds a request other than its record's target starts a ramp (or steps)
struct NupcOutGain {
    GainMirror mirror;
    NupcGain *d = nullptr;                 // [n_out]: 1/scale, output gain and its ramp (the emit step advances it)
    NupcGain *h = nullptr;                 // pinned staging of the records
    hipEvent_t ev = nullptr;               // the last upload out of h has been done
};

// HP-TPDF dither (dither.c; bfhip_nupc_enable_dither): one slot per dithered output, in ascending
// channel order; the table walk advances L0 per block call
struct NupcDither {
    std::vector<int> ch;                   // output channel of each slot
    std::vector<int8_t> table;
    int spacing = 0;
    int *d_slot = nullptr;                 // [n_out]: slot of the channel, -1 = not dithered
    void *d_state = nullptr;               // [n_dither] DitherState
    int8_t *d_table = nullptr;
    void *d_randmap = nullptr;             // 512 reals
    void *d_stage = nullptr;               // [n_dither][L0] reals: the emit step's input to the chain
};

// sub-sample delay (bfhip_nupc_enable_subdelay / _set_subdelay)
struct NupcSubdelay {
    int sdf_length = 0, flen = 0, bs = 0;
    std::vector<int> val[2];               // [io][channel], hundredths of a sample, -100 = the channel has no filter
    bool use[2] = {false, false};          // the side has a filter (fixed at finalize)
    void *d_bank = nullptr;                // [199][flen] reals
    void *d_hist[2] = {nullptr, nullptr};  // [channels][bs] reals: unfiltered history
};

// asynchronous set rewrite (bfhip_nupc_reserve_update / _update_coeff_async): everything is
// allocated at finalize; one rewrite in flight at a time.  A rewrite is a group of members, each a set of
// a filter of its own (bfhip_nupc_render_eq_group_async); every single call is a group of one.
struct UpdMember {
    int filter = -1, set = -1;
    const uint8_t *src = nullptr;          // the member's taps: host (member 0 of a single call only) or device
    long n_taps = 0;
    int result = BFHIP_OK;                 // of the last completed rewrite
};

struct NupcUpdate {
    bool reserve = false;                  // asked for before finalize
    uint8_t *h_taps = nullptr;             // pinned staging: taps() reals (bfhip_nupc_update_buffer)
    uint8_t *d_taps = nullptr;             // device staging of member 0: the segment engines prepare out of their slices
    hipStream_t stream = nullptr;          // loader: low priority, uploads the background segments' slices
    hipEvent_t ev_load = nullptr;          // the loader's upload is done
    hipEvent_t ev_main = nullptr;          // the main-stream segments' share is done
    int *h_bad = nullptr;                  // pinned, one word per segment: the engine's non-finite flag for member 0
    int *h_bad_group = nullptr;            // pinned, [member - 1][segment]: the same for the members behind it
    bool inflight = false;
    bool failed = false;                   // enqueuing it failed part-way: the sets' contents are unknown
    int n_members = 0;                     // of the rewrite in flight / completed last
    UpdMember mem[kEqGroupMax];
    int result = BFHIP_OK;                 // result of the last completed rewrite: BFHIP_OK iff every member's is
    std::vector<std::vector<char>> bad;    // [filter][set]: the last rewrite ended non-finite

    bool rewrites(int filter, int set) const {
        for (int m = 0; m < n_members; m++) if (mem[m].filter == filter && mem[m].set == set) return true;
        return false;
    }
};

// equaliser render (bfhip_nupc_reserve_eq / _render_eq_async, eq_render.h): a producer in front of
// the rewrite, on the loader stream; everything is allocated at finalize
struct NupcEq {
    long reserve = 0;                      // max_taps asked for before finalize, 0 = none
    EqRender lin;
    EqMinphase min;                        // bfhip_nupc_reserve_eq_minimum (eq_minphase.h)
    // render onto a base (bfhip_nupc_reserve_eq_base, eq_apply.h): one more producer step behind the render
    EqApply app;
    std::vector<char> base_want;           // [filter]: reserved before finalize
    std::vector<std::vector<unsigned char>> taps0;   // [filter]: add_filter's taps until finalize, the initial base
    hipEvent_t ev = nullptr;               // the render into lin.taps is done
    int group = 0;                         // bfhip_nupc_reserve_eq_group's max_members, 0 = none
};

// look-ahead peak limiter on the outputs (bfhip_nupc_enable_limiter).  Nothing of it exists in a convolver
// that never enables it.  All of its state lives on the device and never crosses to the host per period.
struct NupcLimGroup {                      // one row of the group table, host and device
    int n_ch, pad;
    int ch[kLimGroupMax];
    double scale[kLimGroupMax];            // the members' fmt.scale (filled at finalize)
};
struct NupcLimThr { double v[kLimGroupsMax]; };     // this period's thresholds: a kernel argument
struct NupcLimiter {
    bool on = false;
    int D = 0;                             // look-ahead in frames
    double release = 0, a = 0;             // release_frames and exp(-1 / release_frames)
    std::vector<NupcLimGroup> groups;
    std::vector<double> thr;               // per group: in force from the next block call
    std::vector<int> group_of;             // [n_out]: the channel's group, -1 = none
    unsigned int meter_reset = 0;          // bit g: the next block call starts group g's meter afresh
    void *d_ring = nullptr;                // [n_out][D + L0] reals: x_c, frame t in cell t mod (D + L0)
    // [group][parity][2 D + 1] float64: the last D values of r, of e (e[t-1] is the last), and the meter's
    // running minimum.  Period k reads parity k & 1 and the group's first member writes the other one.
    // (True-peak detection: De in place of D and one more cell, see state_stride.)
    double *d_state = nullptr;
    NupcLimGroup *d_groups = nullptr;
    int *d_group_of = nullptr;             // [n_out]
    // true-peak detection (bfhip_nupc_set_limiter_detector): the envelope looks ahead De = D - H frames, and
    // the state keeps De values each of r and e, the meter's minimum and the true-peak meter's maximum
    int detector = kTpSamplePeak;
    TruepeakTaps taps = {};                // filled when true-peak mode is selected: a kernel argument
    unsigned int tp_reset = 0;             // bit g: the next block call starts group g's true-peak meter afresh
    bool true_peak() const { return detector == kTpTruePeak; }
    int De() const { return truepeak_envelope_lookahead(detector, D); }
    size_t state_stride() const { return (size_t)2 * De() + (true_peak() ? 2 : 1); }
};

// BS.1770 loudness meter on the emitted block (bfhip_nupc_enable_loudness).  Nothing of it exists in a convolver
// that never enables it.  The filter states, the open sub-block's partial sum and the ring of sub-block energies
// live on the device; the frame counter (block count x L0) and the reset points are the host's.
struct NupcLoudGroup {                     // one row of the group table, host and device
    int n_ch, pad;
    int ch[kLoudGroupMax];
    double weight[kLoudGroupMax];
    double scale[kLoudGroupMax];           // the members' fmt.scale (filled at finalize)
};
// the sections' coefficients and, for the chunked scan, the powers M^(2^i) of the transition matrix M over one
// chunk of zero input (kweighting_transition): a kernel argument
struct NupcLoudCoef { double c[10]; double mp[8][16]; };
struct NupcLoudness {
    bool on = false;
    int rate = 0, S = 0, history = 0;      // S = rate / 10 frames per sub-block
    int chunk = 0;                         // frames per lane (fixed at finalize): L0 = one lane walks the period
    std::vector<NupcLoudGroup> groups;
    std::vector<long long> reset;          // per group: the first sub-block the integrated value covers
    NupcLoudCoef coef = {};
    NupcLoudGroup *d_groups = nullptr;
    double *d_state = nullptr;             // [group][kLoudGroupMax][4]: shelf s1 s2, high-pass s1 s2 per member
    double *d_open = nullptr;              // [group]: the open sub-block's partial sum
    double *d_ring = nullptr;              // [group][history]: sub-block j in cell j mod history
    std::vector<double> h_ring;            // the read-outs' copy of one group's ring (not on the audio path)
};

}  // namespace nupc_host

using namespace nupc_host;

struct bfhip_nupc {
    int device = 0, rs = 4, n_in = 0, n_out = 0;
    pid_t owner = 0;                       // like an engine, it lives in the process that created it
    std::vector<Seg> seg;
    double safety_limit = 0;
    bool finalized = false, finalize_failed = false;
    bool background = true;
    unsigned long long block = 0;          // L0-blocks processed
    hipStream_t stream = nullptr;          // main stream: I/O, zero-slack segments, accumulate, emit
    hipEvent_t ev_in = nullptr;            // this period's frames are in the input ring
    // the rings
    int in_frames = 0;                     // input ring length: 2 * Lmax
    uint8_t *d_in = nullptr;               // raw input ring (not for an input side with a declared buffer)
    uint8_t *d_stage = nullptr;            // [buf_bytes[0]]: the staged period of such a side; its readers are all ordered on the main stream
    uint8_t *d_in_real = nullptr;          // [in_frames][n_in] reals: the ring the engines read instead of d_in
    int A = 0;                             // accumulator ring length in frames
    void *d_acc[2] = {nullptr, nullptr};   // [A][n_out] reals: the accumulator ring and the spare one of the switches
    uint8_t *d_rawout = nullptr;           // one period of raw output (bfhip_nupc_block)
    // one group per concern
    NupcIo io;
    NupcStatus st;
    NupcSets sets;
    NupcOutGain og;
    NupcDither dither;
    std::vector<NupcDelay> dl[2];          // integer delay and mute per raw channel: [io][channel]
    NupcSubdelay sd;
    NupcUpdate upd;
    NupcEq eq;
    NupcLimiter lim;
    NupcLoudness loud;

    int L0() const { return seg[0].L; }
    long taps() const { return seg.back().off + (long)seg.back().L * seg.back().N; }
    void *ring(int i) const { return d_acc[i]; }
    // this block's slot of the input ring, or the stage of a side with a declared buffer (no raw ring: the
    // period is staged, and only its reals are kept)
    size_t in_slot() const { return (size_t)(block * (unsigned long long)L0() % (unsigned long long)in_frames); }
    uint8_t *in_slot_raw() const { return io.buf_bytes[0] ? d_stage : d_in + in_slot() * io.frame_bytes[0]; }
};

NUPC_HOST_NS {

// sets the calling thread's error text (bfhip_nupc_last_error) and returns `code`; a runtime failure's
// sticky error is cleared (argument / state errors make no HIP call)  (nupc.hip)
int nfail(int code, const std::string &msg);

// nupc_update.hip: finalize's step (streams, events and buffers of the reservations; after the segments'),
// destroy's, and the poll of a rewrite in flight (never blocks)
int upd_finalize(bfhip_nupc *n, int prio_least);
void upd_release(bfhip_nupc *n);
int upd_poll(bfhip_nupc *n);

}  // namespace nupc_host

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
