// nupc_sched.h -- the period schedule of the non-uniform convolver (nupc.hip): the state and arithmetic
// that depend on the calls made only, never on samples or streams.  Which assignment a segment block runs
// under and which ring it goes to, when a switch is over and the rings flip, where a gain ramp stands, which
// step a channel's delay line takes.  No HIP: g++ compiles this header on its own, and
// tests/chost/nupc_sched_driver.cpp drives it on the CPU.  Hidden, like engine.h's namespace: the dynamic
// symbols of the library stay those of the C ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/bfhip_nupc.h"

namespace nupc_sched __attribute__((visibility("hidden"))) {

// what a filter runs under: an assignment is one of these per filter.  gain multiplies the filter's
// out_scale; `set` < 0 / a NaN gain in a queued request mean "not asked for"
struct Asg {
    int set = 0;
    double gain = 1.0;
    bool operator==(const Asg &o) const { return set == o.set && gain == o.gain; }
};

// ---- coefficient switches
//
// An aligned switch (the default) has one switch frame t_sw for all segments: the old assignment's output
// goes on into the live ring, the new one's into the spare ring, the emit step blends the two over
// [t_sw, t_sw + F), and when nothing old is left the rings flip.  A staggered switch
// (BFHIP_NUPC_SWITCH_STAGGERED) gives segment k its own frame t_k and blends per segment block into the
// live ring: the spare ring and `cur` play no part.

// what the block of one segment that is due in a period runs as
struct BlockPlan {
    unsigned long long pos = 0;    // first frame it writes: end - L + off
    int mode = 1;                  // assignment: 0 old, 1 new (the live one), 2 both
    int ring = 0, ring2 = -1;      // ring of its (first) output, ring of the second output of an aligned mode 2
    bool fade = false;             // staggered mode 2: blended by the accumulate step
    long long t_k = 0;             // its segment's switch frame
    int F = 0;                     // fade length of the switch
};

struct Switcher {
    struct Shape { int L; long off; };
    std::vector<Shape> seg;                // partition length and first tap of every segment; seg[0].L = L0
    std::vector<Asg> live;                 // per filter: the newest committed assignment
    std::vector<Asg> queued;               // per filter: requested set (-1 = none) and gain (NaN = none)
    std::vector<Asg> sw_old;               // the old assignment of the last switch (the new one is `live`)
    int crossfade = 0;                     // frames for the next switch (default L0)
    int switch_mode = BFHIP_NUPC_SWITCH_ALIGNED;   // for the switches committed from now on
    int cur = 0;                           // ring of the live assignment
    bool sw = false;                       // a committed switch has old-assignment work or fade frames left
    bool sw_stag = false;                  // the switch in flight (sw) is a staggered one
    long long t_sw = -1;                   // its switch frame, staggered: its t_req (-1: none committed yet)
    int sw_F = 0;                          // its fade length
    long long old_hi = 0;                  // aligned: end of the frames the old assignment has written
    std::vector<long long> t_seg;          // per segment: switch frame of the last committed switch

    void add_filter() { live.push_back(Asg()); queued.push_back(Asg{-1, NAN}); }
    bool busy() const { return sw; }
    bool has_request() const {
        for (const Asg &q : queued) if (q.set >= 0 || !std::isnan(q.gain)) return true;
        return false;
    }
    // is the set live, asked for, or the old side of the switch in flight?
    bool set_in_use(int filter, int set) const {
        return set == live[filter].set || set == queued[filter].set || (sw && set == sw_old[filter].set);
    }
    // the assignment mode 0 stands for
    const std::vector<Asg> &old_asg() const { return sw ? sw_old : live; }
    long long segment_frame(int k) const { return t_seg.empty() ? -1 : t_seg[k]; }

    // segment k's first block launched by the block call that emits from t_req on, or a later one, writes
    // frames from here on: e_k - L_k + off_k >= t_req (off_k >= L_k - L0), e_k the first multiple of L_k
    // >= t_req + L0
    long long next_frame(size_t k, unsigned long long t_req) const {
        const unsigned long long L = (unsigned long long)seg[k].L, L0 = (unsigned long long)seg[0].L;
        const unsigned long long e = (t_req + L0 + L - 1) / L * L;
        return (long long)(e - L) + seg[k].off;
    }

    // start of the period whose first output frame is t_req: with no switch in flight, the queued requests
    // become one switch whose first output block is this one
    void commit(unsigned long long t_req) {
        if (sw) return;
        std::vector<Asg> asg = live;
        for (size_t f = 0; f < asg.size(); f++) {
            if (queued[f].set >= 0) asg[f].set = queued[f].set;
            if (!std::isnan(queued[f].gain)) asg[f].gain = queued[f].gain;
        }
        std::fill(queued.begin(), queued.end(), Asg{-1, NAN});
        if (asg == live) return;                                  // nothing changes
        t_seg.resize(seg.size());
        sw_old = live;
        live = asg;
        sw_F = crossfade;
        sw_stag = switch_mode == BFHIP_NUPC_SWITCH_STAGGERED;
        if (sw_stag) {
            // segment k switches at the first frame its next launch writes, t_0 = t_req.  A hard switch needs
            // no block under both assignments: every segment simply runs the new one from its next launch
            // on, and there is nothing to be busy with.
            for (size_t k = 0; k < seg.size(); k++) t_seg[k] = next_frame(k, t_req);
            t_sw = (long long)t_req;
            sw = sw_F > 0;
            return;
        }
        t_sw = (long long)t_req;
        for (size_t k = 0; k < seg.size(); k++) t_sw = std::max(t_sw, next_frame(k, t_req));
        sw = true;
        old_hi = t_sw;             // what was launched before wrote frames < t_sw only
        std::fill(t_seg.begin(), t_seg.end(), t_sw);
    }

    // segment k's block in the period that has received `end` frames (L_k divides end): which assignment(s)
    // its frames [pos, pos + L) need, and into which ring
    BlockPlan block(size_t k, unsigned long long end) {
        BlockPlan b;
        const long long L = seg[k].L;
        b.pos = end - (unsigned long long)L + (unsigned long long)seg[k].off;
        b.ring = cur;
        b.t_k = t_seg.empty() ? 0 : t_seg[k];
        b.F = sw_F;
        const long long pos = (long long)b.pos;
        if (sw && sw_stag) {
            // the segment's own switch frame decides; everything goes into the live ring
            b.fade = pos < b.t_k + sw_F && pos + L > b.t_k;
            b.mode = b.fade ? 2 : 1;
        } else if (sw) {
            const bool need_old = pos < t_sw + sw_F, need_new = pos + L > t_sw;
            b.mode = need_old && need_new ? 2 : need_old ? 0 : 1;
            if (b.mode == 1) b.ring = 1 - cur;
            if (b.mode == 2) b.ring2 = 1 - cur;
            if (need_old) old_hi = std::max(old_hi, pos + L);
        }
        return b;
    }

    // the emit step of the period: inside an aligned switch the old assignment's ring (cur) is read beside
    // the new one's; a staggered switch has blended its fades into the live ring already
    bool two_rings() const { return sw && !sw_stag; }
    long long rel0(unsigned long long opos) const { return two_rings() ? (long long)opos - t_sw : 0; }

    // after the period that received (and emitted up to) `end` frames: the switch is over once no later
    // block can need the old assignment; an aligned one then leaves its old ring, emitted and cleared down
    // to its last written frame, as the spare
    void end_period(unsigned long long end) {
        if (!sw || work_left(end)) return;
        sw = false;
        if (!sw_stag) cur = 1 - cur;
    }

  private:
    bool work_left(unsigned long long end) const {
        if (sw_stag) {
            // does some segment's next block start before the segment's own fade ends?
            for (size_t k = 0; k < seg.size(); k++) {
                const unsigned long long L = (unsigned long long)seg[k].L;
                if ((long long)(end / L * L) + seg[k].off < t_seg[k] + sw_F) return true;
            }
            return false;
        }
        const long long old_end = t_sw + sw_F;                    // old output is needed below this frame
        if ((long long)end < std::max(old_hi, old_end)) return true;
        for (const Shape &s : seg) {
            const unsigned long long L = (unsigned long long)s.L;
            if ((long long)(end / L * L) + s.off < old_end) return true;
        }
        return false;
    }
};

// ---- output gain
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

// the host's mirror of the records: they are a pure function of the calls
struct GainMirror {
    std::vector<double> gain;              // per output: the value asked for last
    std::vector<int> gain_len;             // the ramp length in force at that call
    std::vector<NupcGain> ramp;            // the device records
    int gain_ramp = 0;                     // bfhip_nupc_set_gain_ramp: for the requests from now on
    bool dirty = false;

    void request(int ch, double g) {
        if (gain[ch] != g) { gain[ch] = g; gain_len[ch] = gain_ramp; dirty = true; }
    }
    // start of a period: a channel whose request differs from its record's target starts a step or ramp
    // whose first frame is this period's first, from the gain of the last emitted frame.  true: some record
    // changed, and every record goes up as the mirror has it (where the other channels' ramps are now)
    bool start() {
        if (!dirty) return false;
        dirty = false;
        bool changed = false;
        for (size_t ch = 0; ch < ramp.size(); ch++) {
            NupcGain &r = ramp[ch];
            if (gain[ch] == r.g) continue;
            const double prev = r.done >= r.len ? r.g : r.a + (r.g - r.a) * ((double)r.done / (double)r.len);
            r.a = gain_len[ch] ? prev : gain[ch];
            r.g = gain[ch]; r.done = 0; r.len = gain_len[ch];
            changed = true;
        }
        return changed;
    }
    // a period of L0 frames has been emitted (gain_advance's mirror)
    void advance(int L0) {
        for (NupcGain &r : ramp) if (r.done < r.len) r.done = r.len - r.done < L0 ? r.len : r.done + L0;
    }
};

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

}  // namespace nupc_sched
