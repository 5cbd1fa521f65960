// nupc_sched_driver.cpp -- drives the non-uniform convolver's period schedule (csrc/nupc_sched.h: the switch
// scheduler, the gain-ramp mirror, the delay machine) from a program of its own.  The header has no HIP in
// it, so g++ compiles this alone, plainly and with AddressSanitizer / UBSan.  Built and run by
// tests/test_nupc_sched.py, which writes a scenario of integers on stdin, reads what the schedule decided
// from stdout, and works out what it should have decided from frame ranges in Python.
//
//   frames  n_seg L.. N.. mode n t_req..                   -> per t_req: "t_sw t_0 .. t_{n_seg-1}"
//   walk    n_seg L.. N.. mode fade commit_period periods  -> per due block "B period k pos mode ring ring2 fade t_k",
//                                                             per period "E period two_rings rel0" (at the emit step)
//                                                             and "P period busy cur" (after end_period)
//   gain    n_ch L0 periods n_ev (period kind ch value)..  -> kind 0: set_output_gain(ch, value / 1000), kind 1:
//                                                             set_gain_ramp(value); per period and channel "G period ch
//                                                             done len"; the records a device would hold are advanced
//                                                             frame by frame and must stay equal to the mirror's
//   delay   F ss maxdelay init mute_first periods (req muted hex-of-the-block)..
//                                                          -> per period the block after the step, in hex: the
//                                                             jobs of NupcDelay::step applied to host memory by a
//                                                             serial model of nupc_delay_kernel
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "nupc_sched.h"

using namespace nupc_sched;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "nupc_sched_driver: %s failed (line %d)\n", #c, __LINE__); return 1; } } while (0)

static long long next_int() {
    long long v = 0;
    if (scanf("%lld", &v) != 1) { fprintf(stderr, "nupc_sched_driver: scenario ends early\n"); exit(2); }
    return v;
}

// a scheduler for the schedule on stdin, one filter with a request for set 1 queued
static Switcher read_switcher() {
    Switcher s;
    const int n_seg = (int)next_int();
    std::vector<int> L(n_seg), N(n_seg);
    for (int &v : L) v = (int)next_int();
    for (int &v : N) v = (int)next_int();
    long off = 0;
    for (int k = 0; k < n_seg; k++) { s.seg.push_back({L[k], off}); off += (long)L[k] * N[k]; }
    s.crossfade = L[0];
    s.add_filter();
    s.switch_mode = (int)next_int();
    return s;
}

static int frames() {
    const Switcher fresh = read_switcher();
    const int n = (int)next_int();
    for (int i = 0; i < n; i++) {
        Switcher s = fresh;
        CHECK(s.t_sw == -1 && s.segment_frame(0) == -1 && !s.busy() && !s.has_request());
        s.queued[0].set = 1;
        CHECK(s.has_request() && s.set_in_use(0, 1) && !s.set_in_use(0, 2));
        s.commit((unsigned long long)next_int());
        CHECK(!s.has_request() && s.live[0].set == 1 && s.sw_old[0].set == 0);
        printf("%lld", s.t_sw);
        for (size_t k = 0; k < s.seg.size(); k++) printf(" %lld", s.segment_frame((int)k));
        printf("\n");
    }
    return 0;
}

static int walk() {
    Switcher s = read_switcher();
    s.crossfade = (int)next_int();
    const int commit_period = (int)next_int(), periods = (int)next_int();
    const unsigned long long L0 = (unsigned long long)s.seg[0].L;
    for (int p = 0; p < periods; p++) {
        const unsigned long long opos = (unsigned long long)p * L0, end = opos + L0;
        if (p == commit_period) { CHECK(!s.busy()); s.queued[0].set = 1; }
        s.commit(opos);
        CHECK(s.old_asg()[0].set == (s.busy() ? 0 : s.live[0].set));
        for (size_t k = 0; k < s.seg.size(); k++) {
            if (end % (unsigned long long)s.seg[k].L) continue;
            const BlockPlan b = s.block(k, end);
            CHECK(b.F == s.sw_F);
            printf("B %d %zu %llu %d %d %d %d %lld\n", p, k, b.pos, b.mode, b.ring, b.ring2, b.fade ? 1 : 0, b.t_k);
        }
        printf("E %d %d %lld\n", p, s.two_rings() ? 1 : 0, s.rel0(opos));
        s.end_period(end);
        printf("P %d %d %d\n", p, s.busy() ? 1 : 0, s.cur);
    }
    return 0;
}

static int gain() {
    const int n_ch = (int)next_int(), L0 = (int)next_int(), periods = (int)next_int(), n_ev = (int)next_int();
    struct Ev { int period, kind, ch; long long value; };
    std::vector<Ev> ev(n_ev);
    for (Ev &e : ev) { e.period = (int)next_int(); e.kind = (int)next_int(); e.ch = (int)next_int(); e.value = next_int(); }
    GainMirror m;
    m.gain.assign(n_ch, 1.0);
    m.gain_len.assign(n_ch, 0);
    m.ramp.assign(n_ch, NupcGain{1.0, 1.0, 1.0, 0, 0});
    std::vector<NupcGain> dev = m.ramp;                            // what the device holds
    std::vector<double> last(n_ch, 1.0);                          // gain of the last emitted frame
    for (int p = 0; p < periods; p++) {
        for (const Ev &e : ev) {
            if (e.period != p) continue;
            if (e.kind == 0) m.request(e.ch, (double)e.value / 1000.0);
            else m.gain_ramp = (int)e.value;
        }
        const std::vector<NupcGain> before = m.ramp;
        if (m.start()) {
            for (int ch = 0; ch < n_ch; ch++) {
                const NupcGain &r = m.ramp[ch];
                if (r.g == before[ch].g) { CHECK(memcmp(&r, &before[ch], sizeof(r)) == 0); continue; }
                CHECK(r.done == 0 && r.g == m.gain[ch] && r.len == m.gain_len[ch]);
                CHECK(r.a == (r.len ? last[ch] : r.g));           // a ramp starts from the last emitted gain
            }
            dev = m.ramp;                                          // the upload
        } else
            CHECK(memcmp(m.ramp.data(), before.data(), before.size() * sizeof(NupcGain)) == 0);
        for (int ch = 0; ch < n_ch; ch++) {
            NupcGain &r = dev[ch];
            for (int n = 0; n < L0; n++) {                         // GainFactor::at, then one frame of gain_advance
                const int idx = r.done;
                last[ch] = idx < r.len - 1 ? r.a + (r.g - r.a) * ((double)(idx + 1) / (double)r.len) : r.g;
                if (r.done < r.len) r.done++;
            }
        }
        m.advance(L0);
        for (int ch = 0; ch < n_ch; ch++) {
            CHECK(m.ramp[ch].done == dev[ch].done && m.ramp[ch].len == dev[ch].len);
            CHECK(m.ramp[ch].a == dev[ch].a && m.ramp[ch].g == dev[ch].g);
            printf("G %d %d %d %d\n", p, ch, m.ramp[ch].done, m.ramp[ch].len);
        }
    }
    return 0;
}

// ---- a serial model of nupc_delay_kernel (csrc/nupc_kernels.h) on host memory: the zero-fills, the block
// into the scratch, the per-sample loop
static void job_apply(const NupcDelayJob &j, uint8_t *raw, int F, int mute_first) {
    uint8_t *buf = raw + j.byte_offset;
    const size_t ss = (size_t)j.ss, stride = (size_t)j.stride, fragp = (size_t)j.fragp;
    if (j.kind == 0) {
        for (int n = 0; n < F; n++) memset(buf + n * stride, 0, ss);
        return;
    }
    uint8_t *rest = j.line + (size_t)j.rest_frag * fragp, *sh0 = rest + fragp, *sh1 = sh0 + fragp, *tmp = sh1 + fragp;
    memset(j.line, 0, (size_t)j.zfull);
    memset(rest, 0, (size_t)j.zrest);
    memset(sh0, 0, (size_t)j.zshort);
    memset(sh1, 0, (size_t)j.zshort);
    const bool mute_in = mute_first && j.muted, mute_out = !mute_first && j.muted;
    for (int n = 0; n < F; n++) {
        if (mute_in) memset(tmp + n * ss, 0, ss);
        else memcpy(tmp + n * ss, buf + n * stride, ss);
    }
    const int rr = j.rr;
    std::vector<uint8_t> y(ss);
    for (int n = 0; n < F; n++) {
        if (j.kind == 1) {
            uint8_t *fcur = j.line + (size_t)j.cur * fragp;
            const uint8_t *last = j.line + (size_t)j.last * fragp;
            memcpy(fcur + n * ss, tmp + n * ss, ss);
            if (n < rr) {
                memcpy(y.data(), rest + n * ss, ss);
                memcpy(rest + n * ss, last + (size_t)(F - rr + n) * ss, ss);
            } else
                memcpy(y.data(), last + (size_t)(n - rr) * ss, ss);
        } else {
            uint8_t *shw = j.cur ? sh1 : sh0;
            const uint8_t *shr = j.last ? sh1 : sh0;
            memcpy(y.data(), n < rr ? shr + n * ss : tmp + (size_t)(n - rr) * ss, ss);
            if (n < rr) memcpy(shw + n * ss, tmp + (size_t)(F - rr + n) * ss, ss);
        }
        if (mute_out) memset(buf + n * stride, 0, ss);
        else memcpy(buf + n * stride, y.data(), ss);
    }
}

static int delay() {
    const int F = (int)next_int(), ss = (int)next_int();
    NupcDelay d;
    d.maxdelay = (int)next_int();
    d.req = (int)next_int();
    const int mute_first = (int)next_int(), periods = (int)next_int();
    const size_t bytes = d.init(F, ss);
    std::vector<uint8_t> arena(bytes, 0);                          // exactly what init asks for: the sanitizer watches the rest
    if (bytes) d.arena = arena.data();
    std::vector<uint8_t> raw((size_t)F * ss);
    std::vector<char> hex(2 * raw.size() + 1);
    for (int p = 0; p < periods; p++) {
        d.req = (int)next_int();
        d.muted = next_int() != 0;
        CHECK(scanf("%s", hex.data()) == 1 && strlen(hex.data()) == 2 * raw.size());
        for (size_t i = 0; i < raw.size(); i++) { unsigned v = 0; CHECK(sscanf(hex.data() + 2 * i, "%2x", &v) == 1); raw[i] = (uint8_t)v; }
        NupcDelayJob jb;
        if (d.step(jb)) {
            jb.byte_offset = 0; jb.ss = ss; jb.stride = ss;        // one channel, its samples back to back
            CHECK(jb.kind == 0 || (size_t)(jb.rest_frag + 4) * jb.fragp == bytes);
            job_apply(jb, raw.data(), F, mute_first);
        }
        for (uint8_t v : raw) printf("%02x", v);
        printf(" %d\n", d.curdelay);
    }
    return 0;
}

int main(int argc, char **argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    const int r = cmd == "frames" ? frames() : cmd == "walk" ? walk() : cmd == "gain" ? gain() : cmd == "delay" ? delay() : 2;
    if (r == 0) printf("nupc_sched_driver: clean\n");
    return r;
}
