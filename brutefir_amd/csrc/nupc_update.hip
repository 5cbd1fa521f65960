// nupc_update.hip -- the non-uniform convolver's set rewrites (synchronous and asynchronous) and its
// equaliser renders (include/bfhip_nupc.h; state in nupc.h).  None of this is on the audio path and none of
// it launches a kernel of nupc_kernels.h: a rewrite uploads the taps and has every segment engine prepare
// its slice on the engine's own stream, in order with the segment's blocks; a render (eq_render.h,
// eq_minphase.h, eq_biquad.h, and eq_apply.h where it goes onto a base) is a producer in front of a rewrite, on the loader
// stream.  Which sets may be rewritten is the switch schedule's answer (Switcher::set_in_use).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "coeff_async.h"
#include "eq_biquad.h"
#include "nupc.h"

namespace {

bool set_ok(const bfhip_nupc *n, int filter, int coeff) {
    return filter >= 0 && filter < (int)n->sets.coeff.size() && coeff >= 0 && coeff < (int)n->sets.coeff[filter].size();
}

// set 0 keeps the partitions add_filter gave it: do these taps reach past them?  Host taps may, with
// zeros; a device source cannot be looked at without a wait: it must not reach past them at all
bool past_set(const bfhip_nupc *n, int filter, int coeff, const void *taps, bool on_device, long n_taps) {
    for (const Seg &s : n->seg) {
        const long covered = s.off + (long)s.n_blocks[filter][coeff] * s.L;
        const long from = std::min(covered, n_taps), to = std::min(s.off + (long)s.L * s.N, n_taps);
        if (on_device && from < to) return true;
        for (long i = from; i < to && !on_device; i++)
            if (n->rs == 4 ? ((const float *)taps)[i] != 0.0f : ((const double *)taps)[i] != 0.0) return true;
    }
    return false;
}

// a render on the loader stream: the curve -- bands in `mode`, or sections in `phase` (eq_biquad.h) -- into
// eq.lin.taps[0 .. taps), and with n_base > 0 the bases of those filters convolved with them into
// eq.app.ys[0 .. n_base) (eq_apply.h)
struct EqJob {
    bool sections = false;
    EqBands b;
    EqBiquads q;
    long taps = 0;
    int mode = BFHIP_EQ_LINEAR;
    int phase = BFHIP_BIQUAD_OWN;
    int n_base = 0;
    int base[kEqGroupMax] = {};
};

hipError_t eq_launch(const bfhip_nupc *n, const EqJob &j) {
    const hipStream_t st = n->upd.stream;
    hipError_t err;
    if (j.sections)
        err = n->rs == 4 ? eq_biquad_launch<float>(n->eq.lin, j.q, j.phase, j.taps, st)
                         : eq_biquad_launch<double>(n->eq.lin, j.q, j.phase, j.taps, st);
    else if (j.mode == BFHIP_EQ_MINIMUM)
        err = n->rs == 4 ? eq_minphase_launch<float>(n->eq.lin, n->eq.min, j.b, j.taps, st)
                         : eq_minphase_launch<double>(n->eq.lin, n->eq.min, j.b, j.taps, st);
    else
        err = n->rs == 4 ? eq_render_launch<float>(n->eq.lin, j.b, j.taps, st)
                         : eq_render_launch<double>(n->eq.lin, j.b, j.taps, st);
    if (err != hipSuccess || j.n_base == 0) return err;
    const void *base[kEqGroupMax];
    for (int i = 0; i < j.n_base; i++) base[i] = n->eq.app.base[j.base[i]];
    return n->rs == 4 ? eq_apply_launch<float>(n->eq.app, n->eq.lin, j.n_base, base, n->eq.app.ys, j.taps, st)
                      : eq_apply_launch<double>(n->eq.app, n->eq.lin, j.n_base, base, n->eq.app.ys, j.taps, st);
}

// the pinned word that segment k's engine writes its non-finite flag of member m to
int *bad_word(const NupcUpdate &u, int m, size_t k, size_t n_seg) {
    return m == 0 ? u.h_bad + k : u.h_bad_group + (size_t)(m - 1) * n_seg + k;
}

// enqueue the upload and every segment engine's preparation of the members of u.mem; no host wait, no
// allocation.  Member 0 goes through the staging buffers as every single rewrite does: a host source out of
// the pinned one, a device source behind ready_event, which the loader (and the main stream, for its own
// slices) waits on.  The members behind it are device arrays of the convolver's own that nothing writes
// while the group is in flight (eq.lin.taps, eq.app.ys): the engines prepare straight out of them.
int upd_enqueue(bfhip_nupc *n, bool on_device, void *ready_event) {
    NupcUpdate &u = n->upd;
    const size_t rs = (size_t)n->rs;
    const uint8_t *src = u.mem[0].src;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    bool main_waits = false;
    if (on_device && ready_event) NCHK(hipStreamWaitEvent(u.stream, (hipEvent_t)ready_event, 0));
    // upload: a segment that runs on the main stream gets its own slice there (the high-priority
    // stream never waits for the whole upload); the rest goes through the loader, adjacent slices
    // in one copy
    long run_from = -1, run_to = -1;
    auto flush = [&]() -> hipError_t {
        if (run_from < 0 || run_to <= run_from) { run_from = run_to = -1; return hipSuccess; }
        const hipError_t e = hipMemcpyAsync(u.d_taps + (size_t)run_from * rs, src + (size_t)run_from * rs,
                                            (size_t)(run_to - run_from) * rs, kind, u.stream);
        run_from = run_to = -1;
        return e;
    };
    for (int m = 0; m < u.n_members; m++) {
        for (const Seg &s : n->seg) {
            const long from = s.off, to = std::min(s.off + (long)s.L * s.N, u.mem[m].n_taps);
            if (to <= from) continue;
            if (s.delay_steps > 0) {
                if (m > 0) continue;
                if (run_to != from) { NCHK(flush()); run_from = from; }
                run_to = to;
                continue;
            }
            // the main stream waits only where one of its own segments reads a member's taps
            if (on_device && ready_event && !main_waits) { NCHK(hipStreamWaitEvent(n->stream, (hipEvent_t)ready_event, 0)); main_waits = true; }
            if (m == 0) NCHK(hipMemcpyAsync(u.d_taps + (size_t)from * rs, src + (size_t)from * rs, (size_t)(to - from) * rs, kind, n->stream));
        }
        if (m == 0) NCHK(flush());
    }
    NCHK(hipEventRecord(u.ev_load, u.stream));
    // preparation: one launch per segment engine and member on the engine's own stream, in order with its blocks
    for (size_t k = 0; k < n->seg.size(); k++) {
        Seg &s = n->seg[k];
        const long cap = (long)s.L * s.N;
        if (s.delay_steps > 0) NCHK(hipStreamWaitEvent(s.stream, u.ev_load, 0));
        for (int m = 0; m < u.n_members; m++) {
            const UpdMember &mb = u.mem[m];
            const long left = std::max(0L, std::min(mb.n_taps - s.off, cap));
            const uint8_t *from = m == 0 ? u.d_taps + (size_t)s.off * rs : left > 0 ? mb.src + (size_t)s.off * rs : mb.src;
            ECHK(bfhip_internal_engine_update_coeff_dev_async(s.eng, n->sets.coeff[mb.filter][mb.set], from, (int)left,
                                                              s.n_blocks[mb.filter][mb.set], bad_word(u, m, k, n->seg.size())));
        }
        if (s.delay_steps > 0) NCHK(hipEventRecord(s.ev_upd, s.stream));
    }
    NCHK(hipEventRecord(u.ev_main, n->stream));
    return BFHIP_OK;
}

// every check has passed: the rewrite of n_members sets begins.  eq: the taps are produced by this render on
// the loader stream first, and eq.ev is the ready event (the members' sources are eq.lin.taps / eq.app.ys).
int upd_go(bfhip_nupc *n, int n_members, const UpdMember mem[], bool on_device, void *ready_event, const EqJob *eq) {
    NupcUpdate &u = n->upd;
    NCHK(hipSetDevice(n->device));
    if (eq) {
        // a failure here has touched eq.lin.taps and eq.app.ys only: the sets are as they were
        NCHK(eq_launch(n, *eq));
        NCHK(hipEventRecord(n->eq.ev, u.stream));
        ready_event = n->eq.ev;
    }
    // from here on work may be enqueued: a failure leaves the sets' contents unknown
    u.inflight = true;
    u.n_members = n_members;
    for (int m = 0; m < n_members; m++) {
        u.mem[m] = mem[m];
        u.bad[mem[m].filter][mem[m].set] = 1;
    }
    u.failed = false;
    const int r = upd_enqueue(n, on_device, ready_event);
    if (r < 0) u.failed = true;
    return r;
}

// the checks of a single asynchronous rewrite, then upd_go with a group of one.  Host source: `taps` is the
// pinned staging buffer or is copied into it.  eq: the caller passes taps = eq.lin.taps or eq.app.y, on_device.
int upd_start(bfhip_nupc *n, int filter, int coeff, const void *taps, bool on_device, long n_taps, void *ready_event,
              const EqJob *eq = nullptr) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!set_ok(n, filter, coeff) || !taps || n_taps < 1 || n_taps > n->taps())
        return nfail(BFHIP_EINVAL, "nupc_update_coeff_async: bad argument");
    NupcUpdate &u = n->upd;
    if (!n->finalized || !u.reserve)
        return nfail(BFHIP_ESTATE, "nupc_update_coeff_async: needs bfhip_nupc_reserve_update before finalize, and finalize");
    if (n->sets.sched.set_in_use(filter, coeff))
        return nfail(BFHIP_ESTATE, "nupc_update_coeff_async: the set is live or part of a queued / in-flight switch");
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (u.inflight) return nfail(BFHIP_ESTATE, "nupc_update_coeff_async: a rewrite is in flight (bfhip_nupc_update_busy)");
    if (past_set(n, filter, coeff, taps, on_device, n_taps))
        return nfail(BFHIP_EINVAL, "nupc_update_coeff_async: set 0 of this filter is shorter than these taps (add_filter's length)");
    if (!on_device && taps != (const void *)u.h_taps) memcpy(u.h_taps, taps, (size_t)n_taps * n->rs);
    UpdMember one;
    one.filter = filter; one.set = coeff; one.n_taps = n_taps;
    one.src = on_device ? (const uint8_t *)taps : u.h_taps;
    return upd_go(n, 1, &one, on_device, ready_event, eq);
}

// a render onto a base: the filter's reservation and the limit on eq_taps in force
int eq_base_check(const bfhip_nupc *n, int base, long taps) {
    if (base >= (int)n->eq.app.base.size() || !n->eq.app.base[base])
        return nfail(base >= (int)n->sets.coeff.size() ? BFHIP_EINVAL : BFHIP_ESTATE,
                     "nupc_render_eq_base: needs bfhip_nupc_reserve_eq_base for this filter before finalize");
    const bool pow2 = taps >= 8 && !(taps & (taps - 1));
    if (n->eq.app.reserved_long && (!pow2 || taps > n->eq.reserve))
        return nfail(BFHIP_EINVAL, "nupc_render_eq_base: eq_taps must be a power of two, 8 .. max_taps = " + std::to_string(n->eq.reserve));
    if (!n->eq.app.reserved_long && (!pow2 || taps > std::min(n->eq.reserve, 1L << kEqApplyMaxLog2B)))
        return nfail(BFHIP_EINVAL, "nupc_render_eq_base: eq_taps must be a power of two, 8 .. min(max_taps, 8192)");
    return BFHIP_OK;
}

// state and curve checks shared by the render calls; fills the kernel-argument copy of the bands
int eq_check(const bfhip_nupc *n, long taps, int n_bands, const double freq[], const double mag[],
             const double phase[], int mode, EqJob *j, int base = -1) {
    EqBands *b = &j->b;
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->eq.reserve)
        return nfail(BFHIP_ESTATE, "nupc_render_eq: needs bfhip_nupc_reserve_eq before finalize, and finalize");
    if (mode != BFHIP_EQ_LINEAR && mode != BFHIP_EQ_MINIMUM)
        return nfail(BFHIP_EINVAL, "nupc_render_eq: mode must be BFHIP_EQ_LINEAR or BFHIP_EQ_MINIMUM");
    if (mode == BFHIP_EQ_MINIMUM && !n->eq.min.reserved)
        return nfail(BFHIP_ESTATE, "nupc_render_eq: minimum phase needs bfhip_nupc_reserve_eq_minimum before finalize");
    if (base >= 0) { const int r = eq_base_check(n, base, taps); if (r < 0) return r; }
    if (taps < 8 || (taps & (taps - 1)) || taps > n->eq.reserve)
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
    j->taps = taps; j->mode = mode;
    j->n_base = base >= 0 ? 1 : 0;
    j->base[0] = base;
    return BFHIP_OK;
}

// the same for a cascade of sections (biquad_host.h has the section rules); fills the kernel-argument copy
int bq_check(const bfhip_nupc *n, long taps, int n_sections, const double coef[], int phase_mode, EqJob *j, int base = -1) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->eq.reserve)
        return nfail(BFHIP_ESTATE, "nupc_render_biquads: needs bfhip_nupc_reserve_eq before finalize, and finalize");
    if (phase_mode != BFHIP_BIQUAD_OWN && phase_mode != BFHIP_BIQUAD_LINEAR)
        return nfail(BFHIP_EINVAL, "nupc_render_biquads: phase_mode must be BFHIP_BIQUAD_OWN or BFHIP_BIQUAD_LINEAR");
    if (base >= 0) { const int r = eq_base_check(n, base, taps); if (r < 0) return r; }
    if (taps < 8 || (taps & (taps - 1)) || taps > n->eq.reserve)
        return nfail(BFHIP_EINVAL, "nupc_render_biquads: taps must be a power of two, 8 .. max_taps");
    std::string why;
    if (!biquad_check(n_sections, coef, &j->q, &why)) return nfail(BFHIP_EINVAL, "nupc_render_biquads: " + why);
    j->sections = true;
    j->taps = taps; j->phase = phase_mode;
    j->n_base = base >= 0 ? 1 : 0;
    j->base[0] = base;
    return BFHIP_OK;
}

// a synchronous render alone: the job's taps (or, onto a base, its y) into host memory
int eq_render_sync(bfhip_nupc *n, const EqJob &j, const char *who, void *taps_out) {
    if (!taps_out) return nfail(BFHIP_EINVAL, std::string(who) + ": null buffer");
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (n->upd.inflight) return nfail(BFHIP_ESTATE, std::string(who) + ": a rewrite is in flight (bfhip_nupc_update_busy)");
    NCHK(hipSetDevice(n->device));
    NCHK(eq_launch(n, j));
    const void *from = j.n_base ? n->eq.app.y : n->eq.lin.taps;
    const size_t bytes = (size_t)(j.n_base ? n->taps() : j.taps) * n->rs;
    NCHK(hipMemcpyAsync(taps_out, from, bytes, hipMemcpyDeviceToHost, n->upd.stream));
    NCHK(hipStreamSynchronize(n->upd.stream));
    return BFHIP_OK;
}

// a group render behind its curve check (j holds bands or sections): every member is checked before
// anything is enqueued; the message names the member
int eq_group_start(bfhip_nupc *n, int n_members, const int filter[], const int coeff[], const int onto_base[],
                   long eq_taps, EqJob &j) {
    auto member = [&](int i, int code, const std::string &msg) {
        return nfail(code, "nupc_render_eq_group: member " + std::to_string(i) + ": " + msg);
    };
    for (int i = 0; i < n_members; i++) {
        if (!set_ok(n, filter[i], coeff[i])) return member(i, BFHIP_EINVAL, "no such filter or set");
        if (onto_base && onto_base[i]) {
            const int r = eq_base_check(n, filter[i], eq_taps);
            if (r < 0) return member(i, r, bfhip_nupc_last_error());
        }
        if (n->sets.sched.set_in_use(filter[i], coeff[i]))
            return member(i, BFHIP_ESTATE, "the set is live or part of a queued / in-flight switch");
        for (int k = 0; k < i; k++)
            if (filter[k] == filter[i] && coeff[k] == coeff[i]) return member(i, BFHIP_EINVAL, "the same set as member " + std::to_string(k));
    }
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (n->upd.inflight) return nfail(BFHIP_ESTATE, "nupc_render_eq_group: a rewrite is in flight (bfhip_nupc_update_busy)");
    UpdMember mem[kEqGroupMax];
    j.n_base = 0;
    for (int i = 0; i < n_members; i++) {
        const bool base = onto_base && onto_base[i];
        mem[i].filter = filter[i]; mem[i].set = coeff[i];
        mem[i].n_taps = base ? n->taps() : eq_taps;
        mem[i].src = (const uint8_t *)(base ? n->eq.app.ys[j.n_base] : n->eq.lin.taps);
        if (base) j.base[j.n_base++] = filter[i];
        if (past_set(n, filter[i], coeff[i], mem[i].src, true, mem[i].n_taps))
            return member(i, BFHIP_EINVAL, "set 0 of this filter is shorter than these taps (add_filter's length)");
    }
    return upd_go(n, n_members, mem, true, nullptr, &j);
}

// the state and count checks of a group call, in front of its curve check
int eq_group_check(const bfhip_nupc *n, int n_members, const int filter[], const int coeff[]) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->eq.group)
        return nfail(BFHIP_ESTATE, "nupc_render_eq_group: needs bfhip_nupc_reserve_eq_group before finalize, and finalize");
    if (n_members < 1 || n_members > n->eq.group || !filter || !coeff)
        return nfail(BFHIP_EINVAL, "nupc_render_eq_group: 1 .. max_members = " + std::to_string(n->eq.group) + " members, filter[] and coeff[]");
    return BFHIP_OK;
}

}  // namespace

// finalize's step: everything the asynchronous rewrite and the renders touch, so that they allocate nothing
// on the audio path
int nupc_host::upd_finalize(bfhip_nupc *n, int prio_least) {
    NupcUpdate &u = n->upd;
    if (u.reserve) {
        const size_t bytes = (size_t)n->taps() * n->rs;
        NCHK(bfhip_internal_pin_alloc((void **)&u.h_taps, bytes, hipHostMallocDefault));
        memset(u.h_taps, 0, bytes);
        NCHK(bfhip_internal_dev_alloc((void **)&u.d_taps, bytes));
        NCHK(hipMemset(u.d_taps, 0, bytes));
        NCHK(bfhip_internal_pin_alloc((void **)&u.h_bad, n->seg.size() * sizeof(int), hipHostMallocDefault));
        memset(u.h_bad, 0, n->seg.size() * sizeof(int));
        NCHK(hipStreamCreateWithPriority(&u.stream, hipStreamNonBlocking, prio_least));
        NCHK(hipEventCreateWithFlags(&u.ev_load, hipEventDisableTiming));
        NCHK(hipEventCreateWithFlags(&u.ev_main, hipEventDisableTiming));
        for (auto &s : n->seg) {
            if (s.delay_steps > 0) NCHK(hipEventCreateWithFlags(&s.ev_upd, hipEventDisableTiming));
            ECHK(bfhip_internal_engine_reserve_update(s.eng));
        }
        u.bad.resize(n->sets.coeff.size());
        for (size_t f = 0; f < n->sets.coeff.size(); f++) u.bad[f].assign(n->sets.coeff[f].size(), 0);
    }
    if (n->eq.reserve) {
        NCHK(eq_render_alloc(n->eq.lin, n->rs, n->eq.reserve));
        if (n->eq.min.reserved) NCHK(eq_minphase_alloc(n->eq.min, n->eq.lin));
        NCHK(hipEventCreateWithFlags(&n->eq.ev, hipEventDisableTiming));
    }
    // behind everything else, so that a convolver without this reservation allocates what it did, in order
    if (n->eq.app.reserved) {
        n->eq.base_want.resize(n->sets.coeff.size(), 0);
        NCHK(eq_apply_alloc(n->eq.app, n->eq.lin, n->taps(), n->eq.base_want));
        for (size_t f = 0; f < n->eq.base_want.size(); f++)
            if (n->eq.base_want[f]) NCHK(hipMemcpy(n->eq.app.base[f], n->eq.taps0[f].data(), n->eq.taps0[f].size(), hipMemcpyHostToDevice));
    }
    std::vector<std::vector<unsigned char>>().swap(n->eq.taps0);
    // and the group render's behind those: a result per member beyond the first, and their non-finite words
    if (n->eq.group) {
        const size_t words = (size_t)(n->eq.group - 1) * n->seg.size();
        hipError_t err = n->eq.app.reserved ? eq_apply_group_alloc(n->eq.app, n->eq.lin, n->eq.group) : hipSuccess;
        if (err == hipSuccess) err = bfhip_internal_pin_alloc((void **)&u.h_bad_group, words * sizeof(int), hipHostMallocDefault);
        if (err == hipErrorOutOfMemory) return nfail(BFHIP_ENOMEM, "nupc_finalize: out of memory for bfhip_nupc_reserve_eq_group's results");
        NCHK(err);
        memset(u.h_bad_group, 0, words * sizeof(int));
    }
    return BFHIP_OK;
}

// destroy's step (the streams have been waited for)
void nupc_host::upd_release(bfhip_nupc *n) {
    NupcUpdate &u = n->upd;
    if (u.h_taps) (void)hipHostFree(u.h_taps);
    if (u.h_bad) (void)hipHostFree(u.h_bad);
    if (u.h_bad_group) (void)hipHostFree(u.h_bad_group);
    if (u.d_taps) (void)hipFree(u.d_taps);
    eq_render_free(n->eq.lin);
    eq_minphase_free(n->eq.min);
    eq_apply_free(n->eq.app);
    if (n->eq.ev) (void)hipEventDestroy(n->eq.ev);
    if (u.ev_load) (void)hipEventDestroy(u.ev_load);
    if (u.ev_main) (void)hipEventDestroy(u.ev_main);
    if (u.stream) (void)hipStreamDestroy(u.stream);
}

// has every piece of every member of the rewrite in flight completed?  hipEventQuery only: never blocks.
// On completion the segment engines' non-finite flags (pinned, written behind each preparation)
// become the members' results, and the rewrite's.
int nupc_host::upd_poll(bfhip_nupc *n) {
    NupcUpdate &u = n->upd;
    if (!u.inflight) return BFHIP_OK;
    NCHK(hipSetDevice(n->device));
    for (size_t k = 0; k < n->seg.size() + 2; k++) {
        const hipEvent_t ev = k == 0 ? u.ev_load : k == 1 ? u.ev_main : n->seg[k - 2].ev_upd;
        if (!ev) continue;                                        // a main-stream segment: ev_main covers it
        const hipError_t e = hipEventQuery(ev);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); return BFHIP_OK; }
        if (e != hipSuccess) return nfail(BFHIP_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
    }
    int any = 0;
    for (int m = 0; m < u.n_members; m++) {
        int bad = 0;
        for (size_t k = 0; k < n->seg.size(); k++) bad |= *(volatile int *)bad_word(u, m, k, n->seg.size());
        u.mem[m].result = bad ? BFHIP_EINVAL : u.failed ? BFHIP_EHIP : BFHIP_OK;
        u.bad[u.mem[m].filter][u.mem[m].set] = bad || u.failed ? 1 : 0;
        any |= bad;
    }
    u.result = any ? BFHIP_EINVAL : u.failed ? BFHIP_EHIP : BFHIP_OK;
    u.inflight = false;
    return BFHIP_OK;
}

extern "C" {

// rewrite every partition of an idle set in every segment engine
int bfhip_nupc_update_coeff(bfhip_nupc *n, int filter, int coeff, const void *taps, long n_taps) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!set_ok(n, filter, coeff) || !taps || n_taps < 1 || n_taps > n->taps())
        return nfail(BFHIP_EINVAL, "nupc_update_coeff: bad argument");
    if (n->sets.sched.set_in_use(filter, coeff))
        return nfail(BFHIP_ESTATE, "nupc_update_coeff: the set is live or part of a queued / in-flight switch");
    OWNER(n);
    if (n->upd.reserve && n->finalized) {
        { const int r = upd_poll(n); if (r < 0) return r; }
        if (n->upd.inflight) return nfail(BFHIP_ESTATE, "nupc_update_coeff: an asynchronous rewrite is in flight (bfhip_nupc_update_busy)");
    }
    if (past_set(n, filter, coeff, taps, false, n_taps))
        return nfail(BFHIP_EINVAL, "nupc_update_coeff: set 0 of this filter is shorter than these taps (add_filter's length)");
    NCHK(hipSetDevice(n->device));
    const unsigned char *t = (const unsigned char *)taps;
    for (Seg &s : n->seg) {
        std::vector<unsigned char> part((size_t)s.L * n->rs);
        for (int p = 0; p < s.n_blocks[filter][coeff]; p++) {
            const long first = s.off + (long)p * s.L;
            const long take = std::max(0L, std::min((long)s.L, n_taps - first));
            std::fill(part.begin(), part.end(), 0);
            if (take > 0) memcpy(part.data(), t + (size_t)first * n->rs, (size_t)take * n->rs);
            ECHK(bfhip_engine_update_coeff_block(s.eng, n->sets.coeff[filter][coeff], p, part.data()));
        }
    }
    if (n->upd.reserve && n->finalized) n->upd.bad[filter][coeff] = 0;
    return BFHIP_OK;
}

// ---- asynchronous set rewrite ----------------------------------------------------------------

int bfhip_nupc_reserve_update(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_update after finalize");
    n->upd.reserve = true;
    return BFHIP_OK;
}

void *bfhip_nupc_update_buffer(bfhip_nupc *n) { return n && n->finalized ? n->upd.h_taps : nullptr; }

int bfhip_nupc_update_coeff_async(bfhip_nupc *n, int filter, int coeff, const void *taps, long n_taps) {
    return upd_start(n, filter, coeff, taps, false, n_taps, nullptr);
}

int bfhip_nupc_update_coeff_dev_async(bfhip_nupc *n, int filter, int coeff, const void *taps_dev, long n_taps,
                                      void *ready_event) {
    return upd_start(n, filter, coeff, taps_dev, true, n_taps, ready_event);
}

int bfhip_nupc_update_busy(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->upd.reserve) return 0;
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    return n->upd.inflight ? 1 : 0;
}

int bfhip_nupc_update_result(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->upd.reserve) return nfail(BFHIP_ESTATE, "nupc_update_result: no reservation (bfhip_nupc_reserve_update)");
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (n->upd.inflight) return nfail(BFHIP_ESTATE, "nupc_update_result: the rewrite is still in flight (bfhip_nupc_update_busy)");
    if (n->upd.result == BFHIP_EHIP) return nfail(BFHIP_EHIP, "nupc_update_result: the rewrite could not be enqueued completely");
    if (n->upd.result != BFHIP_OK) return nfail(n->upd.result, "NaN or Inf value among coefficients.");
    return BFHIP_OK;
}

int bfhip_nupc_update_result_member(bfhip_nupc *n, int member) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->upd.reserve) return nfail(BFHIP_ESTATE, "nupc_update_result_member: no reservation (bfhip_nupc_reserve_update)");
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (n->upd.inflight) return nfail(BFHIP_ESTATE, "nupc_update_result_member: the rewrite is still in flight (bfhip_nupc_update_busy)");
    if (member < 0 || member >= n->upd.n_members)
        return nfail(BFHIP_EINVAL, "nupc_update_result_member: the last rewrite had " + std::to_string(n->upd.n_members) + " members");
    const int r = n->upd.mem[member].result;
    if (r == BFHIP_EHIP) return nfail(BFHIP_EHIP, "nupc_update_result_member: the rewrite could not be enqueued completely");
    if (r != BFHIP_OK) return nfail(r, "NaN or Inf value among coefficients.");
    return BFHIP_OK;
}

// blocks: not for the audio thread
int bfhip_nupc_update_wait(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized || !n->upd.reserve) return nfail(BFHIP_ESTATE, "nupc_update_wait: no reservation (bfhip_nupc_reserve_update)");
    OWNER(n);
    if (n->upd.inflight) {
        NCHK(hipSetDevice(n->device));
        NCHK(hipEventSynchronize(n->upd.ev_load));
        NCHK(hipEventSynchronize(n->upd.ev_main));
        for (auto &s : n->seg) if (s.ev_upd) NCHK(hipEventSynchronize(s.ev_upd));
    }
    return bfhip_nupc_update_result(n);
}

// ---- equaliser curves rendered on the device -------------------------------------------------

int bfhip_nupc_reserve_eq(bfhip_nupc *n, long max_taps) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_eq after finalize");
    if (!n->upd.reserve) return nfail(BFHIP_ESTATE, "nupc_reserve_eq: needs bfhip_nupc_reserve_update first");
    if (max_taps < 8 || (max_taps & (max_taps - 1)) || max_taps > std::min(n->taps(), 1L << (kEqMaxLog2H + 1)))
        return nfail(BFHIP_EINVAL, "nupc_reserve_eq: max_taps must be a power of two, 8 .. min(taps, 1048576)");
    n->eq.reserve = max_taps;
    return BFHIP_OK;
}

int bfhip_nupc_reserve_eq_minimum(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_minimum after finalize");
    if (!n->eq.reserve) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_minimum: needs bfhip_nupc_reserve_eq first");
    n->eq.min.reserved = true;
    return BFHIP_OK;
}

int bfhip_nupc_render_eq_mode_async(bfhip_nupc *n, int filter, int coeff, long taps, int n_bands, const double freq[],
                                    const double mag[], const double phase[], int mode) {
    EqJob j;
    { const int r = eq_check(n, taps, n_bands, freq, mag, phase, mode, &j); if (r < 0) return r; }
    return upd_start(n, filter, coeff, n->eq.lin.taps, true, taps, nullptr, &j);
}

int bfhip_nupc_render_eq_async(bfhip_nupc *n, int filter, int coeff, long taps, int n_bands, const double freq[],
                               const double mag[], const double phase[]) {
    return bfhip_nupc_render_eq_mode_async(n, filter, coeff, taps, n_bands, freq, mag, phase, BFHIP_EQ_LINEAR);
}

int bfhip_nupc_render_eq_mode(bfhip_nupc *n, long taps, int n_bands, const double freq[], const double mag[],
                              const double phase[], int mode, void *taps_out) {
    EqJob j;
    { const int r = eq_check(n, taps, n_bands, freq, mag, phase, mode, &j); if (r < 0) return r; }
    return eq_render_sync(n, j, "nupc_render_eq", taps_out);
}

int bfhip_nupc_render_eq(bfhip_nupc *n, long taps, int n_bands, const double freq[], const double mag[],
                         const double phase[], void *taps_out) {
    return bfhip_nupc_render_eq_mode(n, taps, n_bands, freq, mag, phase, BFHIP_EQ_LINEAR, taps_out);
}

// ---- render onto a base impulse response (eq_apply.h) ----------------------------------------

int bfhip_nupc_reserve_eq_base(bfhip_nupc *n, int filter) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_base after finalize");
    if (!n->eq.reserve) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_base: needs bfhip_nupc_reserve_eq first");
    if (filter < 0 || filter >= (int)n->sets.coeff.size()) return nfail(BFHIP_EINVAL, "nupc_reserve_eq_base: no such filter");
    n->eq.base_want.resize(n->sets.coeff.size(), 0);
    n->eq.base_want[filter] = 1;
    n->eq.app.reserved = true;
    return BFHIP_OK;
}

int bfhip_nupc_reserve_eq_base_long(bfhip_nupc *n) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_base_long after finalize");
    if (!n->eq.reserve) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_base_long: needs bfhip_nupc_reserve_eq first");
    n->eq.app.reserved_long = true;
    return BFHIP_OK;
}

// blocks: not for the audio thread
int bfhip_nupc_set_eq_base(bfhip_nupc *n, int filter, const void *taps, long n_taps) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (!n->finalized) return nfail(BFHIP_ESTATE, "nupc_set_eq_base before finalize");
    if (filter < 0 || filter >= (int)n->sets.coeff.size() || !taps || n_taps < 1 || n_taps > n->taps())
        return nfail(BFHIP_EINVAL, "nupc_set_eq_base: bad argument");
    if (filter >= (int)n->eq.app.base.size() || !n->eq.app.base[filter])
        return nfail(BFHIP_ESTATE, "nupc_set_eq_base: needs bfhip_nupc_reserve_eq_base for this filter before finalize");
    OWNER(n);
    { const int r = upd_poll(n); if (r < 0) return r; }
    if (n->upd.inflight) return nfail(BFHIP_ESTATE, "nupc_set_eq_base: a rewrite is in flight (bfhip_nupc_update_busy)");
    for (long i = 0; i < n_taps; i++)
        if (!std::isfinite(n->rs == 4 ? (double)((const float *)taps)[i] : ((const double *)taps)[i]))
            return nfail(BFHIP_EINVAL, "NaN or Inf value among coefficients.");
    NCHK(hipSetDevice(n->device));
    uint8_t *b = (uint8_t *)n->eq.app.base[filter];
    const size_t bytes = (size_t)n_taps * n->rs, all = (size_t)n->taps() * n->rs;
    NCHK(hipMemcpyAsync(b, taps, bytes, hipMemcpyHostToDevice, n->upd.stream));
    if (all > bytes) NCHK(hipMemsetAsync(b + bytes, 0, all - bytes, n->upd.stream));
    NCHK(hipStreamSynchronize(n->upd.stream));
    return BFHIP_OK;
}

int bfhip_nupc_render_eq_base_async(bfhip_nupc *n, int filter, int coeff, long eq_taps, int n_bands, const double freq[],
                                    const double mag[], const double phase[], int mode) {
    if (n && filter < 0) return nfail(BFHIP_EINVAL, "nupc_render_eq_base: no such filter");
    EqJob j;
    { const int r = eq_check(n, eq_taps, n_bands, freq, mag, phase, mode, &j, filter); if (r < 0) return r; }
    return upd_start(n, filter, coeff, n->eq.app.y, true, n->taps(), nullptr, &j);
}

int bfhip_nupc_render_eq_base(bfhip_nupc *n, int filter, long eq_taps, int n_bands, const double freq[], const double mag[],
                              const double phase[], int mode, void *taps_out) {
    if (n && filter < 0) return nfail(BFHIP_EINVAL, "nupc_render_eq_base: no such filter");
    EqJob j;
    { const int r = eq_check(n, eq_taps, n_bands, freq, mag, phase, mode, &j, filter); if (r < 0) return r; }
    return eq_render_sync(n, j, "nupc_render_eq_base", taps_out);
}

// ---- one render across a group of filters ----------------------------------------------------

int bfhip_nupc_reserve_eq_group(bfhip_nupc *n, int max_members) {
    if (!n) return nfail(BFHIP_EINVAL, "null");
    if (n->finalized) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_group after finalize");
    if (!n->eq.reserve) return nfail(BFHIP_ESTATE, "nupc_reserve_eq_group: needs bfhip_nupc_reserve_eq first");
    if (max_members < 2 || max_members > BFHIP_NUPC_GROUP_MAX)
        return nfail(BFHIP_EINVAL, "nupc_reserve_eq_group: 2 .. 16 members");
    n->eq.group = max_members;
    return BFHIP_OK;
}

int bfhip_nupc_render_eq_group_async(bfhip_nupc *n, int n_members, const int filter[], const int coeff[],
                                     const int onto_base[], long eq_taps, int n_bands, const double freq[],
                                     const double mag[], const double phase[], int mode) {
    { const int r = eq_group_check(n, n_members, filter, coeff); if (r < 0) return r; }
    EqJob j;
    { const int r = eq_check(n, eq_taps, n_bands, freq, mag, phase, mode, &j); if (r < 0) return r; }
    return eq_group_start(n, n_members, filter, coeff, onto_base, eq_taps, j);
}

// ---- parametric equaliser sections (eq_biquad.h, biquad_host.h) -------------------------------

int bfhip_biquad_design(int type, double f0, double gain_db, double q, double coef[5]) {
    if (!biquad_design(type, f0, gain_db, q, coef))
        return nfail(BFHIP_EINVAL, "biquad_design: type 0 .. 6, 0 < f0 < 0.5, q > 0, gain_db finite, coef non-NULL");
    return BFHIP_OK;
}

int bfhip_nupc_render_biquads_async(bfhip_nupc *n, int filter, int coeff, long taps, int n_sections, const double coef[],
                                    int phase_mode) {
    EqJob j;
    { const int r = bq_check(n, taps, n_sections, coef, phase_mode, &j); if (r < 0) return r; }
    return upd_start(n, filter, coeff, n->eq.lin.taps, true, taps, nullptr, &j);
}

int bfhip_nupc_render_biquads(bfhip_nupc *n, long taps, int n_sections, const double coef[], int phase_mode, void *taps_out) {
    EqJob j;
    { const int r = bq_check(n, taps, n_sections, coef, phase_mode, &j); if (r < 0) return r; }
    return eq_render_sync(n, j, "nupc_render_biquads", taps_out);
}

int bfhip_nupc_render_biquads_base_async(bfhip_nupc *n, int filter, int coeff, long eq_taps, int n_sections,
                                         const double coef[], int phase_mode) {
    if (n && filter < 0) return nfail(BFHIP_EINVAL, "nupc_render_biquads_base: no such filter");
    EqJob j;
    { const int r = bq_check(n, eq_taps, n_sections, coef, phase_mode, &j, filter); if (r < 0) return r; }
    return upd_start(n, filter, coeff, n->eq.app.y, true, n->taps(), nullptr, &j);
}

int bfhip_nupc_render_biquads_base(bfhip_nupc *n, int filter, long eq_taps, int n_sections, const double coef[],
                                   int phase_mode, void *taps_out) {
    if (n && filter < 0) return nfail(BFHIP_EINVAL, "nupc_render_biquads_base: no such filter");
    EqJob j;
    { const int r = bq_check(n, eq_taps, n_sections, coef, phase_mode, &j, filter); if (r < 0) return r; }
    return eq_render_sync(n, j, "nupc_render_biquads_base", taps_out);
}

int bfhip_nupc_render_biquads_group_async(bfhip_nupc *n, int n_members, const int filter[], const int coeff[],
                                          const int onto_base[], long eq_taps, int n_sections, const double coef[],
                                          int phase_mode) {
    { const int r = eq_group_check(n, n_members, filter, coeff); if (r < 0) return r; }
    EqJob j;
    { const int r = bq_check(n, eq_taps, n_sections, coef, phase_mode, &j); if (r < 0) return r; }
    return eq_group_start(n, n_members, filter, coeff, onto_base, eq_taps, j);
}

}  // extern "C"
