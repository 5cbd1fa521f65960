// channels.hip -- the channel stage (channels.h): its set-up at finalize, its two calls per block around
// the transforms, its tear-down.  What the reference does per channel with host buffers in
// filter_process() (bfrun.c:1503-1531 in front of the forward transforms, :1921-2003 behind the inverse
// ones) runs here as a few launches over job tables that go to the device with every block.
#include <algorithm>
#include <cstring>
#include <map>

#include "engine.h"
#include "dither_init.h"
#include "subdelay_filter.h"

BFHIP_HOST_NS {

void Channels::init(const int n_ch[2]) {
    for (int io = 0; io < 2; io++) {
        n_phys[io] = n_ch[io];
        for (int c = 0; c < n_ch[io]; c++) v2p[io].push_back(c);
        n_vpp[io].assign(n_ch[io], 1);
        for (auto *zero : {&vdelay[io], &vmaxdelay[io], &vmuted[io]}) zero->assign(n_ch[io], 0);
        subdelay[io].assign(n_ch[io], -100);       // BF_UNDEFINED_SUBDELAY
        sd_slot[io].assign(n_ch[io], -1);
    }
}

void Channels::release() {
    for (int io = 0; io < 2; io++) for (auto &dl : vline[io]) dl.mem.release();
    for (DevBuf *b : {&b_incopy, &b_vjobs, &b_sd_bank, &b_sd_rest[0], &b_sd_rest[1], &b_sdin, &b_sdjobs[0], &b_sdjobs[1],
                      &b_dither_ch, &b_dither_state, &b_dither_table, &b_randmap, &b_skip_quant, &b_timeout,
                      &b_planar[0], &b_planar[1], &b_phys_skip})
        b->release();
    for (Stage *s : {&st_vin, &st_vout, &st_sd[0], &st_sd[1]}) s->release();
}

}  // namespace bfhip_host

namespace {

#define BY_REAL(FN, ...) (e->rs == 4 ? FN<float>(__VA_ARGS__) : FN<double>(__VA_ARGS__))

DevFormat to_dev(const bfhip_format &f) {
    DevFormat d;
    d.isfloat = f.isfloat; d.swap = f.swap; d.bytes = f.bytes; d.sbytes = f.sbytes;
    d.sample_spacing = f.sample_spacing; d.byte_offset = f.byte_offset;
    d.alt = nullptr;
    return d;
}

// the delayed private copy of virtual input v (bfrun.c:1509-1531), contiguous; nullptr: v reads the raw frames
uint8_t *private_copy(const bfhip_engine *e, int v) {
    const int row = e->ch.vin_row[v];
    return row < 0 ? nullptr : (uint8_t *)e->ch.b_incopy.p + (size_t)row * e->L * 8;
}

hipError_t grow_zeroed(DevBuf &b, size_t bytes) {
    const hipError_t r = b.grow(bytes);
    return r == hipSuccess ? hipMemset(b.p, 0, bytes) : r;
}

hipError_t grow_filled(DevBuf &b, const void *src, size_t bytes) {
    const hipError_t r = b.grow(bytes);
    return r == hipSuccess ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : r;
}

// ------------------------------------------------------------------ set-up, in the order finalize runs it

// 1. filter slots of the channels with a defined sub-sample delay, and the filters' memory
//    (the filters themselves: subdelay_filter.h, shared with the non-uniform convolver)
int assign_filter_slots(bfhip_engine *e) {
    Channels &c = e->ch;
    if (c.sdf_length <= 0) return BFHIP_OK;
    int n_slots[2] = {0, 0};
    for (int io = 0; io < 2; io++)
        for (int v = 0; v < e->n_ch[io]; v++)
            c.sd_slot[io][v] = c.subdelay[io][v] != -100 ? n_slots[io]++ : -1;      // bfrun.c:1133-1142
    if (n_slots[0] + n_slots[1] == 0) { c.sdf_length = 0; return BFHIP_OK; }
    for (int io = 0; io < 2; io++) c.sd_side[io] = n_slots[io] > 0;
    // bank: index 99 + subdelay, subdelay in (-100, 100) hundredths of a sample (BF_SAMPLE_SLOTS)
    const std::vector<unsigned char> bank = sd_make_bank(c.sdf_length, e->rs);
    HIPCHK(grow_filled(c.b_sd_bank, bank.data(), bank.size()));
    for (int io = 0; io < 2; io++) {
        if (n_slots[io] == 0) continue;
        HIPCHK(grow_zeroed(c.b_sd_rest[io], (size_t)n_slots[io] * c.sd_bs * e->rs));
        HIPCHK(c.b_sdjobs[io].grow((size_t)n_slots[io] * 128));
        HIPCHK(c.st_sd[io].init((size_t)n_slots[io] * 128));
    }
    if (n_slots[0] > 0) HIPCHK(grow_zeroed(c.b_sdin, (size_t)n_slots[0] * e->L * e->rs));
    return BFHIP_OK;
}

// 2. the inputs with a private copy; the output groups the N:1 pass mixes and requantises
void form_groups(bfhip_engine *e) {
    Channels &c = e->ch;
    c.vin_list.clear(); c.vout_groups.clear();
    c.vin_row.assign(e->n_ch[0], -1);
    for (int v = 0; v < e->n_ch[0]; v++)
        if (c.shared(0, v)) { c.vin_row[v] = (int)c.vin_list.size(); c.vin_list.push_back(v); }
    // the members of a shared physical output are mixed in ascending virtual order, the order
    // in which the reference walks phys2virt (bfrun.c:2322-2323, 1938-2003); any mapping is
    // legal (bench4_config: `mapping: 0,1,0,1,0,1`)
    std::map<int, std::vector<int>> shared;
    for (int v = 0; v < e->n_ch[1]; v++) {
        if (c.shared(1, v)) shared[c.v2p[1][v]].push_back(v);
        // a 1:1 output with a sub-sample filter is requantised after the filter: a group of one
        else if (c.sd_slot[1][v] >= 0) c.vout_groups.push_back({v});
    }
    for (auto &kv : shared) c.vout_groups.push_back(kv.second);
    // (groups of outputs another engine converts: not ours to mix -- resolve_shard made sure a
    // group is owned as a whole)
    c.vout_groups.erase(std::remove_if(c.vout_groups.begin(), c.vout_groups.end(),
                                       [&](const std::vector<int> &g) { return !e->out_active[g[0]]; }),
                        c.vout_groups.end());
    c.has_vchan = !c.vin_list.empty() || !c.vout_groups.empty() || c.sdf_length > 0;
}

// 3. enable_dither named PHYSICAL outputs (bfconf->dither_state[physch], bfrun.c:1933): from here on the
//    list holds the virtual channel behind each of them, and who is requantised late is settled
int rank_dither(bfhip_engine *e) {
    Channels &c = e->ch;
    std::vector<std::pair<int, int>> byvirt;            // (virtual channel, rank in the physical list)
    for (size_t i = 0; i < c.dither_channels.size(); i++) {
        const int p = c.dither_channels[i];
        if (p < 0 || p >= c.n_phys[1]) return fail(BFHIP_EINVAL, "dither: output %d does not exist", p);
        int v = 0;
        while (c.v2p[1][v] != p) v++;          // the first (lowest) virtual channel of the physical one
        byvirt.push_back({v, (int)i});
    }
    std::sort(byvirt.begin(), byvirt.end());
    c.dither_channels.clear(); c.dither_rank.clear(); c.dither_late.clear();
    c.vout_dither.assign(c.vout_groups.size(), 0);
    c.any_late = false;
    for (auto &vr : byvirt) {
        const int v = vr.first;
        // an output another engine converts keeps its rank (= where its walk through the
        // random table starts, dither.c) but has no slot here
        if (!e->out_active[v]) continue;
        c.dither_channels.push_back(v);
        c.dither_rank.push_back(vr.second);
        // shared outputs and outputs with a sub-sample filter are requantised by the N:1
        // pass (bfrun.c:1938-2003): their dither runs on what that pass leaves behind
        const bool late = c.shared(1, v) || c.sd_slot[1][v] >= 0;
        c.dither_late.push_back(late);
        c.any_late = c.any_late || late;
        for (size_t g = 0; g < c.vout_groups.size(); g++) if (c.vout_groups[g][0] == v) c.vout_dither[g] = 1;
    }
    return BFHIP_OK;
}

// 4. delay lines of the private input copies and of the group members, the copies, the job tables
int make_delay_lines(bfhip_engine *e) {
    Channels &c = e->ch;
    if (!c.has_vchan) return BFHIP_OK;
    size_t n_ops_max = 0;
    c.vline[0].assign(e->n_ch[0], DelayLine());
    c.vline[1].assign(e->n_ch[1], DelayLine());
    // The reference adds the sub-sample filter's integer part to the delay AND to maxdelay
    // (bfrun.c:1152-1162, 1185-1197) -- also to maxdelay -1 ("cannot be changed"), which turns it
    // into the limit sdf_length - 1, below the delay it allocates for: delay.c:357-374 then sizes
    // the buffer for the limit and fills it with the delay (a heap overrun in the reference, found
    // by tests/test_gpu_refloop.py).  Here a negative maxdelay stays negative (fixed delay), and a
    // delay above a positive limit starts at the limit -- the clamp delay.c:358-360 means to make.
    auto init = [&](int io, int v, bool ours, int sample_size) {
        const int extra = c.extra_delay(io, v, ours);
        const int maxd = c.vmaxdelay[io][v] < 0 ? c.vmaxdelay[io][v] : c.vmaxdelay[io][v] + extra;
        int delay = c.vdelay[io][v] + extra;
        if (maxd > 0 && delay > maxd) delay = maxd;
        const int r = ours ? c.vline[io][v].init(e->L, delay, maxd, sample_size)
                           : c.vline[io][v].init(e->L, 0, 0, sample_size);      // a 1:1 output: dai.c delays it
        n_ops_max += c.vline[io][v].n_full_cap + 10;
        return r == BFHIP_OK ? r : fail(r, "delay buffer allocation failed");
    };
    for (int v : c.vin_list) { const int r = init(0, v, true, e->fmt[0][c.v2p[0][v]].bytes); if (r != BFHIP_OK) return r; }
    for (auto &g : c.vout_groups)
        for (int v : g) { const int r = init(1, v, g.size() > 1, e->rs); if (r != BFHIP_OK) return r; }
    if (!c.vin_list.empty()) HIPCHK(grow_zeroed(c.b_incopy, c.vin_list.size() * (size_t)e->L * 8));
    c.vjobs_slot = (n_ops_max + 8) * sizeof(ByteOp) + (e->n_ch[0] + e->n_ch[1] + 8) * 64;
    HIPCHK(c.b_vjobs.grow(2 * c.vjobs_slot));
    HIPCHK(c.st_vin.init(c.vjobs_slot));
    HIPCHK(c.st_vout.init(c.vjobs_slot));
    return BFHIP_OK;
}

// 5. the outputs K3 does not requantise itself (the dither pass or the N:1 mix does, from the time samples
//    K3 leaves behind), and the outputs another engine converts: nobody here writes them or their overflow state
int make_skip_table(bfhip_engine *e) {
    Channels &c = e->ch;
    if (!c.vout_groups.empty() || !c.dither_channels.empty() || e->sharded) {
        std::vector<unsigned char> skip(e->n_ch[1], 0);
        for (auto &g : c.vout_groups) for (int v : g) skip[v] = 1;
        for (int v : c.dither_channels) skip[v] = 1;
        for (int o = 0; o < e->n_ch[1]; o++) if (!e->out_active[o]) skip[o] = 1;
        HIPCHK(grow_filled(c.b_skip_quant, skip.data(), skip.size()));
    }
    if (!c.vout_groups.empty() || !c.dither_channels.empty()) HIPCHK(grow_zeroed(c.b_timeout, (size_t)e->n_ch[1] * e->L * e->rs));
    return BFHIP_OK;
}

// 6. wide interleaved sides: one uniform frame of >= 128 channels (words of 2, 4 or 8 bytes, channel p
//    at byte p * bytes of the frame), nothing on that side that reads its samples from a private
//    copy already (N:1 inputs, sub-sample delayed inputs); BFHIP_WIDE_IO=1 takes every eligible
//    side, 0 none
int make_wide_sides(bfhip_engine *e) {
    Channels &c = e->ch;
    for (int io = 0; io < 2; io++) {
        const int n = c.n_phys[io];
        bool ok = n >= 1 && !e->big;
        for (int p = 0; p < n && ok; p++) {
            const bfhip_format &f = e->fmt[io][p];
            ok = (f.bytes == 2 || f.bytes == 4 || f.bytes == 8) && f.bytes == e->fmt[io][0].bytes &&
                 f.sample_spacing == n && f.byte_offset == p * f.bytes;
        }
        if (io == 0) ok = ok && c.vin_list.empty() && !c.side_uses_subdelay(0);
        int want = 0;          // (measured on config D, 256 + 256 channels: no gain, DESIGN 6 -- kept as an option)
        if (const char *env = getenv("BFHIP_WIDE_IO")) want = atoi(env) != 0;
        c.wide[io] = ok && want;
        if (c.wide[io]) HIPCHK(grow_zeroed(c.b_planar[io], (size_t)n * e->L * e->fmt[io][0].bytes));
    }
    if (c.wide[1] && e->sharded) {
        std::vector<unsigned char> skip(c.n_phys[1], 0);
        for (int v = 0; v < e->n_ch[1]; v++) if (!e->out_active[v]) skip[c.v2p[1][v]] = 1;
        HIPCHK(grow_filled(c.b_phys_skip, skip.data(), skip.size()));
    }
    return BFHIP_OK;
}

// 7. the device format tables: indexed by VIRTUAL channel, they hold the physical channel's format, or
//    where the stage has put the channel's samples instead
int upload_formats(bfhip_engine *e) {
    const Channels &c = e->ch;
    for (int io = 0; io < 2; io++) {
        std::vector<DevFormat> d;
        for (int v = 0; v < e->n_ch[io]; v++) {
            const int ph = c.v2p[io][v];
            DevFormat f = to_dev(e->fmt[io][ph]);
            if (io == 0 && c.vin_row[v] >= 0) {
                f.alt = private_copy(e, v);
                f.sample_spacing = 1;
                f.byte_offset = 0;
            }
            if (c.wide[io]) {
                // the transforms read / write the planar copy: channel p's L words, contiguous
                f.sample_spacing = 1;
                if (io == 0) { f.alt = (uint8_t *)c.b_planar[0].p + (size_t)ph * e->L * f.bytes; f.byte_offset = 0; }
                else f.byte_offset = (int)((size_t)ph * e->L * f.bytes);       // relative to the planar copy, the `raw` of the output kernels
            }
            if (io == 0 && c.sd_slot[0][v] >= 0) {
                // sub-sample filtered: K1 reads the filtered reals (the conversion from the
                // raw format happened in the filter pass)
                f.alt = (const uint8_t *)c.b_sdin.p + (size_t)c.sd_slot[0][v] * e->L * e->rs;
                f.isfloat = 1; f.swap = 0; f.bytes = e->rs; f.sbytes = e->rs;
                f.sample_spacing = 1; f.byte_offset = 0;
            }
            d.push_back(f);
        }
        if (!d.empty()) HIPCHK(hipMemcpy(e->d_fmt[io], d.data(), d.size() * sizeof(DevFormat), hipMemcpyHostToDevice));
    }
    return BFHIP_OK;
}

// ------------------------------------------------------------------ per block

// sub-sample delay of the channels that have a filter (bfrun.c:1503-1508 apply_subdelay, :1921-1925)
template <typename T>
int filter_subdelays(bfhip_engine *e, int io, const void *rawin_dev) {
    Channels &c = e->ch;
    if (c.sdf_length <= 0) return BFHIP_OK;
    std::vector<SdJob<T>> jobs;
    for (int v = 0; v < e->n_ch[io]; v++) {
        const int slot = c.sd_slot[io][v];
        if (slot < 0) continue;
        // an output another engine converts is not filtered here: nobody mixes or quantises it in this
        // engine, and an engine that owns no such output at all has no time-sample buffer either
        if (io == 1 && (!e->out_active[v] || c.b_timeout.p == nullptr)) continue;
        SdJob<T> j;
        memset(&j, 0, sizeof(j));
        const int sd = c.subdelay[io][v];
        j.taps = (sd > -100 && sd < 100) ? (const T *)c.b_sd_bank.p + (size_t)(99 + sd) * c.sd_flen : nullptr;
        j.rest = (T *)c.b_sd_rest[io].p + (size_t)slot * c.sd_bs;
        if (io == 0) {
            j.fmt = to_dev(e->fmt[0][c.v2p[0][v]]);
            j.raw = (const uint8_t *)rawin_dev;
            if (const uint8_t *copy = private_copy(e, v)) { j.raw = copy; j.fmt.sample_spacing = 1; j.fmt.byte_offset = 0; }
            j.dst = (T *)c.b_sdin.p + (size_t)slot * e->L;
        } else {
            j.src = j.dst = c.timeout<T>(v, e->L);
        }
        jobs.push_back(j);
    }
    if (jobs.empty()) return BFHIP_OK;
    const SdJob<T> *dev = (const SdJob<T> *)c.b_sdjobs[io].p;
    HIPCHK(c.st_sd[io].send(c.b_sdjobs[io].p, {{jobs.data(), jobs.size() * sizeof(SdJob<T>)}}, e->ls));
    const int tile = sd_tile_frames(e->L, c.sd_bs, (int)sizeof(T));        // > 0: enable_subdelay
    const size_t lds = (size_t)(c.sd_bs + tile) * sizeof(T);
    auto k = subdelay_fir_kernel<T>;
    HIPCHK(allow_lds(k, lds));
    hipLaunchKernelGGL(k, dim3((unsigned)jobs.size()), dim3(256), lds, e->ls, dev, e->L, c.sd_bs, c.sd_flen, tile);
    HIPCHK(hipGetLastError());
    return BFHIP_OK;
}

// N:1 inputs: gather + mute + integer delay into the private copies K1 reads (bfrun.c:1509-1531)
int gather_inputs(bfhip_engine *e, const void *rawin_dev) {
    Channels &c = e->ch;
    if (c.vin_list.empty()) return BFHIP_OK;
    std::vector<VInJob> jobs;
    std::vector<ByteOp> ops;
    for (int v : c.vin_list) {
        const bfhip_format &f = e->fmt[0][c.v2p[0][v]];
        VInJob j;
        j.copy = private_copy(e, v);
        j.byte_offset = f.byte_offset; j.sample_spacing = f.sample_spacing; j.bytes = f.bytes;
        j.muted = c.vmuted[0][v];
        j.ops_off = (int)ops.size();
        if (!j.muted) c.vline[0][v].update(j.copy, c.vdelay[0][v] + c.extra_delay(0, v), ops);   // not advanced when muted
        j.n_ops = (int)ops.size() - j.ops_off;
        jobs.push_back(j);
    }
    const size_t jb = jobs.size() * sizeof(VInJob), ob = ops.size() * sizeof(ByteOp);
    if (jb + ob > c.vjobs_slot) return fail(BFHIP_ESTATE, "virtual-channel job table overflow");
    unsigned char *dev = (unsigned char *)c.b_vjobs.p;
    HIPCHK(c.st_vin.send(dev, {{jobs.data(), jb}, {ops.data(), ob}}, e->ls));
    hipLaunchKernelGGL(vchan_in_kernel<0>, dim3((unsigned)jobs.size()), dim3(256), 0, e->ls,
                       (const VInJob *)dev, (const ByteOp *)(dev + jb), (const uint8_t *)rawin_dev, e->L);
    HIPCHK(hipGetLastError());
    return BFHIP_OK;
}

// the HP-TPDF pass over the dither slots whose channel lies in [first, first + count) (the slots are sorted
// by channel), in runs of the requested phase: straight after K3, or after the N:1 mix / sub-sample filter
template <typename T>
int dither_pass(bfhip_engine *e, int first, int count, uint8_t *raw, bool late) {
    const Channels &c = e->ch;
    const int n = (int)c.dither_channels.size();
    for (int s0 = 0; s0 < n;) {
        auto in = [&](int s) { return c.dither_channels[s] >= first && c.dither_channels[s] < first + count && (bool)c.dither_late[s] == late; };
        if (!in(s0)) { s0++; continue; }
        int s1 = s0 + 1;
        while (s1 < n && in(s1)) s1++;
        hipLaunchKernelGGL(dither_kernel<T>, dim3(s1 - s0), dim3(64), 0, e->ls,
                           (const T *)c.b_timeout.p, (const int *)c.b_dither_ch.p + s0,
                           (DitherState<T> *)c.b_dither_state.p + s0, (const int8_t *)c.b_dither_table.p,
                           (int)c.dither_table.size(), (const T *)c.b_randmap.p + 256,
                           e->d_fmt[1], e->d_over, raw, e->L, e->safety_limit, e->d_status);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return fail(BFHIP_EHIP, "dither launch: %s", hipGetErrorString(err));
        s0 = s1;
    }
    return BFHIP_OK;
}

// N:1 outputs: integer delay of every member, mix of the un-muted ones, one requantisation
// (bfrun.c:1938-2003); runs after K3 has left the members' time samples in b_timeout
template <typename T>
int mix_outputs(bfhip_engine *e, uint8_t *raw) {
    Channels &c = e->ch;
    if (c.vout_groups.empty()) return BFHIP_OK;
    std::vector<VOutJob> jobs;
    std::vector<VOutMember> mem;
    std::vector<ByteOp> ops;
    for (size_t gi = 0; gi < c.vout_groups.size(); gi++) {
        const std::vector<int> &g = c.vout_groups[gi];
        // a 1:1 output is here for its sub-sample filter only: its delay and mute are dai.c's business
        // on the raw buffer (bfrun.c:1926-1936 converts it whatever icomm says)
        const bool shared = g.size() > 1;
        VOutJob j;
        j.first_member = (int)mem.size(); j.n_members = (int)g.size(); j.fmt_channel = g[0]; j.dither = c.vout_dither[gi];
        for (int v : g) {
            VOutMember m;
            m.channel = v; m.muted = shared ? c.vmuted[1][v] : 0; m.ops_off = (int)ops.size();
            c.vline[1][v].update((uint8_t *)c.timeout<T>(v, e->L), shared ? c.vdelay[1][v] + c.extra_delay(1, v) : 0, ops);   // always advanced (:1948)
            m.n_ops = (int)ops.size() - m.ops_off;
            mem.push_back(m);
        }
        jobs.push_back(j);
    }
    const size_t jb = jobs.size() * sizeof(VOutJob), mb = mem.size() * sizeof(VOutMember), ob = ops.size() * sizeof(ByteOp);
    if (jb + mb + ob > c.vjobs_slot) return fail(BFHIP_ESTATE, "virtual-channel job table overflow");
    unsigned char *dev = (unsigned char *)c.b_vjobs.p + c.vjobs_slot;      // second half: output side
    HIPCHK(c.st_vout.send(dev, {{jobs.data(), jb}, {mem.data(), mb}, {ops.data(), ob}}, e->ls));
    hipLaunchKernelGGL(vchan_out_kernel<T>, dim3((unsigned)jobs.size()), dim3(256), 0, e->ls,
                       (const VOutJob *)dev, (const VOutMember *)(dev + jb), (const ByteOp *)(dev + jb + mb),
                       (T *)c.b_timeout.p, e->d_fmt[1], e->d_over, raw, e->L, e->safety_limit, e->d_status);
    HIPCHK(hipGetLastError());
    if (!c.any_late) return BFHIP_OK;
    { const int r = dither_pass<T>(e, 0, e->n_ch[1], raw, true); if (r != BFHIP_OK) return r; }
    hipLaunchKernelGGL(vout_spread_overflow_kernel<0>, dim3((unsigned)jobs.size()), dim3(64), 0, e->ls,
                       (const VOutJob *)dev, (const VOutMember *)(dev + jb), e->d_over);
    HIPCHK(hipGetLastError());
    return BFHIP_OK;
}

// wide interleaved sides: frames <-> planar copy of physical channels [first, first + count)
int transpose_side(bfhip_engine *e, int io, const void *src, void *dst, int to_planar, int first, int count) {
    const int rows = e->L, cols = e->ch.n_phys[io], bytes = e->fmt[io][0].bytes;
    const dim3 grid((cols + 63) / 64, (rows + 63) / 64);
    const unsigned char *skip = io == 1 ? (const unsigned char *)e->ch.b_phys_skip.p : nullptr;
    if (bytes == 4)
        hipLaunchKernelGGL(transpose_words_kernel<uint32_t>, grid, dim3(256), 0, e->ls, (const uint32_t *)src, (uint32_t *)dst, rows, cols, to_planar, skip, first, count);
    else if (bytes == 2)
        hipLaunchKernelGGL(transpose_words_kernel<uint16_t>, grid, dim3(256), 0, e->ls, (const uint16_t *)src, (uint16_t *)dst, rows, cols, to_planar, skip, first, count);
    else
        hipLaunchKernelGGL(transpose_words_kernel<uint64_t>, grid, dim3(256), 0, e->ls, (const uint64_t *)src, (uint64_t *)dst, rows, cols, to_planar, skip, first, count);
    HIPCHK(hipGetLastError());
    return BFHIP_OK;
}

template <typename T>
int after_k3(bfhip_engine *e, void *rawout_dev, int first, int count) {
    const Channels &c = e->ch;
    uint8_t *raw = k3_target(e, rawout_dev);
    int r;
    if ((r = dither_pass<T>(e, first, count, raw, false)) != BFHIP_OK) return r;
    if ((r = filter_subdelays<T>(e, 1, nullptr)) != BFHIP_OK) return r;
    if ((r = mix_outputs<T>(e, raw)) != BFHIP_OK) return r;
    if (!c.wide[1]) return BFHIP_OK;
    int p0 = c.n_phys[1], p1 = -1;
    for (int v = first; v < first + count; v++) { p0 = std::min(p0, c.v2p[1][v]); p1 = std::max(p1, c.v2p[1][v]); }
    return p1 < p0 ? BFHIP_OK : transpose_side(e, 1, raw, rawout_dev, 0, p0, p1 - p0 + 1);
}

}  // namespace

BFHIP_HOST_NS {

int channels_setup(bfhip_engine *e) {
    int r;
    if ((r = assign_filter_slots(e)) != BFHIP_OK) return r;
    form_groups(e);
    if ((r = rank_dither(e)) != BFHIP_OK) return r;
    if ((r = make_delay_lines(e)) != BFHIP_OK) return r;
    if ((r = make_skip_table(e)) != BFHIP_OK) return r;
    if ((r = make_wide_sides(e)) != BFHIP_OK) return r;
    return upload_formats(e);
}

int channels_upload_dither(bfhip_engine *e) {
    Channels &c = e->ch;
    if (c.dither_channels.empty()) return BFHIP_OK;
    HIPCHK(grow_filled(c.b_dither_ch, c.dither_channels.data(), c.dither_channels.size() * sizeof(int)));
    // table, randmap, per-slot states (ptr = rank * spacing + 1, error feedback zero)
    HIPCHK(dither_upload_tables(c.dither_table, c.dither_spacing, c.dither_rank, e->rs, (int8_t **)&c.b_dither_table.p,
                                &c.b_randmap.p, &c.b_dither_state.p));
    return BFHIP_OK;
}

int channels_before_k1(bfhip_engine *e, const void *rawin_dev) {
    int r;
    if (e->ch.wide[0] && (r = transpose_side(e, 0, rawin_dev, e->ch.b_planar[0].p, 1, 0, e->ch.n_phys[0])) != BFHIP_OK) return r;
    if ((r = gather_inputs(e, rawin_dev)) != BFHIP_OK) return r;
    return BY_REAL(filter_subdelays, e, 0, rawin_dev);
}

uint8_t *k3_target(bfhip_engine *e, void *rawout_dev) { return e->ch.wide[1] ? (uint8_t *)e->ch.b_planar[1].p : (uint8_t *)rawout_dev; }

int channels_after_k3(bfhip_engine *e, void *rawout_dev, int first, int count) { return BY_REAL(after_k3, e, rawout_dev, first, count); }

}  // namespace bfhip_host
