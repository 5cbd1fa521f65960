// channels.h -- the channel stage of the engine (channels.hip): everything between the caller's raw buffers
// and the buffers the transforms read and write.  N:1 virtual -> physical channels with their integer delay
// lines and mutes, the sub-sample delay filters, the dither pass and its late variant, the planar copies of
// wide interleaved sides, and the device format tables that tell K1 and K3 where to read and write.
// Included by engine.h in front of struct bfhip_engine, which holds one Channels: include engine.h.
#pragma once

struct bfhip_engine;

BFHIP_HOST_NS {

// Pinned staging for the small per-block tables (N:1 channel jobs, delay-line moves, sub-sample
// delay jobs) that go to the device with every block: K slots, one per block in flight, so the
// upload is truly asynchronous and the host copy outlives the call that queued it.
struct Stage {
    static constexpr int K = 4;
    uint8_t *base = nullptr;
    size_t slot = 0;
    unsigned int turn = 0;             // (unsigned: a stream of 64-frame blocks passes 2^31 in a month)
    hipEvent_t done[K] = {nullptr, nullptr, nullptr, nullptr};
    bool pending[K] = {false, false, false, false};

    hipError_t init(size_t slot_bytes) {
        slot = (slot_bytes + 63) & ~(size_t)63;
        hipError_t r = pin_alloc((void **)&base, slot * K, hipHostMallocDefault);
        for (int i = 0; i < K && r == hipSuccess; i++) r = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
        return r;
    }
    void release() {
        for (int i = 0; i < K; i++) if (done[i]) { (void)hipEventDestroy(done[i]); done[i] = nullptr; }
        if (base) { (void)hipHostFree(base); base = nullptr; }
    }
    struct Part { const void *p; size_t bytes; };
    // The tables `parts`, one behind the other, through the next slot to `dev` on st.  The slot is free
    // again once the copy queued from it K blocks ago has run.
    hipError_t send(void *dev, std::initializer_list<Part> parts, hipStream_t st) {
        const int i = (int)(turn++ % (unsigned int)K);
        hipError_t r = hipSuccess;
        if (pending[i]) { if ((r = hipEventSynchronize(done[i])) != hipSuccess) return r; pending[i] = false; }
        uint8_t *pin = base + (size_t)i * slot;
        size_t n = 0;
        for (const Part &t : parts) { if (t.bytes) memcpy(pin + n, t.p, t.bytes); n += t.bytes; }
        if ((r = hipMemcpyAsync(dev, pin, n, hipMemcpyHostToDevice, st)) != hipSuccess) return r;
        r = hipEventRecord(done[i], st);
        pending[i] = r == hipSuccess;
        return r;
    }
};

// Host mirror of the reference's integer delay buffer (delay.c:29-45, 229-340, 346-411): same
// state variables, same decisions; the byte moves themselves are emitted as ByteOps that a
// device kernel executes on buffers in HBM.  Contiguous buffers only (how filter_process() uses
// it for channels that share a physical channel, bfrun.c:1517-1521, 1948).
struct DelayLine {
    int F = 0, ss = 0, maxdelay = 0, curdelay = 0, cur = 0, n_full = 0, n_full_cap = 0, n_rest = 0;
    DevBuf mem;                        // the arena on the device ...
    uint8_t *arena = nullptr;
    std::vector<uint8_t *> full;
    uint8_t *rest = nullptr, *shrt[2] = {nullptr, nullptr}, *tmp = nullptr;

    size_t frag() const { return (size_t)F * ss; }

    bool host = false;                 // ... self test: arena in host memory (the caller's to free), moves executed on the host

    int init(int fragment, int initdelay, int maxd, int sample_size) {
        F = fragment; ss = sample_size;
        int delay = maxd <= 0 ? initdelay : maxd;                      // delay.c:357-360
        if (maxd >= 0 && delay > maxd) delay = initdelay = maxd;
        if (maxd > 0 && initdelay > maxd) initdelay = maxd;            // (the reference overruns its buffer here)
        curdelay = initdelay; maxdelay = maxd;
        n_full_cap = delay > F ? delay / F + 1 : 0;
        const size_t total = (size_t)(n_full_cap + 4) * frag();
        if (host) {
            arena = (uint8_t *)calloc(total, 1);
            if (!arena) return BFHIP_ENOMEM;
        } else {
            if (mem.grow(total) != hipSuccess) return BFHIP_ENOMEM;
            arena = (uint8_t *)mem.p;
            if (hipMemset(arena, 0, total) != hipSuccess) return BFHIP_EHIP;
        }
        uint8_t *p = arena;
        for (int i = 0; i < n_full_cap; i++) { full.push_back(p); p += frag(); }
        rest = p; p += frag();
        shrt[0] = p; p += frag();
        shrt[1] = p; p += frag();
        tmp = p;
        if (delay == 0) return BFHIP_OK;
        if (delay <= F) { n_rest = initdelay; return BFHIP_OK; }       // :365-374
        n_rest = initdelay % F;
        n_full = initdelay / F + 1;
        if (n_full == 1) n_full = 0;
        return BFHIP_OK;
    }

    static void op(std::vector<ByteOp> &ops, uint8_t *dst, const uint8_t *src, size_t n) {
        if (n == 0) return;
        ByteOp o; o.dst = dst; o.src = src; o.n = (unsigned int)n; o.pad = 0;
        ops.push_back(o);
    }

    void retarget(int newdelay, std::vector<ByteOp> &ops) {           // change_delay, :283-318
        if (newdelay == curdelay || newdelay > maxdelay) return;
        if (newdelay <= F) {
            n_rest = newdelay;
            if (curdelay > F || curdelay < newdelay) {
                op(ops, shrt[0], nullptr, (size_t)newdelay * ss);
                op(ops, shrt[1], nullptr, (size_t)newdelay * ss);
            }
            n_full = 0; cur = 0; curdelay = newdelay;
            return;
        }
        n_rest = newdelay % F;
        n_full = newdelay / F + 1;
        if (curdelay < newdelay) {
            for (int i = 0; i < n_full; i++) op(ops, full[i], nullptr, frag());
            if (n_rest != 0) op(ops, rest, nullptr, (size_t)n_rest * ss);
        }
        cur = 0; curdelay = newdelay;
    }

    void update(uint8_t *buf, int delay, std::vector<ByteOp> &ops) {  // delay_update, :320-340
        retarget(delay, ops);
        const size_t rr = (size_t)n_rest * ss;
        if (n_full > 0) {                                              // update_delay_buffer
            uint8_t *last = cur == n_full - 1 ? full[0] : full[cur + 1];
            op(ops, full[cur], buf, frag());
            if (rr != 0) {
                op(ops, buf, rest, rr);
                op(ops, rest, last + (frag() - rr), rr);
            }
            op(ops, buf + rr, last, frag() - rr);
            if (++cur == n_full) cur = 0;
        } else if (n_rest > 0) {                                       // update_delay_short_buffer
            op(ops, shrt[cur], buf + (frag() - rr), rr);
            op(ops, tmp, buf, frag() - rr);                            // shift_samples via a
            op(ops, buf + rr, tmp, frag() - rr);                       // scratch copy
            cur = !cur;
            op(ops, buf, shrt[cur], rr);
        }
    }
};

// The stage's state.  What the setters of the C ABI write before finalize (and the run-time ones after
// it) comes first in every group; the rest is fixed by channels_setup.
struct Channels {
    // N:1 virtual -> physical channels (bfconf->virt2phys): the engine's fmt[] is indexed by PHYSICAL channel
    int n_phys[2] = {0, 0};
    std::vector<int> v2p[2], n_vpp[2], vdelay[2], vmaxdelay[2], vmuted[2];
    std::vector<DelayLine> vline[2];
    std::vector<int> vin_list;             // virtual inputs that share a physical one ...
    std::vector<int> vin_row;              // ... and, per virtual input, its row in b_incopy (-1: read from raw)
    std::vector<std::vector<int>> vout_groups;   // members of every shared physical output; a filtered 1:1 output alone
    std::vector<char> vout_dither;         // per group: requantised with dither (by the late pass)
    DevBuf b_incopy;                       // [vin_list.size()][L * 8]
    DevBuf b_vjobs;                        // per-block job/op tables: input half | output half
    size_t vjobs_slot = 0;
    Stage st_vin, st_vout, st_sd[2];       // their pinned staging, one slot per block in flight
    bool has_vchan = false;                // this engine uploads a per-block table: blocks differ in their launch arguments

    // sub-sample delay (sdf_length / sdf_beta / per-channel subdelay; delay.c:416-505)
    int sdf_length = 0, sd_flen = 0, sd_bs = 0;
    std::vector<int> subdelay[2];          // current value per virtual channel (-100 = undefined)
    std::vector<int> sd_slot[2];           // filter slot of a channel, -1 = none (fixed at finalize)
    bool sd_side[2] = {false, false};      // some channel of the side has a filter
    DevBuf b_sd_bank;                      // [199][flen] taps, index 99 + subdelay
    DevBuf b_sd_rest[2];
    DevBuf b_sdin;                         // [n filtered inputs][L] reals, what K1 reads
    DevBuf b_sdjobs[2];

    // HP-TPDF dither (dither.c, dither.h)
    std::vector<int> dither_channels;      // output channel of each dither slot (virtual, ascending, after finalize)
    std::vector<int> dither_rank;          // its rank among the dithered PHYSICAL outputs: where its table walk starts
    std::vector<char> dither_late;         // slot is the head of a shared / sub-sample-filtered output: dithered after the mix
    bool any_late = false;
    std::vector<int8_t> dither_table;
    int dither_spacing = 0;
    DevBuf b_dither_ch, b_dither_state, b_dither_table, b_randmap;     // (the last three: dither_upload_tables allocates them)
    DevBuf b_skip_quant;                   // [n_out] 1 = K3 does not requantise this channel (the dither pass or the mix does, or nobody here)
    DevBuf b_timeout;                      // [n_out][L] time samples K3 leaves for those passes

    // wide interleaved sides (>= 128 channels in one uniform frame; BFHIP_WIDE_IO=0/1): the raw frames are
    // transposed to / from a planar copy by a coalesced pass of their own (transpose_words_kernel)
    bool wide[2] = {false, false};
    DevBuf b_planar[2];                    // [n_phys][L] words of the side's sample size
    DevBuf b_phys_skip;                    // [n_phys out] 1 = another engine's channel (shards)

    void init(const int n_ch[2]);          // identity maps, nothing delayed, muted, filtered or dithered
    void release();

    bool shared(int io, int v) const { return n_vpp[io][v2p[io][v]] > 1; }
    bool side_uses_subdelay(int io) const { return sd_side[io]; }
    // The integer part of the side's sub-sample filters, sdf_length frames, which a channel WITHOUT a filter
    // is delayed by on top of its own delay so that the side stays aligned: bfrun.c:1152-1162 (inputs) and
    // 1185-1197 (outputs) at set-up, :1512-1516 and :1948 per block.  `ours`: the channel's delay is the
    // engine's to apply at all -- every private input copy, a member of a shared output, but not a 1:1
    // output that is here for its own filter (dai.c delays that one on the raw buffer).
    int extra_delay(int io, int v, bool ours = true) const { return ours && sd_side[io] && sd_slot[io][v] < 0 ? sdf_length : 0; }

    // what K3 is handed beside `raw`
    const unsigned char *skip_quant() const { return (const unsigned char *)b_skip_quant.p; }
    template <typename T> T *timeout(int first, int L) const { return b_timeout.p ? (T *)b_timeout.p + (size_t)first * L : (T *)nullptr; }

    // BEFORE set-up, of the whole configuration: no physical channel is shared ...
    bool one_to_one() const {
        for (int io = 0; io < 2; io++) for (int c : n_vpp[io]) if (c > 1) return false;
        return true;
    }
    // ... and nothing but the transforms touches a sample: what the fused [K3 | K1] schedules need
    bool configured_plain() const { return one_to_one() && sdf_length <= 0 && dither_channels.empty(); }
    // AFTER set-up, of this engine's share: the stage adds no launch to a block but the transposes of a wide side
    bool plain() const { return !has_vchan && dither_channels.empty(); }
    // launches of the stage follow the inverse transforms (timed apart: the reference's real2raw column)
    bool follows_k3() const { return !dither_channels.empty() || !vout_groups.empty() || sd_side[1]; }
    // the N:1 mix takes all of a block's outputs at once
    bool outputs_at_once() const { return !vout_groups.empty(); }
    // K3 alone writes the caller's output buffer
    bool k3_writes_raw() const { return dither_channels.empty() && !wide[1] && vout_groups.empty() && !sd_side[1]; }
};

// channels.hip.  Set-up, called by finalize between the ring allocation and the filter classification
// (resolve_shard has run; e->d_fmt[] is allocated), and the dither tables, which go up later:
int channels_setup(bfhip_engine *e);
int channels_upload_dither(bfhip_engine *e);
// Per block, on e->ls.  In front of the forward transforms: transpose of a wide side, N:1 gather with delay
// and mute, input sub-sample filters.
int channels_before_k1(bfhip_engine *e, const void *rawin_dev);
// what the output kernels get as `raw`
uint8_t *k3_target(bfhip_engine *e, void *rawout_dev);
// Behind the inverse transforms of virtual outputs [first, first + count), which wrote k3_target(): early
// dither, output sub-sample filters, N:1 mix with its late dither and overflow spread, transpose back.
int channels_after_k3(bfhip_engine *e, void *rawout_dev, int first, int count);

}  // namespace bfhip_host
