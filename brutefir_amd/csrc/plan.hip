// plan.hip -- the plan builder of the engine (bfhip.hip): the filter network as the device sees it.
//
// build_plan turns the filters into MAC entries, level jobs, chunk boundaries and the job table of the
// diag kernel, in host steps over one Plan value (plan_collect .. plan_level_blob: no runtime call, the
// engine read-only, device addresses as plain values); plan_upload then grows the device buffers, copies
// the tables and brings the two stream-ordered coefficient layouts up to date, and plan_commit alone
// writes the engine's geometry.  Whatever fails, plan_dirty stays set and the next block builds again.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>

#include "engine.h"

namespace {

// the environment's say in a plan, read once per build (tests change it between builds of one process)
struct PlanKnobs {
    bool has_target_wgs = false;
    int target_wgs = 256;              // BFHIP_MAC_TARGET_WGS: MAC workgroups to aim for (set: no cost model)
    bool mac_nt = true;                // BFHIP_MAC_NT; unset: what the engine holds
    int mac_unroll = 0;                // BFHIP_MAC_UNROLL; likewise
    bool diag = true;                  // BFHIP_MAC_DIAG=0 keeps the crossbar kernel
    bool has_diag_split = false;
    int diag_split = 0;                // BFHIP_DIAG_SPLIT: parts of a one-to-one plan
    int long_chunks = 1;               // BFHIP_LONG_CHUNKS
    int lookahead = -1, lookahead_far = -1;    // BFHIP_LOOKAHEAD, BFHIP_LOOKAHEAD_FAR: 1 / 0 always / never, -1 by volume
};

bool env_int(const char *name, int *v) {
    const char *s = getenv(name);
    if (s) *v = atoi(s);
    return s != nullptr;
}

PlanKnobs read_knobs(const bfhip_engine *e) {
    PlanKnobs k;
    int v = 0;
    if ((k.has_target_wgs = env_int("BFHIP_MAC_TARGET_WGS", &v))) k.target_wgs = std::max(1, v);
    k.mac_nt = env_int("BFHIP_MAC_NT", &v) ? v != 0 : e->mac_nt;
    k.mac_unroll = env_int("BFHIP_MAC_UNROLL", &v) ? v : e->mac_unroll;
    if (env_int("BFHIP_MAC_DIAG", &v)) k.diag = v != 0;
    k.has_diag_split = env_int("BFHIP_DIAG_SPLIT", &k.diag_split);
    if (env_int("BFHIP_LONG_CHUNKS", &v)) k.long_chunks = std::max(1, v);
    if (env_int("BFHIP_LOOKAHEAD", &v)) k.lookahead = v != 0 ? 1 : 0;
    if (env_int("BFHIP_LOOKAHEAD_FAR", &v)) k.lookahead_far = v != 0 ? 1 : 0;
    return k;
}

// what plan_long_whole found on the whole configuration's entries: a plain uniform crossbar (ok), its
// entries per group (E) and partitions (P), and the whole-plan position of every entry of `flat`
struct LongWhole { bool ok = false; int E = 0, P = 0; std::vector<int> wpos; };

// A plan on the host: what the steps hand on to each other, and what plan_commit writes into the engine.
template <typename T> struct Plan {
    PlanKnobs knobs;
    // geometry
    int n_groups = 0, n_out_padded = 0, mac_threads = 256, n_tiles = 1, S = 1;
    bool all_dense = false, mac_diag = false, any_fading = false;
    bool diag_plan = false;            // one-to-one: chunk c = part c of every entry
    bool lw_plain = true;              // no filter mixes, cascades, fades or has a ring of its own
    long n_names = 0;                  // ring ids of materialised outputs start at I + n_names
    // the MAC entries of every group, in step: which terms belong to filters another engine runs
    // ([group][entry] bit j) and, in a diag plan, which part an entry is
    std::vector<std::vector<MacEntry<T>>> per_group;
    std::vector<std::vector<unsigned int>> foreign;
    std::vector<std::vector<int>> part_of;
    // (ring id, delay) -> the entries of a group made for it, in the order they were needed
    std::vector<std::map<std::pair<long, int>, std::vector<int>>> index;
    std::vector<MacEntry<T>> flat;
    std::vector<ChunkRange> chunks;
    std::vector<int> diag_jobs;
    LongWhole lwh;
    // the levelled (non fast-path) filters: jobs per level, then one device blob
    std::vector<std::vector<FillJob<T>>> fills;
    std::vector<std::vector<FilterJob<T>>> filts;
    std::vector<std::vector<FadeJob<T>>> fades;
    std::vector<MixSrc<T>> srcs;
    std::vector<unsigned char> blob;
    std::vector<bfhip_engine::LevelJobs> level_jobs;
    size_t src_off = 0;
    // coefficient bytes a block reads here / in the whole configuration (what the launch geometry is chosen for)
    double bytes_H = 0, bytes_H_plan = 0;
    // ring id: 0..I-1 input rings, I+f private ring of filter f, I+F+f materialised Y_f
    std::map<long, std::vector<char>> ring_used;
};

// long partitions [p_first, p_first + n_p) of the long entries listed in d_lwhich[0 .. n_which)
int derive_long(bfhip_engine *e, int n_groups, int p_first, int n_p, int n_which) {
    const size_t lds = lds_fft_bytes(LW_LOG2, sizeof(c2<float>));
    auto k = coeff_long_kernel<float, LW_LOG2>;
    HIPCHK(allow_lds(k, lds));
    hipLaunchKernelGGL(k, dim3((unsigned)n_p, (unsigned)OG, (unsigned)n_which), dim3(fft_threads<float>(LW_LOG2)), lds,
                       e->stream, (const MacEntry<float> *)e->b_lentries.p, (const StreamWhere *)e->b_lwhere.p,
                       (const int *)e->d_lwhich, p_first, e->lw_Pstd, e->N, n_groups, e->lw_chunks, e->lstream,
                       (const c2<float> *)e->d_tw, (const c2<float> *)e->d_tw14);
    HIPCHK(hipGetLastError());
    return sync_all(e);
}

// (Re)build the stream-ordered coefficient copy for the plan just uploaded, if the plan is a
// uniform crossbar: every entry OG coefficient terms of the same length, no split entries, every
// chunk the same number of entries, no idle blocks in the grid.  Entries whose OG sets did not
// change since the last build are left alone (scale changes rebuild the plan, not the data).
template <typename T>
int build_stream_layout(bfhip_engine *e, const Plan<T> &pl) {
    const std::vector<MacEntry<T>> &flat = pl.flat;
    const std::vector<ChunkRange> &chunks = pl.chunks;
    const int S = pl.S;
    e->hstream = StreamLayout{nullptr, 0, 0, 0};
    if (!e->stream_wanted || !pl.all_dense || flat.empty()) return BFHIP_OK;
    if (e->stream_wanted == 1 && pl.bytes_H < 64.0 * 1048576.0) return BFHIP_OK;      // cache resident anyway
    const int n_tc = pl.n_tiles * S;
    if (n_tc % 8 != 0 || pl.mac_threads != 256 || !pl.knobs.mac_nt || pl.knobs.mac_unroll != 0) return BFHIP_OK;
    const int P = flat[0].maxP, E_c = chunks[0].end - chunks[0].begin;
    for (auto &cr : chunks) if (cr.end - cr.begin != E_c) return BFHIP_OK;
    for (auto &en : flat) if (en.dense != 1 || en.p0 != 0 || en.maxP != P) return BFHIP_OK;
    if (E_c < 1 || P < 1) return BFHIP_OK;
    const unsigned int chunk = 256u * 16u;
    const unsigned long long entry_bytes = (unsigned long long)P * OG * chunk;
    const unsigned long long slice = (unsigned long long)E_c * entry_bytes;
    if (entry_bytes >= (1ull << 31) || slice >= (1ull << 32)) return BFHIP_OK;       // 32-bit offsets inside a slice
    const unsigned long long grid = (unsigned long long)n_tc * pl.n_groups;
    const size_t total = (size_t)(grid * slice);
    const int geom[5] = {(int)flat.size(), E_c, P, n_tc, pl.n_groups};
    const bool same_geom = e->b_stream.p != nullptr && memcmp(geom, e->stream_geom, sizeof(geom)) == 0;
    if (!same_geom) {
        if (e->b_stream.grow(total) != hipSuccess) {
            (void)hipGetLastError();
            return BFHIP_OK;                 // no room for the second copy: the set-major path still works
        }
        e->stream_keys.clear();
        memcpy(e->stream_geom, geom, sizeof(geom));
    }
    // which entries hold other sets than last time?
    std::vector<int> changed;
    std::vector<StreamWhere> where(flat.size());
    e->stream_keys.resize(flat.size(), std::array<const void *, OG>{});
    for (int g = 0; g < pl.n_groups; g++) {
        for (int c = 0; c < S; c++) {
            const ChunkRange cr = chunks[(size_t)g * S + c];
            for (int q = 0; q < E_c; q++) {
                const int idx = cr.begin + q;
                where[idx] = StreamWhere{g, c, q, 0};
                std::array<const void *, OG> key;
                for (int j = 0; j < OG; j++) key[j] = flat[idx].term[j].H;
                if (key != e->stream_keys[idx]) { changed.push_back(idx); e->stream_keys[idx] = key; }
            }
        }
    }
    StreamLayout sl;
    sl.base = (const unsigned char *)e->b_stream.p; sl.slice = slice; sl.entry_bytes = (unsigned int)entry_bytes; sl.chunk = chunk;
    if (!changed.empty()) {
        const size_t wb = where.size() * sizeof(StreamWhere), cb = changed.size() * sizeof(int);
        if (wb + cb > e->b_where.cap) HIPCHK(e->b_where.grow(wb + flat.size() * sizeof(int)));
        e->d_which = (int *)((unsigned char *)e->b_where.p + wb);
        HIPCHK(hipMemcpy(e->b_where.p, where.data(), wb, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(e->d_which, changed.data(), cb, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(stream_relayout_kernel<T>, dim3((unsigned)P, (unsigned)pl.n_tiles, (unsigned)changed.size()), dim3(256), 0,
                           e->stream, (const MacEntry<T> *)e->b_entries.p, (const StreamWhere *)e->b_where.p, (const int *)e->d_which,
                           0, e->L, pl.n_groups, S, sl);
        HIPCHK(hipGetLastError());
        { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    }
    e->hstream = sl;
    return BFHIP_OK;
}

// May the long plan run the look-ahead MAC (la), and its far tier on top (far)?  Decided on the long
// entries and the knobs; the caller still has to find room for the ahead buffers.
//   la: the whole plan is this engine's (`whole`), one chunk per group, no tail partition reaches a block
// younger than t - 3 (the shifted last partition does when it is p = 1), and the coefficients are large
// enough to be worth three ahead buffers per block (BFHIP_LOOKAHEAD=1 / 0: always / never).
//   far: some entry has a partition >= 2 beyond the first, none of them reaches a block younger than
// t - 6 (the shifted last partition does when it is p = 2 without delay), and the same volume
// (BFHIP_LOOKAHEAD_FAR=1 / 0: whenever the first tier runs / never; BFHIP_LOOKAHEAD=1 alone: not).
struct LongGates { bool la, far; };
LongGates long_gates(const bfhip_engine *e, const std::vector<MacEntry<float>> &lflat, const PlanKnobs &k, int SL, bool whole) {
    double vol = 0;
    for (auto &c : e->coeffs) vol += (double)c.n_blocks * (double)e->L * (double)sizeof(c2<float>);
    const bool large = vol >= 1073741824.0;
    bool la = k.lookahead != 0 && (k.lookahead == 1 || large) && SL == 1 && !e->sharded && !e->pairs && whole;
    for (size_t i = 0; i < lflat.size() && la; i++) {
        const MacEntry<float> &en = lflat[i];
        la = en.dense == 1 && en.p0 == 0 && (en.maxP < 2 || 3 * (en.maxP - 1) - en.shift + en.delay >= 3);
    }
    bool far = la && k.lookahead_far != 0 && (k.lookahead_far == 1 || large);
    bool any3 = false;
    for (size_t i = 0; i < lflat.size() && far; i++) {
        const MacEntry<float> &en = lflat[i];
        any3 = any3 || en.maxP >= 3;
        far = en.maxP < 3 || 3 * (en.maxP - 1) - en.shift + en.delay >= 6;
    }
    return LongGates{la, far && any3};
}

// The long-window plan for a plain uniform crossbar: the standard plan's entries with the long rings
// (ring step 3 in the MAC), chunks of lw_chunks per group, and the long coefficient partitions derived
// from the sets' standard spectra straight into their own stream-ordered layout (StreamLayout; only the
// entries whose sets, delay or length changed since the last build).  Anything else: lw_active = false
// and every block runs the standard path.
int build_long_layout(bfhip_engine *e, const Plan<float> &pl) {
    const std::vector<MacEntry<float>> &flat = pl.flat;
    const std::vector<ChunkRange> &chunks = pl.chunks;
    const LongWhole &lwh = pl.lwh;
    const int S = pl.S;
    e->lw_active = false;
    e->la_active = e->far_active = false;
    e->la_epoch++;                 // a new plan: other sets, scales, delays or lengths than the stored products used
    if (!lwh.ok || flat.empty() || pl.mac_diag || !pl.knobs.mac_nt || pl.knobs.mac_unroll != 0 || pl.mac_threads != 256)
        return BFHIP_OK;
    const size_t L = e->L, LL = 2 * L;
    const c2<float> *ring0 = (const c2<float> *)e->d_ring;
    // (a filter delayed by d blocks uses min(P, N - d) partitions: what the derivation cuts, coeff_long_kernel)
    const int P = lwh.P, SL = pl.knobs.long_chunks;
    if (lwh.E % SL != 0) return BFHIP_OK;
    // long chunk c of a group = the whole plan's entries [c E_c, (c + 1) E_c) of it (those of them this
    // engine runs: a shard's entries keep their whole-plan order, its chunks may be shorter)
    const int E_c = lwh.E / SL, PL = (P + 2) / 3;
    std::vector<ChunkRange> lchunks((size_t)pl.n_groups * SL);
    int E_here = 1;
    for (int g = 0; g < pl.n_groups; g++) {
        int idx = chunks[(size_t)g * S].begin;
        const int end = chunks[(size_t)g * S + S - 1].end;
        for (int c = 0; c < SL; c++) {
            ChunkRange cr{idx, idx};
            while (idx < end && lwh.wpos[idx] / E_c == c) idx++;
            cr.end = idx;
            lchunks[(size_t)g * SL + c] = cr;
            E_here = std::max(E_here, cr.end - cr.begin);
        }
        if (idx != end) return BFHIP_OK;
    }
    const int tiles = (int)(LL * sizeof(c2<float>) / 4096u);
    const int n_tc = tiles * SL;
    if (n_tc % 8 != 0) return BFHIP_OK;
    const unsigned int chunk = 256u * 16u;
    const unsigned long long entry_bytes = (unsigned long long)PL * OG * chunk;
    const unsigned long long slice = (unsigned long long)E_here * entry_bytes;
    if (entry_bytes >= (1ull << 31) || slice >= (1ull << 32)) return BFHIP_OK;
    const size_t total = (size_t)((unsigned long long)n_tc * pl.n_groups * slice);
    const bool same_geom = e->b_lstream.p != nullptr && e->lw_chunks == SL && e->lw_P == PL && e->lkeys.size() == flat.size() &&
                           e->lstream.slice == slice;
    if (!same_geom) {
        if (e->b_lstream.grow(total) != hipSuccess) {
            (void)hipGetLastError();
            return BFHIP_OK;                 // no room for the long copy: the standard path
        }
        e->lkeys.assign(flat.size(), std::array<const void *, OG + 1>{});
    }
    // the long entries, and which of them hold other sets (or another delay / length) than last time
    std::vector<MacEntry<float>> lflat(flat);
    std::vector<StreamWhere> where(flat.size());
    std::vector<int> changed;
    for (int g = 0; g < pl.n_groups; g++)
        for (int c = 0; c < SL; c++) {
            const ChunkRange cr = lchunks[(size_t)g * SL + c];
            for (int q = 0; q < cr.end - cr.begin; q++) {
                const int idx = cr.begin + q;
                MacEntry<float> &en = lflat[idx];
                const size_t in = (size_t)(en.ring - ring0) / (e->R * L);
                en.ring = (const c2<float> *)e->d_lring + in * e->R * LL;
                en.shift = 3 * ((en.maxP + 2) / 3) - en.maxP;     // the last partition's (kernels.h)
                en.maxP = (en.maxP + 2) / 3;
                where[idx] = StreamWhere{g, c, q, 0};
                std::array<const void *, OG + 1> key;
                for (int j = 0; j < OG; j++) key[j] = en.term[j].H;
                key[OG] = (const void *)(uintptr_t)(((size_t)(unsigned)en.delay << 32) | (unsigned)P);
                if (key != e->lkeys[idx]) { changed.push_back(idx); e->lkeys[idx] = key; }
            }
        }
    const size_t eb = lflat.size() * sizeof(MacEntry<float>), cb = lchunks.size() * sizeof(ChunkRange);
    const size_t wb = where.size() * sizeof(StreamWhere), ib = flat.size() * sizeof(int);
    HIPCHK(e->b_lentries.grow(eb));
    HIPCHK(e->b_lchunks.grow(cb));
    HIPCHK(e->b_lwhere.grow(wb + ib));
    e->d_lwhich = (int *)((unsigned char *)e->b_lwhere.p + wb);
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    HIPCHK(hipMemcpy(e->b_lentries.p, lflat.data(), eb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->b_lchunks.p, lchunks.data(), cb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->b_lwhere.p, where.data(), wb, hipMemcpyHostToDevice));
    e->lw_chunks = SL; e->lw_P = PL; e->lw_tiles = tiles; e->lw_Pstd = P;
    e->lstream = StreamLayout{(const unsigned char *)e->b_lstream.p, slice, (unsigned int)entry_bytes, chunk,
                              (unsigned int)E_here * OG * chunk};
    if (!changed.empty()) {
        HIPCHK(hipMemcpy(e->d_lwhich, changed.data(), changed.size() * sizeof(int), hipMemcpyHostToDevice));
        const int r = derive_long(e, pl.n_groups, 0, PL, (int)changed.size());
        if (r != BFHIP_OK) { e->lkeys.clear(); return r; }
    }
    e->lw_active = true;
    // the two look-ahead tiers, each if there is room for its buffers (without the first, no second)
    LongGates gt = long_gates(e, lflat, pl.knobs, SL, flat.size() == (size_t)pl.n_groups * (size_t)lwh.E);
    if (gt.la && e->b_ahead.grow((size_t)4 * 3 * pl.n_out_padded * LL * sizeof(c2<float>)) != hipSuccess) {
        (void)hipGetLastError();
        gt.la = gt.far = false;
    }
    e->la_active = gt.la;
    if (gt.far && e->b_far.grow((size_t)7 * LA_FAR * pl.n_out_padded * LL * sizeof(c2<float>)) != hipSuccess) {
        (void)hipGetLastError();
        gt.far = false;                      // one tier
    }
    e->far_active = gt.far;
    if (gt.la && e->blocks_done == 0) return la_prime(e);
    return BFHIP_OK;
}

// ---------------------------------------------------------------- the steps of a build

// lazily loaded coefficient sets: whatever an active filter refers to now has to be on the device
int plan_make_resident(bfhip_engine *e) {
    for (const Filter &f : e->filters) {
        if (!f.active) continue;
        for (int c : {f.coeff, (f.crossfade && f.prevcoeff != f.coeff) ? f.prevcoeff : -1}) {
            if (c < 0 || c >= (int)e->coeffs.size() || e->coeffs[c].d_H != nullptr) continue;
            const int r = coeff_make_resident(e, c);
            if (r != BFHIP_OK) return r;
        }
    }
    return BFHIP_OK;
}

// ring ids order the entries of a group: filters go by the host's own numbering where it gave one,
// so that the order does not depend on the order the filters were added in
long filter_name(const bfhip_engine *e, int fi) { return (long)(e->filters[fi].name >= 0 ? e->filters[fi].name : fi); }

template <typename T> c2<T> *y_of(const bfhip_engine *e, int fi) { return (c2<T> *)e->d_Y + (size_t)e->y_index[fi] * e->L; }

// one filter as plan_collect sees it: where its history lives, how to index it, what it needs
template <typename T> struct FilterView {
    const c2<T> *ring;
    long ring_id;
    int rdelay;
    double rscale;
    int delay, P;
    bool owner;                        // reads a ring of its own (an N-way mix, a cascade, a promoted filter)
    bool fading, needY;                // its output is materialised: a cascade source or a cross-fade
};

// the fill job of a filter with a ring of its own: its inputs and the filter outputs it takes, mixed
template <typename T>
void collect_fill_job(const bfhip_engine *e, Plan<T> &pl, int fi, const FilterView<T> &v) {
    const Filter &f = e->filters[fi];
    const size_t L = e->L;
    FillJob<T> job;
    memset(&job, 0, sizeof(job));
    job.ring = (c2<T> *)v.ring;
    job.delay = v.delay;
    job.n_in = (int)f.in_ch.size();
    job.in_off = (int)pl.srcs.size();
    for (size_t i = 0; i < f.in_ch.size(); i++) {
        MixSrc<T> m;
        m.spec = (const c2<T> *)e->d_ring + (size_t)f.in_ch[i] * e->R * L;
        m.scale = (T)(f.in_scale[i] * e->fmt[0][e->ch.v2p[0][f.in_ch[i]]].scale);      // bfrun.c:1641 (virtscales)
        m.R = e->R;
        pl.srcs.push_back(m);
    }
    job.n_up = (int)f.in_f.size();
    job.up_off = (int)pl.srcs.size();
    for (size_t i = 0; i < f.in_f.size(); i++) {
        MixSrc<T> m;
        m.spec = y_of<T>(e, f.in_f[i]);
        m.scale = (T)f.in_fscale[i];
        m.R = 1;
        pl.srcs.push_back(m);
    }
    job.evalprev = job.n_up > 0 ? (T *)e->d_evalprev + (size_t)e->sink_index[fi] * L : nullptr;
    pl.fills[e->level[fi]].push_back(job);
}

// the job that materialises a filter's output and, in a fade block, the old coefficients' beside it
template <typename T>
void collect_filter_jobs(const bfhip_engine *e, Plan<T> &pl, int fi, const FilterView<T> &v) {
    const Filter &f = e->filters[fi];
    const size_t L = e->L;
    FilterJob<T> job;
    job.ring = v.ring; job.R = v.owner ? e->N : e->R; job.delay = v.rdelay; job.scale = (T)v.rscale;
    job.H = f.coeff < 0 ? nullptr : (const c2<T> *)e->coeffs[f.coeff].d_H;
    job.P = v.P; job.kind = f.coeff < 0 ? TERM_DIRAC : TERM_COEFF;
    job.Y = y_of<T>(e, fi);
    pl.filts[e->level[fi]].push_back(job);
    if (f.coeff >= 0) pl.bytes_H += (double)v.P * (double)L * (double)sizeof(c2<T>);
    if (!v.fading) return;
    // old-coefficient result for the fade (bfrun.c:1726-1769, 1803-1827)
    FilterJob<T> old = job;
    const int pc = f.prevcoeff;
    old.H = pc < 0 ? nullptr : (const c2<T> *)e->coeffs[pc].d_H;
    old.P = pc < 0 ? 1 : cblocks_of(e, pc, v.delay);
    old.kind = pc < 0 ? TERM_DIRAC : TERM_COEFF;
    old.Y = (c2<T> *)e->d_Yold + (size_t)e->fade_index[fi] * L;
    pl.filts[e->level[fi]].push_back(old);
    FadeJob<T> fj;
    fj.Ynew = job.Y; fj.Yold = old.Y;
    pl.fades[e->level[fi]].push_back(fj);
}

// the filter's term in the entry of its (ring, delay) in every output group it feeds
template <typename T>
void collect_outputs(const bfhip_engine *e, Plan<T> &pl, int fi, const FilterView<T> &v) {
    const Filter &f = e->filters[fi];
    const size_t L = e->L;
    const int I = e->n_ch[0];
    for (size_t oi = 0; oi < f.out_ch.size(); oi++) {
        const int o = f.out_ch[oi];
        const int g = o / OG, j = o % OG;
        const double s_out = f.out_scale[oi] / e->fmt[1][e->ch.v2p[1][o]].scale;            // bfrun.c:1850
        const std::pair<long, int> key = v.needY ? std::make_pair((long)(I + pl.n_names + filter_name(e, fi)), 0)
                                                 : std::make_pair(v.ring_id, v.rdelay);
        auto &slots = pl.index[g][key];
        int ei = -1;
        for (int cand : slots) {
            if (pl.per_group[g][cand].term[j].kind == TERM_NONE) { ei = cand; break; }
        }
        if (ei < 0) {
            MacEntry<T> ne;
            memset(&ne, 0, sizeof(ne));
            ne.ring = v.needY ? (f.active ? y_of<T>(e, fi) : nullptr) : v.ring;
            ne.R = v.needY ? 1 : (v.owner ? e->N : e->R);
            ne.delay = v.needY ? 0 : v.rdelay;
            ne.live = (!v.needY && !v.owner && e->d_ps_live) ? e->d_ps_live + v.ring_id : nullptr;
            for (int q = 0; q < OG; q++) ne.term[q].kind = TERM_NONE;
            pl.per_group[g].push_back(ne);
            pl.foreign[g].push_back(0u);
            ei = (int)pl.per_group[g].size() - 1;
            slots.push_back(ei);
        }
        MacTerm<T> &tm = pl.per_group[g][ei].term[j];
        if (!f.active) pl.foreign[g][ei] |= 1u << j;
        if (v.needY) {
            tm.kind = TERM_IDENT; tm.H = nullptr; tm.P = 1; tm.scale = (T)s_out;
        } else {
            tm.kind = f.coeff < 0 ? TERM_DIRAC : TERM_COEFF;
            tm.H = f.coeff < 0 ? nullptr : (const c2<T> *)e->coeffs[f.coeff].d_H;
            tm.P = v.P;
            tm.scale = (T)(v.rscale * s_out);
            if (f.coeff >= 0) {
                pl.bytes_H_plan += (double)v.P * (double)L * (double)sizeof(c2<T>);
                if (f.active) pl.bytes_H += (double)v.P * (double)L * (double)sizeof(c2<T>);
            }
        }
        pl.per_group[g][ei].maxP = std::max(pl.per_group[g][ei].maxP, tm.P);
    }
}

// the filter loop: every filter's level jobs, ring use and MAC terms
template <typename T>
int plan_collect(const bfhip_engine *e, Plan<T> &pl) {
    const int I = e->n_ch[0], F = (int)e->filters.size();
    const size_t L = e->L;
    pl.n_groups = (e->n_ch[1] + OG - 1) / OG;
    pl.n_out_padded = pl.n_groups * OG;
    pl.per_group.resize(pl.n_groups);
    pl.foreign.resize(pl.n_groups);
    pl.index.resize(pl.n_groups);
    pl.fills.resize(e->n_levels);
    pl.filts.resize(e->n_levels);
    pl.fades.resize(e->n_levels);
    pl.n_names = F;
    for (auto &f : e->filters) pl.n_names = std::max(pl.n_names, (long)f.name + 1);

    for (int fi = 0; fi < F; fi++) {
        const Filter &f = e->filters[fi];
        if (f.coeff >= (int)e->coeffs.size()) return fail(BFHIP_EINVAL, "filter %d: bad coeff", fi);
        FilterView<T> v;
        v.delay = clamp_delay(e, f.delayblocks);
        v.P = f.coeff < 0 ? 1 : cblocks_of(e, f.coeff, v.delay);
        // (an inactive filter is classified like an active one -- the plan's shape must not depend
        // on who runs what -- but owns no memory here)
        const bool owner_kind = f.in_ch.size() != 1 || !f.in_f.empty();
        v.owner = f.active ? (e->owner_index[fi] >= 0 || e->promoted[fi] != nullptr)
                           : (owner_kind || e->promoted[fi] != nullptr);
        v.fading = f.crossfade && f.prevcoeff != f.coeff;
        v.needY = e->is_source[fi] || v.fading;
        if (v.fading && f.active) pl.any_fading = true;
        if (v.owner || owner_kind || v.needY) pl.lw_plain = false;        // (every engine sees every filter's state)
        if (f.active && v.needY && e->y_index[fi] < 0) return fail(BFHIP_ESTATE, "filter %d: no output buffer reserved", fi);

        if (v.owner) {
            v.ring = !f.active ? nullptr
                   : e->promoted[fi] ? (const c2<T> *)e->promoted[fi]
                                     : (const c2<T> *)e->d_fring + (size_t)e->owner_index[fi] * e->N * L;
            v.ring_id = I + filter_name(e, fi); v.rdelay = 0; v.rscale = 1.0;
            if (f.active) collect_fill_job(e, pl, fi, v);
        } else {
            const int ch = f.in_ch[0];
            v.ring = (const c2<T> *)e->d_ring + (size_t)ch * e->R * L;
            v.ring_id = ch; v.rdelay = v.delay;
            v.rscale = f.in_scale[0] * e->fmt[0][e->ch.v2p[0][ch]].scale;                         // bfrun.c:1664
        }
        if (f.active) {
            auto &u = pl.ring_used[v.ring_id];
            u.resize(e->N, 0);
            for (int p = 0; p < v.P; p++) u[(p + v.rdelay) % e->N] = 1;
        }
        if (v.needY && f.active) collect_filter_jobs(e, pl, fi, v);
        if (v.needY && f.coeff >= 0) pl.bytes_H_plan += (double)v.P * (double)L * (double)sizeof(c2<T>);
        collect_outputs(e, pl, fi, v);
    }
    return BFHIP_OK;
}

// Canonical entry order inside a group: by (ring, delay), then by the order in which the same
// key was needed again (an output fed twice from one ring).  An output's terms are then summed
// in an order that depends on its own filters only -- not on which other outputs share its
// group, nor on the order the host listed its filters in.
template <typename T>
void plan_order(Plan<T> &pl) {
    for (int g = 0; g < pl.n_groups; g++) {
        std::vector<std::pair<std::pair<std::pair<long, int>, int>, int>> order;     // ((key, n-th use), old index)
        for (auto &kv : pl.index[g])
            for (size_t n = 0; n < kv.second.size(); n++) order.push_back({{kv.first, (int)n}, kv.second[n]});
        std::sort(order.begin(), order.end());
        std::vector<MacEntry<T>> sorted;
        std::vector<unsigned int> fsorted;
        for (auto &o : order) { sorted.push_back(pl.per_group[g][o.second]); fsorted.push_back(pl.foreign[g][o.second]); }
        pl.per_group[g].swap(sorted);
        pl.foreign[g].swap(fsorted);
    }
}

// One-to-one plans (massive_config, BASELINE configs[3]): every entry a single coefficient term,
// every output fed by one entry.  They get mac_diag_kernel -- a workgroup per (chunk, output)
// that walks whole spectra -- and their parallelism from splitting the PARTITIONS of every entry
// into S parts (part c of every entry = chunk c), not from bin tiles.  -> the parts, 0: not such a plan
template <typename T>
int diag_parts(const bfhip_engine *e, const Plan<T> &pl, int bins_per_wg) {
    // (a workgroup holds up to 16 tiles of the spectrum in registers, a job is split over up to 8: 128 tiles)
    if (e->big || (e->L + bins_per_wg - 1) / bins_per_wg > 128 || !pl.knobs.diag) return 0;
    std::vector<char> fed(pl.n_out_padded, 0);
    int n_ent = 0, maxlen = 1;
    for (int g = 0; g < pl.n_groups; g++)
        for (auto &en : pl.per_group[g]) {
            int n_terms = 0, only = -1;
            for (int q = 0; q < OG; q++) if (en.term[q].kind != TERM_NONE) { n_terms++; only = q; }
            if (n_terms != 1 || en.term[only].kind != TERM_COEFF || fed[g * OG + only]) return 0;
            fed[g * OG + only] = 1;
            n_ent++;
            maxlen = std::max(maxlen, en.maxP);
        }
    if (n_ent == 0) return 0;
    // ~512 workgroups keep every CU busy with two; every part costs the output pass one more
    // partial spectrum per channel
    // (workgroups come from splitting a job's SPECTRUM first -- up to 8 runs of tiles, no partial
    // sums -- and only then from parts of the partition axis: config D 256 entries x 2 tile runs)
    const int all_tiles = std::max(1, e->L / bins_per_wg);
    const int per_entry = std::min(all_tiles, 8);
    if (pl.knobs.has_diag_split) return std::max(1, std::min(maxlen, pl.knobs.diag_split));
    return std::max(1, std::min(std::min(4, maxlen), (256 + n_ent * per_entry - 1) / (n_ent * per_entry)));
}

// launch geometry: one fat workgroup per CU measured best on MI355X (tools/tune_mac.py): each
// wave keeps 18 KiB of loads in flight, so 4 waves per CU already saturate HBM, and fewer
// chunks mean fewer partial sums to write and re-read
template <typename T>
void plan_choose_split(const bfhip_engine *e, Plan<T> &pl) {
    pl.mac_threads = std::min(256, std::max(64, e->L / (int)(16 / sizeof(c2<T>))));
    const int bins_per_wg = pl.mac_threads * (int)(16 / sizeof(c2<T>));
    pl.n_tiles = (e->L + bins_per_wg - 1) / bins_per_wg;
    const int s_full = std::max(1, std::min(64, (pl.knobs.target_wgs + pl.n_tiles * pl.n_groups - 1) / (pl.n_tiles * pl.n_groups)));
    pl.S = s_full;
    if (!pl.knobs.has_target_wgs) {
        // every chunk costs the output pass one more partial spectrum to read (~2 us measured);
        // a workgroup streams ~1.35 GB/s per KiB it keeps in flight per wave (2 partitions x
        // (1 ring + n coefficient loads) KiB; 25 GB/s at the crossbar's 18 KiB), the chip
        // ~6.4 TB/s, and a launch is never shorter than ~13 us.  Pick the split that minimises
        // MAC + output-pass time (matters for small crossbars; config C: S = 2).
        double n_terms = 0, n_ent = 0;
        for (auto &v : pl.per_group)
            for (auto &en : v) {
                n_ent += 1;
                for (int q = 0; q < OG; q++) n_terms += en.term[q].kind == TERM_COEFF ? 1 : 0;
            }
        const double rate = 1.35e9 * 2.0 * (1.0 + (n_ent > 0 ? n_terms / n_ent : 1.0));
        double best = 1e30;
        for (int c = 1; c <= s_full; c++) {
            const double wgs = std::min(256.0, (double)pl.n_tiles * pl.n_groups * c);
            const double t_mac = std::max(std::max(13e-6, pl.bytes_H_plan / 6.4e12), pl.bytes_H_plan / (wgs * rate));
            const double t_out = 2e-6 * c;
            if (t_mac + t_out < best - 1e-9) { best = t_mac + t_out; pl.S = c; }
        }
    }
    const int parts = diag_parts(e, pl, bins_per_wg);
    pl.diag_plan = parts > 0;
    if (pl.diag_plan) pl.S = parts;
}

// few filters with many partitions (room correction): split entries along p until every
// group has S work items
template <typename T>
void plan_split_entries(Plan<T> &pl) {
    const int S = pl.S;
    pl.part_of.assign(pl.n_groups, std::vector<int>());
    for (int g = 0; g < pl.n_groups; g++) {
        auto &v = pl.per_group[g];
        if (v.empty()) continue;
        if (!pl.diag_plan && (int)v.size() >= S) continue;
        if (pl.diag_plan && S == 1) continue;
        const int parts = pl.diag_plan ? S : (S + (int)v.size() - 1) / (int)v.size();
        std::vector<MacEntry<T>> split;
        std::vector<unsigned int> fsplit;
        std::vector<int> psplit;
        auto emit = [&](size_t i, int q) {
            const MacEntry<T> &en = v[i];
            const int len = en.maxP;
            const int np = std::max(1, std::min(parts, len));
            if (q >= np) return;
            MacEntry<T> sub = en;
            sub.p0 = (int)((long)len * q / np);
            sub.maxP = (int)((long)len * (q + 1) / np);
            if (sub.maxP > sub.p0) { split.push_back(sub); fsplit.push_back(pl.foreign[g][i]); psplit.push_back(q); }
        };
        if (pl.diag_plan) {
            for (int q = 0; q < parts; q++) for (size_t i = 0; i < v.size(); i++) emit(i, q);      // part-major: chunk c = part c
        } else {
            for (size_t i = 0; i < v.size(); i++) for (int q = 0; q < parts; q++) emit(i, q);
        }
        v.swap(split);
        pl.foreign[g].swap(fsplit);
        if (pl.diag_plan) pl.part_of[g].swap(psplit);
    }
    size_t max_entries = 1;
    for (auto &v : pl.per_group) max_entries = std::max(max_entries, v.size());
    pl.S = std::max(1, std::min<int>(S, (int)max_entries));
}

// the path of every entry: the crossbar (dense 1), one coefficient term (2 + its index), the crossbar
// over a subset of the outputs (16, mask), or the generic path (0)
template <typename T>
void plan_classify(Plan<T> &pl) {
    for (auto &v : pl.per_group) {
        for (auto &en : v) {
            bool dense = en.maxP > en.p0;
            for (int q = 0; q < OG; q++) dense = dense && en.term[q].kind == TERM_COEFF && en.term[q].P >= en.maxP;
            en.dense = dense ? 1 : 0;
            // exactly one coefficient term (one-to-one filters, massive_config style): its own
            // pipelined path, 2 + index of the term
            int n_active = 0, only = -1;
            for (int q = 0; q < OG; q++) if (en.term[q].kind != TERM_NONE) { n_active++; only = q; }
            if (!dense && n_active == 1 && en.term[only].kind == TERM_COEFF && en.maxP > en.p0) en.dense = 2 + only;
            // several (not all OG) coefficient terms of full length: the crossbar path over a subset
            en.mask = 0;
            if (!dense && n_active >= 2 && en.maxP > en.p0) {
                bool ok = true;
                int mask = 0;
                for (int q = 0; q < OG; q++) {
                    if (en.term[q].kind == TERM_NONE) continue;
                    ok = ok && en.term[q].kind == TERM_COEFF && en.term[q].P >= en.maxP;
                    mask |= 1 << q;
                }
                if (ok) { en.dense = 16; en.mask = mask; }
            }
        }
    }
}

// Whether the long-window plan (kernels.h) can take this plan is decided on the WHOLE configuration's
// entries, before foreign terms are taken out: a shard then runs the plan the one-process engine runs,
// and every output is summed in the same order (the subset path rounds like the crossbar path).
template <typename T>
void plan_long_whole(const bfhip_engine *e, Plan<T> &pl) {
    LongWhole &lwh = pl.lwh;
    const size_t L = e->L;
    lwh.ok = e->lw_struct && pl.lw_plain;
    for (int g = 0; g < pl.n_groups && lwh.ok; g++) {
        const auto &v = pl.per_group[g];
        if (g == 0) lwh.E = (int)v.size();
        if ((int)v.size() != lwh.E || v.empty()) lwh.ok = false;
        for (auto &en : v) lwh.P = std::max(lwh.P, en.maxP);
    }
    for (int g = 0; g < pl.n_groups && lwh.ok; g++)
        for (auto &en : pl.per_group[g]) {
            const ptrdiff_t off = (const c2<T> *)en.ring - (const c2<T> *)e->d_ring;
            bool ok = en.dense == 1 && en.p0 == 0 && en.maxP >= 1 && en.maxP == std::min(lwh.P, e->N - en.delay) &&
                      en.live == nullptr && en.R == e->R && en.ring != nullptr && off >= 0 &&
                      off % (ptrdiff_t)(e->R * L) == 0 && off / (ptrdiff_t)(e->R * L) < e->n_ch[0];
            for (int j = 0; j < OG && ok; j++) ok = en.term[j].kind == TERM_COEFF;
            if (!ok) { lwh.ok = false; break; }
        }
}

// chunk boundaries from the WHOLE plan; then the terms of filters another engine runs are taken
// out (an entry's path -- crossbar, single term, generic -- stays the one the whole plan gave it:
// the single-term path rounds differently from the others), entries left empty are dropped
template <typename T>
void plan_flatten(Plan<T> &pl) {
    const int S = pl.S;
    pl.chunks.assign((size_t)pl.n_groups * S, ChunkRange{0, 0});
    for (int g = 0; g < pl.n_groups; g++) {
        const auto &v = pl.per_group[g];
        long total = 0;
        for (auto &en : v) total += en.maxP - en.p0;
        size_t pos = 0;
        long acc = 0;
        for (int c = 0; c < S; c++) {
            ChunkRange cr;
            cr.begin = (int)pl.flat.size();
            const long want = (total * (c + 1) + S - 1) / S;
            // (a one-to-one plan split along p: chunk c is part c of every entry, whatever their lengths)
            const bool by_part = pl.diag_plan && pl.part_of[g].size() == v.size();
            while (pos < v.size() && (by_part ? pl.part_of[g][pos] == c : (acc < want || c == S - 1))) {
                acc += v[pos].maxP - v[pos].p0;
                MacEntry<T> en = v[pos];
                const unsigned int fm = pl.foreign[g][pos];
                pos++;
                if (fm) {
                    unsigned int present = 0;
                    for (int q = 0; q < OG; q++) if (en.term[q].kind != TERM_NONE) present |= 1u << q;
                    const unsigned int keep = present & ~fm;
                    if (keep == 0) continue;                              // nothing of ours in it
                    if (en.dense == 1) { en.dense = 16; en.mask = (int)keep; }
                    else if (en.dense == 16) en.mask &= (int)keep;
                    for (int q = 0; q < OG; q++)
                        if (fm & (1u << q)) { en.term[q].kind = TERM_NONE; en.term[q].H = nullptr; }
                }
                pl.flat.push_back(en);
                pl.lwh.wpos.push_back((int)pos - 1);
            }
            cr.end = (int)pl.flat.size();
            pl.chunks[(size_t)g * S + c] = cr;
        }
    }
    pl.all_dense = !pl.flat.empty();           // every MAC entry takes the crossbar path
    for (auto &en : pl.flat) if (en.dense != 1) pl.all_dense = false;
}

// mac_diag_kernel's job table: the one entry behind every (chunk, output), or -1.  Checked on the
// plan as it came out (unequal filter lengths can put two parts of one entry into one chunk):
// anything unexpected keeps the crossbar kernel, which takes every plan.
template <typename T>
void plan_diag_jobs(Plan<T> &pl) {
    const int S = pl.S;
    pl.mac_diag = pl.diag_plan && !pl.flat.empty();
    if (!pl.mac_diag) return;
    pl.diag_jobs.assign((size_t)S * pl.n_out_padded, -1);
    for (int g = 0; g < pl.n_groups && pl.mac_diag; g++)
        for (int c = 0; c < S && pl.mac_diag; c++) {
            const ChunkRange cr = pl.chunks[(size_t)g * S + c];
            for (int idx = cr.begin; idx < cr.end; idx++) {
                const MacEntry<T> &en = pl.flat[idx];
                if (en.dense < 2 || en.dense >= 2 + OG) { pl.mac_diag = false; break; }
                int &slot = pl.diag_jobs[(size_t)c * pl.n_out_padded + g * OG + (en.dense - 2)];
                if (slot != -1) { pl.mac_diag = false; break; }
                slot = idx;
            }
        }
}

// job arrays for the levelled (non fast-path) filters, one device blob
template <typename T>
void plan_level_blob(const bfhip_engine *e, Plan<T> &pl) {
    auto append = [&](const void *p, size_t n) {
        const size_t off = (pl.blob.size() + 15) & ~(size_t)15;
        pl.blob.resize(off + n);
        if (n) memcpy(pl.blob.data() + off, p, n);
        return off;
    };
    pl.src_off = append(pl.srcs.data(), pl.srcs.size() * sizeof(MixSrc<T>));
    pl.level_jobs.assign(e->n_levels, bfhip_engine::LevelJobs());
    for (int lv = 0; lv < e->n_levels; lv++) {
        auto &lj = pl.level_jobs[lv];
        lj.n_fill = (int)pl.fills[lv].size();
        lj.fill_off = append(pl.fills[lv].data(), pl.fills[lv].size() * sizeof(FillJob<T>));
        lj.n_filt = (int)pl.filts[lv].size();
        lj.filt_off = append(pl.filts[lv].data(), pl.filts[lv].size() * sizeof(FilterJob<T>));
        lj.n_fade = (int)pl.fades[lv].size();
        lj.fade_off = append(pl.fades[lv].data(), pl.fades[lv].size() * sizeof(FadeJob<T>));
    }
}

// the plan's tables to the device, the coefficient layouts that follow from them, the partial-sum ring
template <typename T>
int plan_upload(bfhip_engine *e, const Plan<T> &pl) {
    const size_t L = e->L;
    const size_t eb = pl.flat.size() * sizeof(MacEntry<T>);
    const size_t cb = pl.chunks.size() * sizeof(ChunkRange);
    const size_t db = pl.mac_diag ? pl.diag_jobs.size() * sizeof(int) : 0;
    HIPCHK(e->b_entries.grow(std::max(eb, sizeof(MacEntry<T>))));
    HIPCHK(e->b_chunks.grow(cb + db));
    HIPCHK(e->b_jobs.grow(pl.blob.size()));
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    if (eb) HIPCHK(hipMemcpy(e->b_entries.p, pl.flat.data(), eb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->b_chunks.p, pl.chunks.data(), cb, hipMemcpyHostToDevice));
    e->d_diag_jobs = nullptr;
    if (pl.mac_diag) {
        e->d_diag_jobs = (const int *)((const unsigned char *)e->b_chunks.p + cb);
        HIPCHK(hipMemcpy((void *)e->d_diag_jobs, pl.diag_jobs.data(), db, hipMemcpyHostToDevice));
    }
    if (!pl.blob.empty()) HIPCHK(hipMemcpy(e->b_jobs.p, pl.blob.data(), pl.blob.size(), hipMemcpyHostToDevice));
    {   // stream-ordered coefficient copy (StreamLayout) for uniform crossbar plans
        const int r = build_stream_layout<T>(e, pl);
        if (r != BFHIP_OK) return r;
    }
    e->lw_active = false;
    e->la_active = e->far_active = false;
    e->la_epoch++;
    if constexpr (std::is_same<T, float>::value) {
        const int r = build_long_layout(e, pl);
        if (r != BFHIP_OK) return r;
    }
    size_t zb = (size_t)pl.S * pl.n_out_padded * L * sizeof(c2<T>);
    if (e->lw_active) zb = std::max(zb, (size_t)e->lw_chunks * pl.n_out_padded * 2 * L * sizeof(c2<T>));
    if (zb > e->zp_bytes) {
        for (void *&z : e->d_Zp) { if (z) (void)hipFree(z); z = nullptr; }
        for (int i = 0; i < zp_depth(e); i++) HIPCHK(dev_alloc(&e->d_Zp[i], zb));
        for (bool &z : e->zp_long) z = false;
        e->zp_bytes = zb;
        e->zp_last = 0;
    }
    return BFHIP_OK;
}

// the uploaded plan becomes the engine's: its geometry (here and nowhere else), what a block moves
template <typename T>
void plan_commit(bfhip_engine *e, const Plan<T> &pl) {
    e->n_groups = pl.n_groups; e->n_out_padded = pl.n_out_padded;
    e->n_chunks = pl.S; e->n_tiles = pl.n_tiles; e->mac_threads = pl.mac_threads;
    e->n_entries = (int)pl.flat.size();
    e->mac_nt = pl.knobs.mac_nt; e->mac_unroll = pl.knobs.mac_unroll;
    e->all_dense = pl.all_dense; e->mac_diag = pl.mac_diag; e->any_fading = pl.any_fading;
    e->level_jobs = pl.level_jobs; e->src_off = pl.src_off;
    // algorithmic bytes per block, SURVEY 8(d): C*(F*P + U*P + U + O) + (I+O)*L*s_raw
    const double C = (double)e->L * sizeof(c2<T>);
    double bytes_ring = 0, raw = 0;
    for (auto &kv : pl.ring_used) for (char u : kv.second) bytes_ring += u ? C : 0;
    for (int io = 0; io < 2; io++)
        for (int c = 0; c < e->ch.n_phys[io]; c++) raw += (double)e->L * e->fmt[io][c].bytes;
    int O_here = 0;
    for (int o = 0; o < e->n_ch[1]; o++) O_here += e->out_active.empty() || e->out_active[o] ? 1 : 0;
    e->alg_bytes_mac = pl.bytes_H + bytes_ring + C * O_here;
    e->alg_bytes_total = e->alg_bytes_mac + C * (e->n_ch[0] + e->n_owners) + raw;
    e->plan_dirty = false;
}

template <typename T>
int build_plan_t(bfhip_engine *e) {
    Plan<T> pl;
    pl.knobs = read_knobs(e);
    { const int r = plan_make_resident(e); if (r != BFHIP_OK) return r; }
    { const int r = plan_collect(e, pl); if (r != BFHIP_OK) return r; }
    plan_order(pl);
    plan_choose_split(e, pl);
    plan_split_entries(pl);
    plan_classify(pl);
    plan_long_whole(e, pl);
    plan_flatten(pl);
    plan_diag_jobs(pl);
    plan_level_blob(e, pl);
    { const int r = plan_upload(e, pl); if (r != BFHIP_OK) return r; }
    plan_commit(e, pl);
    return BFHIP_OK;
}

}  // namespace

BFHIP_HOST_NS {

int clamp_delay(const bfhip_engine *e, int d) {          // bfrun.c:1579-1584
    if (d < 0) return 0;
    if (d > e->N - 1) return e->N - 1;
    return d;
}

int cblocks_of(const bfhip_engine *e, int coeff, int delay) {   // bfrun.c:1585-1591
    if (coeff < 0 || e->coeffs[coeff].n_blocks > e->N - delay) return e->N - delay;
    return e->coeffs[coeff].n_blocks;
}

int build_plan(bfhip_engine *e) {
    return e->rs == 4 ? build_plan_t<float>(e) : build_plan_t<double>(e);
}

// standard partition `block` of set H changed in place: long partition block / 3 of every long entry
// that uses H (or, with no long plan in force now, forget that those entries hold H)
int long_refresh_block(bfhip_engine *e, const void *H, int block) {
    e->la_epoch++;                 // products of the rewritten partition may be stored ahead
    if (e->lkeys.empty()) return BFHIP_OK;
    std::vector<int> hit;
    for (size_t i = 0; i < e->lkeys.size(); i++)
        for (int j = 0; j < OG; j++) if (e->lkeys[i][j] == H) { hit.push_back((int)i); break; }
    if (hit.empty()) return BFHIP_OK;
    if (!e->lw_active || e->plan_dirty || block / 3 >= e->lw_P) {
        for (int i : hit)
            for (int j = 0; j < OG; j++) if (e->lkeys[i][j] == H) e->lkeys[i][j] = STREAM_KEY_STALE;
        return BFHIP_OK;
    }
    { int _r = sync_all(e); if (_r != BFHIP_OK) return _r; }
    HIPCHK(hipMemcpy(e->d_lwhich, hit.data(), hit.size() * sizeof(int), hipMemcpyHostToDevice));
    return derive_long(e, e->n_groups, block / 3, 1, (int)hit.size());
}

// one partition of a coefficient set changed in place (update_coeff_block, refresh of a watched
// set): bring the stream-ordered copy up to date
template <typename T>
int stream_refresh_block(bfhip_engine *e, const void *H, int block) {
    if constexpr (std::is_same<T, float>::value) {
        const int r = long_refresh_block(e, H, block);
        if (r != BFHIP_OK) return r;
    }
    if (e->hstream.base == nullptr || e->plan_dirty) {
        // no copy now (the plan is about to be rebuilt, or this block runs without the stream-ordered
        // copy: a cross-fade block).  The rebuild compares entries by their set POINTERS, which an
        // in-place rewrite does not change: forget that these entries hold H, so that the next
        // build_stream_layout lays them out again from the new data.
        for (auto &k : e->stream_keys)
            for (int j = 0; j < OG; j++) if (k[j] == H) k[j] = STREAM_KEY_STALE;
        return BFHIP_OK;
    }
    std::vector<int> hit;
    for (size_t i = 0; i < e->stream_keys.size(); i++)
        for (int j = 0; j < OG; j++) if (e->stream_keys[i][j] == H) { hit.push_back((int)i); break; }
    if (hit.empty()) return BFHIP_OK;
    const int P = e->stream_geom[2];
    if (block >= P) return BFHIP_OK;
    HIPCHK(hipMemcpy(e->d_which, hit.data(), hit.size() * sizeof(int), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(stream_relayout_kernel<T>, dim3(1u, (unsigned)e->n_tiles, (unsigned)hit.size()), dim3(256), 0, e->stream,
                       (const MacEntry<T> *)e->b_entries.p, (const StreamWhere *)e->b_where.p, (const int *)e->d_which,
                       block, e->L, e->n_groups, e->n_chunks, e->hstream);
    HIPCHK(hipGetLastError());
    return sync_all(e);
}
template int stream_refresh_block<float>(bfhip_engine *, const void *, int);
template int stream_refresh_block<double>(bfhip_engine *, const void *, int);

}  // namespace bfhip_host
