// nupc_loudness.h -- the kernel of the BS.1770 loudness meter (bfhip_nupc_enable_loudness; the definition is in
// include/bfhip_nupc.h and, frame by frame, in loudness_host.h) and the host wrapper that launches it.  Included
// by nupc.hip only, behind nupc_kernels.h.
#pragma once
#include "nupc_kernels.h"

namespace {

// Where the plain walk ends and the chunked scan begins: one lane walking 64 or 128 frames per
// member takes the launch 15.9 and 25.9 us, the scan over 16-frame chunks 13.1 us at L0 = 256 and 15.8 us at 2048.
// The walk is kept up to 128 frames, the sizes a low-latency first block has, although the scan would save a few
// microseconds there: it does the definition's arithmetic in the definition's order.  The high-pass has an almost
// double pole (Q = 0.5003), so the decay rate of its free response is sensitive to rounding: carried by the scan's
// matrix powers, the tail of a programme that falls silent drifts from the frame-by-frame walk by some 1e-10
// relative per chunk -- 7e-8 in E once E has fallen below 1e-250 of full scale, measured at L0 = 64 -- where the
// walk stays within an ulp or so of it.
constexpr int kLoudSerialMax = 128;    // periods up to here: one lane per member walks the whole period
constexpr int kLoudChunk = 16;         // longer ones: frames per lane of the chunked scan
constexpr int kLoudLanes = 256;
constexpr int kLoudBlock = 16;         // frames a lane reads from LDS ahead of its recursion
// LDS of the launch beside its static arrays: one member's tile of decoded samples, float64, a chunk's frames
// followed by one cell of padding (lane p walks cells p (C + 1) ..: C + 1 doubles apart, no bank in common)
static size_t nupc_loud_lds(int L0, int C) {
    const int cnt = std::min(L0, kLoudLanes * C);
    return (size_t)(cnt + cnt / C + 1) * sizeof(double);
}
// a chunk lies in at most two sub-blocks: S >= kLoudRateMin / 10
static_assert(kLoudChunk % kLoudBlock == 0, "a full chunk is whole blocks");
static_assert(kLoudSerialMax <= kLoudRateMin / 10 && kLoudChunk <= kLoudRateMin / 10, "a chunk must not span a whole sub-block");

// an aligned sample of BYTES bytes, loaded as one word: what load_raw's fast paths make of it
template <int BYTES> __device__ __forceinline__ double loud_word(uint64_t w, const DevFormat &f) {
    if (BYTES == 8) {
        if (f.swap) w = __builtin_bswap64(w);
        return f.isfloat ? __longlong_as_double((long long)w) : (double)(int32_t)(uint32_t)w;
    }
    if (BYTES == 4) {
        uint32_t lo = (uint32_t)w;
        if (f.swap) lo = __builtin_bswap32(lo);
        return f.isfloat ? (double)__uint_as_float(lo) : (double)(int32_t)lo;
    }
    uint16_t h = (uint16_t)w;
    if (f.swap) h = __builtin_bswap16(h);
    return (double)(int16_t)h;
}

// cnt samples of one channel -- load_raw<double> times the format's scale, a value that is not finite as 0 -- into
// vv, frame i in cell i + i / C, by the whole workgroup.  Naturally aligned words take load_raw's fast paths with
// eight loads in flight per lane; everything else goes through load_raw sample by sample.
template <int BYTES, typename W>
__device__ __forceinline__ void loud_stage_words(double *vv, const uint8_t *base, size_t stride, const DevFormat &f, double scale,
                                                 int cnt, int C, int tid) {
    for (int i0 = tid; i0 < cnt; i0 += kLoudLanes * 8) {
        W w[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const int i = min(i0 + u * kLoudLanes, cnt - 1); w[u] = *reinterpret_cast<const W *>(base + (size_t)i * stride); }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int i = i0 + u * kLoudLanes;
            const double v = loud_word<BYTES>((uint64_t)w[u], f) * scale;
            if (i < cnt) vv[i + i / C] = isfinite(v) ? v : 0.0;
        }
    }
}
__device__ __forceinline__ void loud_stage(double *vv, const uint8_t *base, size_t stride, const DevFormat &f, double scale, int cnt,
                                           int C, int tid) {
    const bool words = f.bytes > 0 && ((uintptr_t)base % (unsigned)f.bytes) == 0 && stride % (unsigned)f.bytes == 0;
    if (words && f.bytes == 8) loud_stage_words<8, uint64_t>(vv, base, stride, f, scale, cnt, C, tid);
    else if (words && f.bytes == 4) loud_stage_words<4, uint32_t>(vv, base, stride, f, scale, cnt, C, tid);
    else if (words && f.bytes == 2 && !f.isfloat) loud_stage_words<2, uint16_t>(vv, base, stride, f, scale, cnt, C, tid);
    else
        for (int i = tid; i < cnt; i += kLoudLanes) {
            const double v = load_raw<double>(base + (size_t)i * stride, f) * scale;
            vv[i + i / C] = isfinite(v) ? v : 0.0;
        }
}

// One workgroup per group, one launch per period, on the raw block that leaves the convolver.  The period is taken
// in tiles of 256 chunks of C frames (C = L0: one chunk, one lane, a plain walk); the members take turns, in the
// group's order, each through the whole workgroup:
//   stage    the tile's samples, decoded with load_raw and scaled, into LDS: adjacent lanes take adjacent frames, and
//            no recursion waits for a load from global memory
//   pass 1   lane p walks chunk p from zero state (lane 0: from the member's saved state) -> the chunk's end state
//   scan     end[p] = M end[p - 1] + zero-state end[p], M the transition over C frames of zero input: a log-step
//            scan through LDS with the host's M^(2^i)
//   pass 2   lane p walks chunk p again from end[p - 1], squares and sums -- into two partials where a sub-block
//            boundary falls inside the chunk
//   fold     per sub-block the tile touches, the lanes' partials go down a fixed tree (shuffles, then the four waves'
//            totals) and the member's weighted sum is added to the sub-block's energy: the members in ascending
//            order, no atomics, the same bits every run
// Both passes read a block of samples from LDS into registers before they walk it: the recursion waits for its own
// two multiply-adds per frame and section, not for a load.
// and behind the last member the sub-blocks that end inside the tile go to the ring, the one still open to the
// partial.  Frame t of the period is frame `pos` + t of sub-block j0 (and on from there).
__global__ __launch_bounds__(256) void
nupc_loudness_kernel(const uint8_t *__restrict__ raw, const DevFormat *__restrict__ fmt,
                     const NupcLoudGroup *__restrict__ groups, double *__restrict__ state, double *__restrict__ open,
                     double *__restrict__ ring, int H, int L0, int S, int C, long long j0, int pos, const NupcLoudCoef co) {
    __shared__ double st[kLoudGroupMax][4];
    __shared__ double zs[kLoudLanes][4];
    __shared__ double wave_sum[2][4];
    __shared__ double seg_e[kLoudLanes + 1];
    __shared__ double open_s;
    extern __shared__ __attribute__((aligned(16))) unsigned char loud_smem[];
    double *vv = reinterpret_cast<double *>(loud_smem);
    const int g = blockIdx.x, tid = threadIdx.x;
    const NupcLoudGroup *grp = groups + g;
    const int n_ch = grp->n_ch;
    if (tid < n_ch * 4) st[tid >> 2][tid & 3] = state[((size_t)g * kLoudGroupMax + (tid >> 2)) * 4 + (tid & 3)];
    if (tid == 0) open_s = open[g];
    const int tile = kLoudLanes * C;
    for (int t0 = 0; t0 < L0; t0 += tile) {
        const int cnt = min(tile, L0 - t0), P = (cnt + C - 1) / C;
        const long long at = (long long)pos + t0;
        const int tpos = (int)(at % S);                     // the tile's first frame inside its sub-block
        const long long tj = j0 + at / S;                   // and that sub-block's number
        const int nseg = (tpos + cnt - 1) / S + 1;          // sub-blocks the tile touches: <= P + 1
        for (int q = tid; q < nseg; q += kLoudLanes) seg_e[q] = 0.0;
        __syncthreads();                                    // st, open_s, seg_e
        const int n0 = tid * C, n1 = min(n0 + C, cnt);
        for (int k = 0; k < n_ch; k++) {
            const double w = grp->weight[k];
            if (w == 0.0) continue;                         // contributes exactly nothing (the whole workgroup skips)
            const DevFormat f = fmt[grp->ch[k]];
            const uint8_t *base = raw + f.byte_offset + (size_t)t0 * f.sample_spacing * f.bytes;
            const size_t stride = (size_t)f.sample_spacing * f.bytes;
            loud_stage(vv, base, stride, f, grp->scale[k], cnt, C, tid);
            __syncthreads();
            const double *mine = vv + tid;                  // frame n of this lane's chunk: cell n + n / C = n + tid
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            if (tid == 0) { s[0] = st[k][0]; s[1] = st[k][1]; s[2] = st[k][2]; s[3] = st[k][3]; }
            const double from[4] = {s[0], s[1], s[2], s[3]};       // lane 0 keeps it: the last lane overwrites st[k]
            if (P > 1) {
                if (tid < P) {
                    // (a chunk that ends early is the tile's last: nobody starts from its end state)
                    for (int b = n0; b < n1; b += kLoudBlock) {
                        double x[kLoudBlock];
#pragma unroll
                        for (int u = 0; u < kLoudBlock; u++) x[u] = mine[min(b + u, n1 - 1)];
#pragma unroll
                        for (int u = 0; u < kLoudBlock; u++) (void)kweighting_step(co.c, s, x[u]);
                    }
                    zs[tid][0] = s[0]; zs[tid][1] = s[1]; zs[tid][2] = s[2]; zs[tid][3] = s[3];
                }
                __syncthreads();
                for (int i = 0, d = 1; d < P; i++, d <<= 1) {
                    const bool on = tid < P && tid >= d;
                    double add[4] = {0.0, 0.0, 0.0, 0.0};
                    if (on) {
                        const double *m = co.mp[i], *z = zs[tid - d];
#pragma unroll
                        for (int r = 0; r < 4; r++) add[r] = m[r * 4] * z[0] + m[r * 4 + 1] * z[1] + m[r * 4 + 2] * z[2] + m[r * 4 + 3] * z[3];
                    }
                    __syncthreads();
                    if (on) { zs[tid][0] += add[0]; zs[tid][1] += add[1]; zs[tid][2] += add[2]; zs[tid][3] += add[3]; }
                    __syncthreads();
                }
                if (tid > 0 && tid < P) { s[0] = zs[tid - 1][0]; s[1] = zs[tid - 1][1]; s[2] = zs[tid - 1][2]; s[3] = zs[tid - 1][3]; }
                else { s[0] = from[0]; s[1] = from[1]; s[2] = from[2]; s[3] = from[3]; }
            }
            // frames of the chunk in the sub-block its first frame lies in (qa), and in the next one
            double sum_a = 0.0, sum_b = 0.0;
            const int qa = (tpos + n0) / S;
            if (tid < P) {
                const int split = min(n1, (qa + 1) * S - tpos);
                for (int b = n0; b < n1; b += kLoudBlock) {
                    double x[kLoudBlock];
#pragma unroll
                    for (int u = 0; u < kLoudBlock; u++) x[u] = mine[min(b + u, n1 - 1)];
#pragma unroll
                    for (int u = 0; u < kLoudBlock; u++) {
                        if (b + u < n1) {                   // (b, n1 and split are the same for all but the last lane)
                            const double z = kweighting_step(co.c, s, x[u]);
                            if (b + u < split) sum_a += z * z; else sum_b += z * z;
                        }
                    }
                }
                if (tid == P - 1) { st[k][0] = s[0]; st[k][1] = s[1]; st[k][2] = s[2]; st[k][3] = s[3]; }
            }
            // fold: per sub-block of the tile the lanes' partials (0 from a lane that has none) down a fixed tree,
            // the waves' four totals added in one order by lane 0
            for (int q = 0; q < nseg; q++) {
                double x = tid < P ? (qa == q ? sum_a : qa == q - 1 ? sum_b : 0.0) : 0.0;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
                if ((tid & 63) == 0) wave_sum[q & 1][tid >> 6] = x;
                __syncthreads();
                if (tid == 0) seg_e[q] += w * ((wave_sum[q & 1][0] + wave_sum[q & 1][1]) + (wave_sum[q & 1][2] + wave_sum[q & 1][3]));
            }
            __syncthreads();                                // vv, zs and st[k] are free for the next member
        }
        const double open_in = open_s;                      // behind a barrier, whether or not a member ran
        __syncthreads();                                    // every lane has it: the last sub-block's lane may write
        for (int q = tid; q < nseg; q += kLoudLanes) {
            const double e = q == 0 ? open_in + seg_e[0] : seg_e[q];
            const bool closes = (q + 1) * S - tpos <= cnt;
            if (closes) ring[(size_t)g * H + (size_t)((tj + q) % H)] = e;
            if (q == nseg - 1) open_s = closes ? 0.0 : e;
        }
        __syncthreads();
    }
    if (tid < n_ch * 4) state[((size_t)g * kLoudGroupMax + (tid >> 2)) * 4 + (tid & 3)] = st[tid >> 2][tid & 3];
    if (tid == 0) open[g] = open_s;
}

// this period's launch: the sub-block counter and the position inside the open sub-block come from the host's
// frame counter, so nothing is uploaded or read back
int nupc_loudness(bfhip_nupc *n, unsigned long long opos, const void *rawout_dev) {
    NupcLoudness &ld = n->loud;
    hipLaunchKernelGGL(nupc_loudness_kernel, dim3((unsigned)ld.groups.size()), dim3(kLoudLanes), nupc_loud_lds(n->L0(), ld.chunk), n->stream,
                       (const uint8_t *)rawout_dev, n->io.d_fmt[1], ld.d_groups, ld.d_state, ld.d_open, ld.d_ring,
                       ld.history, n->L0(), ld.S, ld.chunk, (long long)(opos / (unsigned long long)ld.S),
                       (int)(opos % (unsigned long long)ld.S), ld.coef);
    NCHK(hipGetLastError());
    return BFHIP_OK;
}

}  // namespace
