// passes.h -- the passes of a block and the engine's other kernel launches (passes.hip): which kernel runs,
// with which arguments.  When, and on which stream (e->ls), is the caller's business: the schedules, the
// coefficient store and real-time mode of bfhip.hip.  Internal: nothing here is part of include/.
#pragma once
#include "engine.h"

BFHIP_HOST_NS {

// event records of a timed block's stage on e->ls (nothing while the block is not timed or a graph is captured)
int record_begin(bfhip_engine *e, int stage);
int record_end(bfhip_engine *e, int stage);

// blocks the rings will hold of the block `ahead` after this one, itself included (procblocks, bfrun.c:1745)
int block_age(const bfhip_engine *e, int ahead = 0);
// scratch of the transforms above 8192 points for n_tr of them; waits for the device when it has to grow
int big_reserve(bfhip_engine *e, size_t n_tr);

// ---- a block, each pass on e->ls
// channel stage and forward transforms of the block `ahead` after the counter's (block pairs: 1)
int do_inputs(bfhip_engine *e, const void *rawin_dev, unsigned int ahead = 0u);
// the per-filter kernels in front of the MAC (N-way mixes, cascades, cross-fades), timed as T_LEVELS
int do_levels(bfhip_engine *e);
// the MAC into the partial sums Zp; may_long: the long-window plan may cover the block (not the phase calls)
int do_mac(bfhip_engine *e, void *Zp, bool may_long = true);
// this block and the next in one pass over the coefficients (mac_xbar2_kernel)
int do_mac_pair(bfhip_engine *e, void *Zp0, void *Zp1);
// the sum over the chunks of Zp into Z (Z == Zp: in place, into chunk 0)
int sum_chunks(bfhip_engine *e, const void *Zp, void *Z);
// inverse transforms of outputs [first, first + count) and the channel stage behind them
int do_outputs(bfhip_engine *e, const void *Zp, size_t chunk_stride, int n_chunks, int first, int count,
               void *rawout_dev);
// [K3 of an owed block | K1 of this block] in one launch; callers take this path only when the channel stage is
// plain(), so that its two calls add nothing around the launch but the transposes of wide sides, and never
// above 8192 points.  The LDS transform reads one spectrum per output (n_chunks == 1: the phase calls).
int fused_outputs_inputs(bfhip_engine *e, const void *Zp, size_t chunk_stride, int n_chunks, int first, int count,
                         void *rawout_dev, const void *rawin_dev);

// ---- coefficients, on e->stream
// n_blocks partitions H from n_taps reals in device memory (zero-padded); reserves the scratch it needs
int coeff_prep(bfhip_engine *e, const void *taps_dev, int n_taps, double scale, void *H, int n_blocks);
// n_blocks partitions between the reference's layout (taps: 2L reals each) and the packed one (H)
int coeff_reorder(bfhip_engine *e, void *taps, void *H, int n_blocks, bool to_packed);
// the last n_valid blocks of an input's ring, delayed and scaled, into a filter's private ring
int promote_ring(bfhip_engine *e, const void *src, void *ring, int delay, double scale, int n_valid);

// ---- real-time mode, on e->stream
int rt_copy_in(bfhip_engine *e, const RtCopy &in);
// `grid` workgroups: copy out, advance the device's block state, period p's overflow, status and arrival words
int rt_tail(bfhip_engine *e, unsigned int grid, const RtCopy &out, int p);

}  // namespace bfhip_host
