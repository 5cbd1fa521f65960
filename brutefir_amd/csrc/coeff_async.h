// coeff_async.h -- the engine half of the non-uniform convolver's asynchronous set rewrite
// (bfhip_nupc_update_coeff_async, include/bfhip_nupc.h).  Internal to libbfhip.so: defined in
// bfhip.hip, called from nupc_update.hip.  bfhip_engine_update_coeff_block (include/bfhip.h) is the
// synchronous, one-partition counterpart.
#pragma once
#include "../../include/bfhip.h"

extern "C" {
// after finalize, off the audio path: allocates what the rewrite below would otherwise need lazily
// (the big-FFT scratch for all N partitions of an engine above 8192)
int bfhip_internal_engine_reserve_update(bfhip_engine *e);
// partitions [0, n_blocks) of resident set `coeff` from n_taps reals at taps_dev (zero-padded), by
// one K7 launch (or the big-FFT sequence) on the engine's stream, in order with its blocks.  No
// host wait, no allocation, no blocking copy.  The non-finite flag goes to *bad_host (pinned) behind
// the preparation.  The set must be idle: no block handed in after this call may read it before a
// filter is pointed at it again.
int bfhip_internal_engine_update_coeff_dev_async(bfhip_engine *e, int coeff, const void *taps_dev, int n_taps,
                                                 int n_blocks, int *bad_host);
}
