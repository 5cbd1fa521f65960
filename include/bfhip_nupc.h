/*
 * bfhip_nupc.h -- non-uniform partitioned convolution (low-latency first block) on top of the
 * uniform engines of bfhip.h.  An EXTENSION beyond the reference, which only supports uniform
 * partitions (`filter_length: L,N`, bfconf.c:1495-1520): BASELINE.json's room-correction
 * configuration asks for it.  Results are the linear convolution a uniform run computes; only
 * the I/O block -- the latency -- shrinks from L to the smallest segment length.
 *
 * The impulse response is cut into segments; segment k has partition length seg_length[k]
 * (ascending powers of two, each a multiple of the previous) and seg_blocks[k] partitions and
 * covers the taps after the previous segments.  I/O happens in blocks of seg_length[0] frames.
 * Segment k must start at a tap >= seg_length[k] - seg_length[0] so that its result is ready
 * when needed (checked); "2 x 64, 2 x 128, 2 x 256, ..." style schedules satisfy it.
 *
 * Scheduling: a segment whose first output frame is due later than the period it is launched in
 * (every segment but the first in the doubling schedule) runs on its own low-priority stream
 * beside the periods that follow; the main stream waits for it only when its output is due, so
 * the longest period costs about what the common one does (tools/nupc_latency.py).
 *
 * Filters are single-input single-output impulse responses (a crossbar is one call per pair).
 *
 * Raw I/O buffers hold one period of seg_length[0] (L0) frames per side, in one of two layouts:
 *   - Interleaved frames (the default; dai.c's layout of one interleaved device): all channels of
 *     the side share sample_spacing and bytes, a frame is sample_spacing * bytes bytes and the
 *     buffer is L0 frames.  The input frames go straight into a raw ring that the segments read.
 *   - A declared buffer (bfhip_nupc_set_buffer_bytes, per side): every channel has its own
 *     byte_offset, sample_spacing and sample format -- dai.c's period buffer for any set of devices
 *     laid back to back, interleaved or not (calc_buffer_format, dai.c:537-576): planes as JACK
 *     delivers them, two sound cards with different sample widths.  Such an input period is staged
 *     on the device, delayed and muted in place and converted once into the ring of reals the
 *     segments read; the results are those of the interleaved path, bit for bit.
 */
#ifndef BFHIP_NUPC_H
#define BFHIP_NUPC_H

#include "bfhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bfhip_nupc bfhip_nupc;

const char *bfhip_nupc_last_error(void);
bfhip_nupc *bfhip_nupc_create(int device, int realsize, int n_in, int n_out, int n_segments,
                              const int seg_length[], const int seg_blocks[]);
void bfhip_nupc_destroy(bfhip_nupc *n);
long bfhip_nupc_taps(const bfhip_nupc *n);        /* taps covered by the schedule */
int bfhip_nupc_latency(const bfhip_nupc *n);      /* I/O block size in frames = seg_length[0] */
/* before finalize (BFHIP_ESTATE after): sample format and place of one raw channel in the side's
   period buffer; sample t (0 <= t < L0) lies at byte_offset + t * sample_spacing * bytes.  On a
   side that does not declare its buffer all channels must share sample_spacing and bytes (one
   interleaved frame layout; checked at finalize) and the buffer is L0 * sample_spacing * bytes
   long.  On a side that does (below) every channel is on its own. */
int bfhip_nupc_set_format(bfhip_nupc *n, int io, int channel, const bfhip_format *bf);
/* before finalize (BFHIP_ESTATE after); bytes >= 1, io BFHIP_IN / BFHIP_OUT (BFHIP_EINVAL otherwise,
   NULL handle included).  Declares side io's period buffer to be `bytes` long with every channel
   laid out on its own: sample t (0 <= t < L0) of channel c lies at
   byte_offset_c + t * sample_spacing_c * bytes_c, bytes_c wide -- dai.c's buffer for any set of
   devices (interleaved or not, one sample format each).  Finalize then checks, per channel and with
   BFHIP_EINVAL and a message naming it: sample_spacing >= 1, byte_offset >= 0, the last sample
   inside the buffer, and no byte shared with another channel of the side; there is no alignment
   rule.  An input side that declares its buffer has at most 256 channels.
   Every call keeps its documented semantics per channel: block and block_dev, the overflow structs,
   dither, gains and ramps, switches and cross-fades, integer delay and mute, sub-sample delay.
   Bytes of the output buffer that no channel owns (like the gap bytes of gapped frames):
   bfhip_nupc_block returns them as zero, bfhip_nupc_block_dev does not touch them.
   bfhip_nupc_block_dev never modifies the caller's input buffer on either kind of side.
   Cost: one copy into the stage and one conversion launch per period on an input side that
   declares its buffer, nothing on the output side.  A convolver that never
   calls this allocates, launches and computes exactly as before. */
int bfhip_nupc_set_buffer_bytes(bfhip_nupc *n, int io, long bytes);
/* after finalize: bytes of one period buffer of the side, whichever way it was declared
   (L0 * sample_spacing * bytes for a side that did not opt in); BFHIP_ESTATE before finalize,
   BFHIP_EINVAL on a NULL handle or bad io */
long bfhip_nupc_buffer_bytes(const bfhip_nupc *n, int io);
int bfhip_nupc_set_safety_limit(bfhip_nupc *n, double limit);
int bfhip_nupc_add_filter(bfhip_nupc *n, int in_channel, int out_channel, const void *taps,
                          long n_taps, double in_scale, double out_scale);
int bfhip_nupc_finalize(bfhip_nupc *n);
/* one I/O block of seg_length[0] frames; host buffers, synchronous; returns status bits
   (BFHIP_ST_*) or a negative error */
int bfhip_nupc_block(bfhip_nupc *n, const void *rawin, void *rawout, bfhip_overflow overflow[]);
/* device-resident buffers, asynchronous on the convolver's stream */
int bfhip_nupc_block_dev(bfhip_nupc *n, const void *rawin_dev, void *rawout_dev);
/* waits for the periods handed in so far and returns the status bits collected since the last
   call (background segment blocks that are not due yet keep running) */
int bfhip_nupc_sync(bfhip_nupc *n);
int bfhip_nupc_get_overflow(bfhip_nupc *n, int out_channel, bfhip_overflow *of);

/* HP-TPDF dither (dither.c, dither_funs.h:7-69) on the listed outputs, with dither_init()'s
   parameters, like bfhip_engine_enable_dither; before finalize (BFHIP_ESTATE after).  Channels
   ascending and in range, integer output formats only (set the formats first), sample_rate >= 1;
   a max_size too small for the table fails with the reference's message.  The table spacing uses
   max_samples_per_loop = seg_length[0], and the table walk advances seg_length[0] samples per
   block call: the output equals what the reference produces with a period of seg_length[0] frames.
   The dither input is the value the output would be quantised from without dither (cross-fade
   blend, output gain and 1/scale applied), so gain 0 gives dithered silence.  Non-finite and
   safety-limit samples are skipped and reported as BFHIP_ST_* bits by the same block call.
   Runs inside the emit step: no launch of its own. */
int bfhip_nupc_enable_dither(bfhip_nupc *n, const int out_channels[], int n_ch, int sample_rate, int max_size);

/* ---- run-time control: coefficient switches (cfc) and output gain (cfoa) ------------------
 * Filters are numbered 0, 1, ... in add_filter order.  Each filter can hold several impulse
 * responses ("sets"); set 0 is add_filter's taps.  A switch changes which set filters run.
 *
 * Switch frame.  Output frames are counted from the convolver's first output frame: block call
 * b emits frames [b*L0, (b+1)*L0).  Requests queued by bfhip_nupc_set_coeff are committed by the
 * next block call; t_req is that call's first output frame.  Segment k (length L_k, first tap
 * off_k) computes, when launched, frames up to off_k ahead of the output, so part of the future
 * is already fixed under the old sets.  The switch takes effect at
 *     t_sw = max(t_req, max_k (e_k - L_k + off_k)),  e_k = first multiple of L_k >= t_req + L0,
 * the first frame all of whose contributions are launched after the request:
 * t_req <= t_sw <= t_req + max_k off_k.
 *
 * Output.  y_old / y_new are the full-history convolutions of the input under the old and the
 * new assignment (filter in/out scales included), F the cross-fade length, w(j) = j / (F - 1):
 *     t < t_sw              y_old(t)
 *     t_sw <= t < t_sw + F  (1 - w(t - t_sw)) y_old(t) + w(t - t_sw) y_new(t)
 *     t >= t_sw + F         y_new(t)
 * then the output gain, then the output format's 1/scale, then quantisation.  Old weight 1 at
 * the first frame of the ramp, new weight 1 at its last, like the reference's cross-fade.
 * Between t_req and the end of the window the segment blocks that need both assignments run
 * their input transform once and the MAC + inverse transform twice, into two accumulators.
 * Outside a window the cost and the output bits are those of a convolver without sets.
 */
/* another impulse response for `filter` (before finalize).  n_taps <= bfhip_nupc_taps(); shorter
   sets are zero-padded.  Returns the set index (>= 1). */
int bfhip_nupc_add_coeff(bfhip_nupc *n, int filter, const void *taps, long n_taps);
/* cross-fade length in frames for the switches committed from now on: 0 = hard switch, >= 2 =
   linear ramp; default L0 (the reference's one-block fade); 1 or > 1048576: BFHIP_EINVAL */
int bfhip_nupc_set_crossfade(bfhip_nupc *n, int frames);
/* queue filter -> set (after finalize); every call made before the next block call forms ONE
   switch (a preset).  BFHIP_ESTATE while the previous switch is still in flight
   (bfhip_nupc_switch_busy), and nothing changes.  A group that changes no filter's set commits
   no switch. */
int bfhip_nupc_set_coeff(bfhip_nupc *n, int filter, int coeff);
/* t_sw of the last committed switch; -1 if none yet (a NULL handle: BFHIP_ESTATE) */
long bfhip_nupc_switch_frame(const bfhip_nupc *n);
/* 1 while a committed switch has old-coefficient work or fade frames left, else 0 */
int bfhip_nupc_switch_busy(const bfhip_nupc *n);
/* ---- staggered switches: heard within one period (an opt-in mode) ---------------------------
 * The aligned switch above waits for the first frame ALL of whose contributions were launched
 * after the request: up to max_k off_k frames, and until then every segment block runs twice.
 * In staggered mode every segment switches as soon as its own next block is launched, as
 * time-varying partitioned convolvers usually do: the head of the impulse response changes in the
 * very next period, the tail follows as its blocks come due.
 *
 * Switch frames.  A request group committed by the block call whose first output frame is t_req
 * gives segment k the switch frame
 *     t_k = e_k - L_k + off_k,   e_k = first multiple of L_k >= t_req + L0,
 * the first frame segment k's next launch writes.  off_k >= L_k - L0 gives t_k >= t_req, and
 * t_0 = t_req always.
 *
 * Output, in front of output gain, 1/scale, sub-delay FIR, dither and quantisation (unchanged):
 *     y(t)   = sum_k [ (1 - w_k(t)) y_old,k(t) + w_k(t) y_new,k(t) ]
 *     w_k(t) = 0 for t < t_k,  (t - t_k) / (F - 1) for t_k <= t < t_k + F,  1 from t_k + F on
 * (F = 0: a step at t_k).  y_A,k is the full-history convolution of the inputs with segment k's
 * slice [off_k, off_k + N_k L_k) of the taps under assignment A (a (set, gain) pair per filter,
 * in and out scales included); sum_k y_A,k is y_A of the aligned contract.  F is
 * bfhip_nupc_set_crossfade's, with its meaning and limits.  During the fade of segment k the
 * output is a blend of two assignments that is neither y_old nor y_new in any band: that is what
 * "the tail follows" means.
 *
 * bfhip_nupc_switch_frame returns t_0 = t_req of the last committed switch in this mode, and
 * bfhip_nupc_switch_frame_segment t_k (in aligned mode: t_sw for every segment).
 *
 * bfhip_nupc_switch_busy, after a block call that has received `end` frames, is 1 iff some
 * segment's NEXT block starts before the segment's own fade ends:
 *     floor(end / L_k) L_k + off_k < t_k + F   for some k.
 * Only blocks that overlap [t_k, t_k + F) run under both assignments (the split-phase MAC +
 * inverse transform twice); they are blended into the one accumulator ring by one kernel.  With
 * F = 0 a staggered switch is never busy and there is no block under two assignments at all:
 * every segment runs the new assignment from its next launch on.  A second F = 0 switch committed
 * before a long segment's e_k therefore REPLACES the first one for that segment: the same t_k,
 * and the later assignment wins there (the first is never heard from that segment).
 * Overlapping cross-fades are not offered: set_coeff / set_filter_gain answer BFHIP_ESTATE while
 * busy, as in aligned mode.  The state rules of update_coeff* and render_eq* keep their wording:
 * live set, queued set, set of an in-flight (busy) switch.
 * The mode needs what a switch needs anyway (a second set or bfhip_nupc_reserve_filter_gain) and
 * allocates nothing.  A convolver that never selects it allocates, launches and computes exactly
 * as before.  Cost: DESIGN.md section 4.
 */
#define BFHIP_NUPC_SWITCH_ALIGNED   0   /* default: one switch frame t_sw for all segments */
#define BFHIP_NUPC_SWITCH_STAGGERED 1
/* for the switches committed from now on; before or after finalize.  BFHIP_ESTATE, and nothing
   changes, while bfhip_nupc_switch_busy is 1 or a set_coeff / set_filter_gain request is queued;
   BFHIP_EINVAL on a NULL handle or any other mode */
int bfhip_nupc_set_switch_mode(bfhip_nupc *n, int mode);
int bfhip_nupc_get_switch_mode(const bfhip_nupc *n);
/* t_k of the last committed switch (aligned mode: t_sw for every segment); -1 if none yet; a NULL
   handle or a segment out of range: BFHIP_ESTATE, like bfhip_nupc_switch_frame (BFHIP_EINVAL is -1,
   which means "no switch yet" here) */
long bfhip_nupc_switch_frame_segment(const bfhip_nupc *n, int segment);
/* rewrite a set that is neither live nor part of a queued / in-flight switch (BFHIP_ESTATE
   otherwise), at run time (bflogic_eq's "render into the inactive set, then switch").  Sets added
   by add_coeff cover the whole schedule; set 0 keeps add_filter's length, and taps past it must
   be zero (BFHIP_EINVAL).  Synchronous: waits for the segment engines' pending blocks. */
int bfhip_nupc_update_coeff(bfhip_nupc *n, int filter, int coeff, const void *taps, long n_taps);
/* ---- run-time control: set rewrites that never stall the audio thread ----------------------
 * bfhip_nupc_update_coeff above waits for every segment engine three times per partition and
 * copies synchronously: fine offline, not in the thread that owes a block every period.  The
 * calls below rewrite an idle set with no host wait and no allocation on the audio path:
 *
 *     reserve_update (before finalize)       everything is allocated at finalize
 *     render taps into update_buffer()       pinned staging of bfhip_nupc_taps() reals
 *     update_coeff_async(filter, set, ...)   enqueues the upload and the preparation, returns
 *     ... block calls ... update_busy() == 0 polled with hipEventQuery
 *     update_result() == BFHIP_OK            then set_coeff(filter, set) as usual
 *
 * Upload: host staging -> device staging on a low-priority loader stream of its own; a segment
 * that runs on the main stream (zero slack, or all of them with BFHIP_NUPC_BACKGROUND=0) has its
 * own slice copied on the main stream instead, so the main stream never waits for the whole
 * upload.  Preparation: one coefficient-preparation launch per segment engine for the segment's
 * whole slice, on the engine's own stream, in order with the engine's blocks (it shares their
 * FFT scratch above 8192).  Per partition it is the arithmetic of bfhip_nupc_update_coeff: the
 * prepared set, and the output after a switch onto it, have the same bits.
 * Exactness: a rewrite of an idle set changes no output byte until a switch onto the set; the
 * state rules are those of bfhip_nupc_update_coeff.  One rewrite is in flight at a time (a rewrite is
 * one set, or the sets of one bfhip_nupc_render_eq_group_async call).
 * A convolver that never calls reserve_update allocates nothing more, makes the same launches
 * and changes no byte.
 * Cost: DESIGN.md section 4 and profiles/nupc_rewrite_latency.jsonl.
 */
/* before finalize (BFHIP_ESTATE after) */
int bfhip_nupc_reserve_update(bfhip_nupc *n);
/* the pinned staging buffer (bfhip_nupc_taps() reals, realsize wide) after finalize; NULL without a
   reservation.  The caller may write it while no rewrite is in flight. */
void *bfhip_nupc_update_buffer(bfhip_nupc *n);
/* arguments and state rules of bfhip_nupc_update_coeff; BFHIP_ESTATE without a reservation, and
   while bfhip_nupc_update_busy is 1 (nothing changes; bfhip_nupc_update_coeff answers the same
   then).  taps may be the staging buffer itself (no copy); else one host memcpy into it.  Makes
   no stream, device or event wait, no blocking copy and no allocation, and no later block call
   makes one on its behalf. */
int bfhip_nupc_update_coeff_async(bfhip_nupc *n, int filter, int coeff, const void *taps, long n_taps);
/* the same from device memory.  ready_event: a hipEvent_t or NULL, as in bfhip_engine_block_dev_ev;
   the loader stream waits on it, and so does the main stream before it copies its own slices, so
   the host does not.  The buffer is the caller's again when bfhip_nupc_update_busy returns 0.
   The taps-past-set-0 rule cannot look at device memory: n_taps itself must not reach past set 0's
   partitions (BFHIP_EINVAL). */
int bfhip_nupc_update_coeff_dev_async(bfhip_nupc *n, int filter, int coeff, const void *taps_dev, long n_taps,
                                      void *ready_event);
/* 1 until every piece of the rewrite has completed on the device, then 0; never blocks */
int bfhip_nupc_update_busy(bfhip_nupc *n);
/* result of the last completed rewrite, without blocking: BFHIP_OK, or BFHIP_EINVAL with the
   reference's "NaN or Inf value among coefficients." if a tap was not finite; BFHIP_ESTATE while
   busy.  bfhip_nupc_set_coeff onto a set answers BFHIP_ESTATE while a rewrite of it is in flight
   and after a non-finite one, until a later rewrite of the set succeeds. */
int bfhip_nupc_update_result(bfhip_nupc *n);
/* blocks until the rewrite is done and returns its result: for tests and offline use, NOT for the
   audio thread */
int bfhip_nupc_update_wait(bfhip_nupc *n);
/* ---- run-time control: equaliser curves rendered on the device (bflogic_eq's "render into the
 * inactive set, then switch") -----------------------------------------------------------------
 * The producer in front of bfhip_nupc_update_coeff_dev_async: the host hands over the curve (at
 * most 130 bands of three doubles), the device evaluates it, transforms it and rewrites the set,
 * so a run-time equaliser needs no host FFT and uploads no taps.
 *
 * What is rendered is the reference's render_equaliser (rendereq.h:20-62) for taps = R.  With
 *     ci(a1, a2, f1, f2, f) = (a1 - a2) 0.5 cos(pi (f - f1) / (f2 - f1)) + (a1 + a2) 0.5
 * bin n = 1 .. R/2 - 1 at f = n / R, i the first band with f <= freq[i + 1], is
 *     X[n] = (-1)^n  ci(mag[i], mag[i+1], freq[i], freq[i+1], f) / R  (cos phi + i sin phi),
 *     phi  = ci(phase[i], phase[i+1], freq[i], freq[i+1], f),
 * X[0] = mag[0] / R and X[R/2] = mag[n_bands-1] / R are real, and
 *     taps[t] = X[0] + (-1)^t X[R/2] + 2 sum_n (Re X[n] cos(2 pi n t / R) - Im X[n] sin(2 pi n t / R))
 * (FFTW's unnormalised HC2R).  mag is linear and phase in radians, converted as bflogic_eq.c:173-175
 * does.  The reference writes the linear-phase term as cos(-R pi f + phi), which is (-1)^n cos phi
 * in exact arithmetic; the sign form is computed here, in float64 for both precisions and rounded
 * to the convolver's real type once, so the float32 build of the reference is not reproduced at
 * long lengths.  A render is a pure function of its arguments: the same
 * arguments give the same bytes.
 */
/* before finalize, after bfhip_nupc_reserve_update (BFHIP_ESTATE otherwise / after finalize).
   max_taps: a power of two, 8 <= max_taps <= min(bfhip_nupc_taps(), 1048576) (BFHIP_EINVAL).
   Everything the render needs is allocated at finalize. */
int bfhip_nupc_reserve_eq(bfhip_nupc *n, long max_taps);
/* render the curve into `taps` reals on the device and rewrite set `coeff` of `filter` with them
   (taps beyond `taps` are zero).  State rules, busy/result/wait calls and the exactness contract
   are those of bfhip_nupc_update_coeff_dev_async.  No host wait, no allocation, no blocking copy;
   the bands are copied at the call.
   taps: a power of two, 8 <= taps <= max_taps, and within set 0's partitions when coeff == 0.
   n_bands 2..130; freq[0] == 0, freq[n_bands-1] == 0.5, strictly ascending; mag finite and >= 0;
   phase finite: BFHIP_EINVAL otherwise and nothing changes.  Without bfhip_nupc_reserve_eq:
   BFHIP_ESTATE. */
int bfhip_nupc_render_eq_async(bfhip_nupc *n, int filter, int coeff, long taps, int n_bands,
                               const double freq[], const double mag[], const double phase[]);
/* the same render alone, synchronous, `taps` reals (realsize wide) into host memory: for tests and
   offline use.  BFHIP_ESTATE while a rewrite is in flight (it shares the scratch). */
int bfhip_nupc_render_eq(bfhip_nupc *n, long taps, int n_bands, const double freq[],
                         const double mag[], const double phase[], void *taps_out);
/* ---- minimum-phase render (an extension: bflogic_eq has no such mode) --------------------------
 * The linear render above carries (-1)^n: a flat curve of R taps is a unit pulse at tap R/2, and
 * every curve rendered with it adds R/2 frames of delay.  BFHIP_EQ_MINIMUM renders the same
 * magnitude curve with minimum phase (the homomorphic method): the energy sits at the first taps and
 * the equaliser adds no delay.  With R = taps, ci and the band search as above, n = 0 .. R/2:
 *     M[0] = mag[0],  M[R/2] = mag[n_bands-1],  M[n] = ci(mag[i], mag[i+1], freq[i], freq[i+1], n/R)
 *     phi[0] = phi[R/2] = 0,                    phi[n] = ci(phase[i], ...)        (1 <= n < R/2)
 *     c    = irfft(log M, R)                    the real cepstrum, R values (normalised inverse)
 *     c^[0] = c[0], c^[t] = 2 c[t] (1 <= t < R/2), c^[R/2] = c[R/2], c^[t] = 0 (t > R/2)
 *     S[k] = sum_t c^[t] exp(-2 pi i k t / R)
 *     X[k] = M[k] / R  (cos(Im S[k] + phi[k]) + i sin(Im S[k] + phi[k])),  X[0] and X[R/2] real
 *     taps = the unnormalised HC2R of X, as above; there is no (-1)^n term
 * (Re S[k] = log M[k] in exact arithmetic: the magnitude is taken from M[k] itself.)  phase[] is
 * excess phase on top of the minimum phase; all zeros give the minimum-phase response.  Curve, log,
 * sine and cosine are float64 for both precisions, the three transforms run in the convolver's real
 * type.  A render is a pure function of its arguments. */
#define BFHIP_EQ_LINEAR  0
#define BFHIP_EQ_MINIMUM 1
/* before finalize, after bfhip_nupc_reserve_eq (BFHIP_ESTATE otherwise / after finalize).  What the
   minimum-phase render needs beyond the linear one (one more buffer of max_taps reals when
   max_taps > 16384) is allocated at finalize.  A convolver that never calls this allocates nothing
   more and behaves as before. */
int bfhip_nupc_reserve_eq_minimum(bfhip_nupc *n);
/* bfhip_nupc_render_eq_async / bfhip_nupc_render_eq with a mode.  BFHIP_EQ_LINEAR gives the bytes of
   those calls and needs bfhip_nupc_reserve_eq only.  BFHIP_EQ_MINIMUM needs
   bfhip_nupc_reserve_eq_minimum (BFHIP_ESTATE without it) and every mag finite and > 0.  Any other
   mode, or a magnitude <= 0 in minimum mode: BFHIP_EINVAL and nothing changes.  All other argument
   and state rules, and the "no host wait, no allocation, no blocking copy" contract of the
   asynchronous call, are those of the two calls above. */
int bfhip_nupc_render_eq_mode_async(bfhip_nupc *n, int filter, int coeff, long taps, int n_bands,
                                    const double freq[], const double mag[], const double phase[], int mode);
int bfhip_nupc_render_eq_mode(bfhip_nupc *n, long taps, int n_bands, const double freq[],
                              const double mag[], const double phase[], int mode, void *taps_out);
/* ---- render onto a base impulse response (an extension: the reference cascades an equaliser
 * filter into the main one with to_filters / from_filters; this convolver has no cascades) --------
 * The renders above REPLACE a set with the curve's taps.  With a base the idle set receives
 * base (*) eq: a room-correction response keeps its correction under a tone control, with no host
 * convolution and no upload.
 *
 * Base.  A filter with a reservation owns a base of T = bfhip_nupc_taps() reals on the device.  At
 * finalize it holds bfhip_nupc_add_filter's taps, zero-padded (the scales are not part of it: the
 * filter applies them as always); bfhip_nupc_set_eq_base replaces it.  The base belongs to the
 * filter, not to a set.
 *
 * Result.  e[0 .. R), R = eq_taps, are the taps bfhip_nupc_render_eq_mode returns for the same
 * curve and mode, in the convolver's real type, b is the base, and
 *     y[t] = sum_{j = 0}^{min(t, R - 1)} e[j] b[t - j],   0 <= t < T
 * The convolution is TRUNCATED at T: a base with at least R trailing zeros loses nothing, a longer
 * one loses the tail that would reach past the schedule.  BFHIP_EQ_LINEAR adds R/2 frames of delay,
 * as the plain render does.  y is computed in the convolver's real type by FFT overlap-save
 * (eq_apply.h; block length in DESIGN.md section 4) and is a pure function of curve, mode, R and
 * base: the same arguments give the same bytes.  The synchronous call returns exactly the array the
 * asynchronous call writes into the set: a set written by bfhip_nupc_render_eq_base_async has the
 * bits of bfhip_nupc_update_coeff_async with the synchronous call's array.
 *
 * eq_taps: a power of two, 8 <= eq_taps <= min(max_taps, 8192), and 8 <= eq_taps <= max_taps with
 * bfhip_nupc_reserve_eq_base_long.  8192 is what one workgroup transforms in LDS at float64; a
 * longer curve (at 48 kHz 8192 taps are 5.9 Hz per bin, too coarse for room modes) is one block of
 * the overlap-save per eq_taps, transformed through the big FFT over global scratch.
 * Everything is allocated at finalize and only under a reservation: T reals per reserved filter, one
 * result of T reals, one spectrum, and the twiddle tables the renders do not already have.  A
 * convolver that never calls bfhip_nupc_reserve_eq_base allocates, launches and computes exactly as
 * before.
 */
/* before finalize, after bfhip_nupc_reserve_eq (BFHIP_ESTATE otherwise / after finalize); filter in
   range (BFHIP_EINVAL) */
int bfhip_nupc_reserve_eq_base(bfhip_nupc *n, int filter);
/* before finalize, after bfhip_nupc_reserve_eq (BFHIP_ESTATE otherwise / after finalize).  Lifts the
   eq_taps limit of bfhip_nupc_render_eq_base* from min(max_taps, 8192) to max_taps; every other rule
   of the two calls holds unchanged, and an eq_taps above the limit in force is BFHIP_EINVAL with that
   limit in the message.  Independent of the order of the bfhip_nupc_reserve_eq_base calls.  For
   eq_taps <= 8192 it changes no byte and no launch.  Allocates (at finalize) only when
   max_taps > 8192 and some filter has a base reservation: three buffers of (ceil(T / B) + 1) B
   complex values, the largest over the lengths B = 16384 .. max_taps (T + max_taps where max_taps
   divides T), one spectrum of max_taps complex values and the twiddle table of max_taps points
   (2 max_taps complex values).  T = 1 048 576 at float64: 150 994 944 bytes for
   max_taps = 1 048 576, 56 623 104 bytes for max_taps = 65536.  A convolver that never calls this
   allocates, launches and answers exactly as before. */
int bfhip_nupc_reserve_eq_base_long(bfhip_nupc *n);
/* after finalize; synchronous, for set-up and offline use, NOT for the audio thread.  taps: realsize
   wide, 1 <= n_taps <= T, shorter input is zero-padded (BFHIP_EINVAL otherwise).  A non-finite tap:
   BFHIP_EINVAL with the reference's "NaN or Inf value among coefficients.", and the base stays as it
   was.  BFHIP_ESTATE before finalize, without the filter's reservation, and while
   bfhip_nupc_update_busy is 1. */
int bfhip_nupc_set_eq_base(bfhip_nupc *n, int filter, const void *taps, long n_taps);
/* render the curve, convolve it onto the filter's base and rewrite set `coeff` of `filter` with the T
   reals.  Curve and mode rules are those of bfhip_nupc_render_eq_mode_async (BFHIP_EQ_MINIMUM needs
   bfhip_nupc_reserve_eq_minimum).  y spans the whole schedule, so the set-length rule of
   bfhip_nupc_update_coeff_dev_async applies with n_taps = T: coeff == 0 is accepted only where set 0
   covers every partition (BFHIP_EINVAL otherwise); the usual flow alternates between two sets made
   with bfhip_nupc_add_coeff.  State rules, busy / result / wait calls, "one rewrite in flight" and
   "no host wait, no allocation, no blocking copy, bands copied at the call" are those of
   bfhip_nupc_render_eq_mode_async; a failed argument or state check changes nothing.  BFHIP_ESTATE
   without the filter's reservation. */
int bfhip_nupc_render_eq_base_async(bfhip_nupc *n, int filter, int coeff, long eq_taps, int n_bands,
                                    const double freq[], const double mag[], const double phase[], int mode);
/* the same computation alone, synchronous: bfhip_nupc_taps() reals (realsize wide) into host memory,
   for tests and offline use.  BFHIP_ESTATE while a rewrite is in flight. */
int bfhip_nupc_render_eq_base(bfhip_nupc *n, int filter, long eq_taps, int n_bands, const double freq[],
                              const double mag[], const double phase[], int mode, void *taps_out);
/* ---- one render across a group of filters (an extension) ------------------------------------------
 * A tone control turns every filter of a crossbar under ONE curve, each filter on its own base.  With
 * the calls above that is one rewrite after another, each a round trip the host has to poll for, and
 * the curve rendered once per filter.  A group render names up to BFHIP_NUPC_GROUP_MAX idle sets of
 * different filters in one call: the curve is rendered once, its spectrum is computed once, every
 * member's convolution onto its base runs in one batched launch (eq_apply.h; beyond 8192 taps the
 * members go through the big FFT's buffers one after another, the curve transformed with each), all
 * members' preparations are enqueued together, and there is one completion to poll.  The
 * bfhip_nupc_set_coeff group then switches the members as one preset.
 *
 * Bytes.  After completion every member's set holds exactly the bytes the corresponding single call
 * writes into it -- bfhip_nupc_render_eq_base_async for a member rendered onto its base,
 * bfhip_nupc_render_eq_mode_async for a plain one, with the same curve, mode and eq_taps, and the same
 * base -- so the output after a switch onto the set is byte-identical to the output after the single
 * call.  A group of one IS the single call: the same launches.
 *
 * Argument and state rules.  Every member is checked before anything is enqueued: any failing check
 * answers its code, NOTHING changes for any member, and the message names the member.  Each member
 * obeys its single call's rules: eq_taps within the limit in force for a member onto a base (8192, or
 * max_taps with bfhip_nupc_reserve_eq_base_long) and within max_taps for a plain one; the curve rules
 * unchanged; BFHIP_EQ_MINIMUM needs its reservation; coeff == 0 only where set 0 covers every partition
 * (onto a base) or the eq_taps (plain); the set idle: neither live, queued, nor part of an in-flight
 * switch (BFHIP_ESTATE).  Beyond those: 1 <= n_members <= max_members, filter and coeff non-NULL, the
 * (filter, coeff) pairs pairwise distinct (BFHIP_EINVAL), no rewrite in flight and the reservation
 * made (BFHIP_ESTATE).
 *
 * Busy, result and wait.  bfhip_nupc_update_busy is 1 until every piece of every member is complete;
 * bfhip_nupc_update_wait waits for the group.  bfhip_nupc_update_result is BFHIP_OK iff every member is;
 * if a member ended non-finite it is BFHIP_EINVAL with the reference's message, and
 * bfhip_nupc_update_result_member says which.  bfhip_nupc_set_coeff onto a member's set answers
 * BFHIP_ESTATE while the group is in flight, and afterwards only for the members that ended
 * non-finite: the others can be switched to.  While a group is in flight every rewrite, render and
 * bfhip_nupc_set_eq_base call answers what it answers during a single rewrite.
 *
 * Audio path.  The call makes no host wait, no allocation and no blocking copy, and no later block
 * call makes one on its behalf; bands are copied at the call; the members' base and result pointers
 * travel as kernel arguments (16 pointer pairs, 256 bytes): there is no upload.  The main stream waits
 * for the render only where one of its own zero-slack segments reads a member's taps, as in a single
 * render; it then waits for the whole group's render.
 *
 * Allocation.  At finalize, behind every other allocation: one result of T reals per member beyond the
 * first (only where some filter has a base reservation), and (max_members - 1) * n_segments pinned
 * words for the per-member non-finite flags.  T = 1 048 576 at float64 and a group of four:
 * 3 * 8 388 608 = 25 165 824 bytes of device memory, and 12 pinned bytes per segment.  The members
 * behind the first are prepared straight out of their results (and the plain ones out of the one
 * rendered array: no copy per member), so the device staging buffer stays one.  A convolver that never
 * calls bfhip_nupc_reserve_eq_group allocates, launches and computes exactly as before; one that
 * reserves but never renders a group changes no output byte, and its single calls keep their bytes.
 */
#define BFHIP_NUPC_GROUP_MAX 16
/* before finalize, after bfhip_nupc_reserve_eq (BFHIP_ESTATE otherwise / after finalize);
   2 <= max_members <= BFHIP_NUPC_GROUP_MAX (BFHIP_EINVAL).  Everything a group needs is allocated at
   finalize, behind every allocation made without it. */
int bfhip_nupc_reserve_eq_group(bfhip_nupc *n, int max_members);
/* one curve into n_members idle sets at once.  Member i is set coeff[i] of filter filter[i];
   onto_base[i] != 0: the set receives base_i (*) eq as bfhip_nupc_render_eq_base_async writes it
   (needs that filter's bfhip_nupc_reserve_eq_base), == 0: the curve's taps as
   bfhip_nupc_render_eq_mode_async writes them.  onto_base == NULL: all zero. */
int bfhip_nupc_render_eq_group_async(bfhip_nupc *n, int n_members, const int filter[], const int coeff[],
                                     const int onto_base[], long eq_taps, int n_bands, const double freq[],
                                     const double mag[], const double phase[], int mode);
/* result of member i of the last completed group (a single rewrite is a group of one, member 0):
   BFHIP_OK, BFHIP_EINVAL (non-finite), BFHIP_ESTATE while busy, BFHIP_EINVAL for i out of range */
int bfhip_nupc_update_result_member(bfhip_nupc *n, int member);
/* ---- parametric equaliser sections rendered on the device (an extension: bflogic_eq knows bands only) --
 * The second curve producer in front of the same machinery.  A tone control holds second-order sections
 * -- shelves, peaks, notches, high and low passes -- not knots; sampled into 130 cosine-joined knots they
 * are approximate and lose their own (minimum) phase.  Here the host hands over 5 doubles per section and
 * the device evaluates the cascade exactly, per bin, in float64: no host FFT, no upload of taps.
 *
 * Sections.  coef holds n_sections * 5 doubles, section k being b0, b1, b2, a1, a2 with a0 = 1:
 *     H_k(z) = (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2)
 * 1 <= n_sections <= BFHIP_BIQUAD_MAX; every value finite; every section strictly stable, |a2| < 1 and
 * |a1| < 1 + a2 (which keeps the denominator off zero on the unit circle: a render has no device-side
 * error path beyond the non-finite flag every rewrite has).  Anything else: BFHIP_EINVAL, the message
 * names the section, nothing changes.
 *
 * Response.  R = taps, bin n = 0 .. R/2, s = sin^2(pi n / R), u = sin(2 pi n / R):
 *     N_k  = ((b0 + b1) + b2) - 2 (b0 + b2) s + i (b0 - b2) u
 *     D_k  = ((1  + a1) + a2) - 2 (1  + a2) s + i (1  - a2) u
 *     G[n] = prod_k N_k / D_k          (k ascending, float64 complex for both precisions)
 * = prod_k H_k(e^{i 2 pi n / R}); the common factor e^{-i w} cancels.  This form, not b0 + b1 z + b2 z^2:
 * at low frequencies 1 + a1 + a2 is of the order w0^2, and the direct polynomial loses that many digits
 * again at every bin.
 *
 * Phase.  BFHIP_BIQUAD_OWN:    X[n] = G[n] / R (0 < n < R/2), X[0] = Re G[0] / R, X[R/2] = Re G[R/2] / R.
 *         BFHIP_BIQUAD_LINEAR: X[n] = (-1)^n |G[n]| / R,      X[0] = |G[0]| / R,  X[R/2] = |G[R/2]| / R.
 * Any other value: BFHIP_EINVAL.  The taps are the unnormalised HC2R of X exactly as in the band render
 * above: X is rounded to the convolver's real type once and the transform runs in that type.
 * OWN gives taps[t] = sum_m h[t + m R], h the cascade's infinite impulse response: the response
 * TIME-ALIASED at R.  It adds no delay; R must be long enough for h to have decayed (a Q = 30 notch at
 * 50 Hz / 48 kHz rings for about 1e5 frames: what has not decayed wraps onto the first taps).  LINEAR
 * gives the magnitude alone with R/2 frames of delay, like BFHIP_EQ_LINEAR.  There is no homomorphic mode
 * for sections: a cascade that is minimum phase (peaks, shelves, low and high passes) is so under OWN.
 * These constants are a namespace of their own: BFHIP_EQ_* and what the band calls answer are unchanged.
 *
 * Calls.  Each one is its band counterpart with (n_bands, freq, mag, phase, mode) replaced by
 * (n_sections, coef, phase_mode); the reservations are the band calls' own (bfhip_nupc_reserve_eq,
 * _reserve_eq_base, _reserve_eq_base_long, _reserve_eq_group): no new reservation and no new allocation,
 * the sections travel as kernel arguments (at most 1280 bytes).  State rules, the taps and eq_taps limits,
 * the set-0 length rule, busy / result / wait / bfhip_nupc_update_result_member, "one rewrite in flight",
 * "no host wait, no allocation, no blocking copy, arguments copied at the call", "a failed check changes
 * nothing" and the group's all-members-checked-first rule are the corresponding band call's, word for
 * word.  A render is a pure function of its arguments; what the asynchronous call writes into a set has
 * the bits of bfhip_nupc_update_coeff_async with the synchronous call's array; a group member's set has
 * the bytes of the single call.  A convolver that never calls these allocates, launches and computes
 * exactly as before, and the band renders keep their bytes.
 */
#define BFHIP_BIQUAD_MAX    32
#define BFHIP_BIQUAD_OWN    0
#define BFHIP_BIQUAD_LINEAR 1
/* bfhip_nupc_render_eq_mode: synchronous, `taps` reals into host memory */
int bfhip_nupc_render_biquads(bfhip_nupc *n, long taps, int n_sections, const double coef[], int phase_mode,
                              void *taps_out);
/* bfhip_nupc_render_eq_mode_async */
int bfhip_nupc_render_biquads_async(bfhip_nupc *n, int filter, int coeff, long taps, int n_sections,
                                    const double coef[], int phase_mode);
/* bfhip_nupc_render_eq_base: synchronous, bfhip_nupc_taps() reals into host memory */
int bfhip_nupc_render_biquads_base(bfhip_nupc *n, int filter, long eq_taps, int n_sections, const double coef[],
                                   int phase_mode, void *taps_out);
/* bfhip_nupc_render_eq_base_async */
int bfhip_nupc_render_biquads_base_async(bfhip_nupc *n, int filter, int coeff, long eq_taps, int n_sections,
                                         const double coef[], int phase_mode);
/* bfhip_nupc_render_eq_group_async */
int bfhip_nupc_render_biquads_group_async(bfhip_nupc *n, int n_members, const int filter[], const int coeff[],
                                          const int onto_base[], long eq_taps, int n_sections,
                                          const double coef[], int phase_mode);
/* Section designer: host only, makes no HIP call and works on a machine without a device.  f0 is
 * normalised like the bands' freq, 0 < f0 < 0.5; q > 0; gain_db finite (ignored by the last four types);
 * type one of the seven below; coef non-NULL: BFHIP_EINVAL otherwise, and coef is untouched.  The
 * audio-EQ-cookbook formulas, with
 *     A = 10^(gain_db / 40),  w0 = 2 pi f0,  c = cos w0,  alpha = sin w0 / (2 q),  r = 2 sqrt(A) alpha,
 *     S = sin^2(w0 / 2) = (1 - c) / 2,  C = cos^2(w0 / 2) = (1 + c) / 2   (written so: nothing is lost at low f0)
 * and every value divided by a0:
 *   PEAK        b = 1 + alpha A,  -2 c,  1 - alpha A                  a = 1 + alpha / A,  -2 c,  1 - alpha / A
 *   LOW_SHELF   b0 = A ((A+1) - (A-1) c + r)   b1 =  2 A ((A-1) - (A+1) c)   b2 = A ((A+1) - (A-1) c - r)
 *               a0 =    (A+1) + (A-1) c + r    a1 = -2   ((A-1) + (A+1) c)   a2 =    (A+1) + (A-1) c - r
 *   HIGH_SHELF  b0 = A ((A+1) + (A-1) c + r)   b1 = -2 A ((A-1) + (A+1) c)   b2 = A ((A+1) + (A-1) c - r)
 *               a0 =    (A+1) - (A-1) c + r    a1 =  2   ((A-1) - (A+1) c)   a2 =    (A+1) - (A-1) c - r
 *   LOW_PASS    b = S,  2 S,  S                                       a = 1 + alpha,  -2 c,  1 - alpha
 *   HIGH_PASS   b = C,  -2 C,  C                                      a = 1 + alpha,  -2 c,  1 - alpha
 *   NOTCH       b = 1,  -2 c,  1                                      a = 1 + alpha,  -2 c,  1 - alpha
 *   ALL_PASS    b = 1 - alpha,  -2 c,  1 + alpha                      a = 1 + alpha,  -2 c,  1 - alpha
 * coef receives b0/a0, b1/a0, b2/a0, a1/a0, a2/a0. */
#define BFHIP_BIQUAD_PEAK       0
#define BFHIP_BIQUAD_LOW_SHELF  1
#define BFHIP_BIQUAD_HIGH_SHELF 2
#define BFHIP_BIQUAD_LOW_PASS   3
#define BFHIP_BIQUAD_HIGH_PASS  4
#define BFHIP_BIQUAD_NOTCH      5
#define BFHIP_BIQUAD_ALL_PASS   6
int bfhip_biquad_design(int type, double f0, double gain_db, double q, double coef[5]);
/* per-output gain applied at the emit step, in force from the first frame of the next block call's
   output (a step, or the start of a ramp: bfhip_nupc_set_gain_ramp below); 0.0 mutes; default 1.0
   (multiplied into the 1/scale factor in float64: exact) */
int bfhip_nupc_set_output_gain(bfhip_nupc *n, int out_ch, double gain);

/* ---- run-time control: per-filter gains (cffa / cfoa) and ramped output gain ----------------
 * Per-filter gain.  An assignment is, per filter, a pair (set, gain), not a set alone: under an
 * assignment filter f contributes  in_scale * out_scale * gain_f * (x_in * taps_set).  A gain
 * change is a switch like any other -- t_sw, y_old / y_new as full-history convolutions, the
 * linear ramp of bfhip_nupc_set_crossfade, then output gain, 1/scale and quantisation, all as
 * defined above -- so it is click-free through the cross-fade and exact in the sense a set switch
 * is.  In a 2x2 crossbar that is the balance, the crossfeed amount and the polarity of one path.
 * All bfhip_nupc_set_coeff and bfhip_nupc_set_filter_gain calls made before the next block call
 * form ONE switch; a group that changes neither a set nor a gain commits none (switch_frame, the
 * launches and the output bytes stay as they were).  A per-filter change takes effect up to
 * max_k off_k frames after the request, as a set switch does, and costs what a switch window
 * costs (dual segment blocks, one plan rebuild each); the output gain below is the knob for
 * immediate changes.  The gain multiplies the segment engines' output scale (out_scale * 1.0 is
 * out_scale: gain 1.0 changes no bit); the state rules of the set rewrites refer to sets only.
 * A convolver that neither reserves nor has a second set allocates nothing more, makes the same
 * launches and changes no byte.
 *
 * Output gain ramp, per output channel.  g_prev is the gain applied to the last emitted frame
 * (before the first frame: the channel's gain at finalize), g_tgt the current target.  A call
 * set_output_gain(ch, g) with g == g_tgt changes nothing and does not restart a running ramp.
 * Otherwise, with t0 the first frame of the next block call, R the ramp length in force at the
 * call and a = g_prev at t0 - 1:
 *     R == 0   g(t) = g for t >= t0 (a step: the bits of a convolver that never set a ramp)
 *     R >= 1   g(t0 + j) = a + (g - a) (j + 1) / R   for 0 <= j < R - 1,   g exactly for j >= R - 1
 * across as many periods as it takes.  A new target during a ramp starts a new ramp from the value
 * of the last emitted frame; of several calls for a channel before one block call the last counts.
 * g is evaluated in float64 for both precisions and the sample is multiplied by
 * (real)((1 / scale) * g); everything behind the factor -- the sub-delay FIR's input, the dither
 * chain's input, the quantiser, the overflow accounting -- is as before, so the FIR filters the
 * ramped values and a gain ramped to 0 gives dithered silence.  The emit step evaluates the factor
 * per frame and advances the ramp on the device: a ramp in progress needs no upload, no launch and
 * no host wait; only a new target uploads the channels' records (32 bytes each).
 * Cost: DESIGN.md section 4.
 */
/* gain-only switches need the spare accumulator ring and the second segment output buffers, which
   otherwise exist only when some filter has a second set: before finalize (BFHIP_ESTATE after) */
int bfhip_nupc_reserve_filter_gain(bfhip_nupc *n);
/* gain: finite (BFHIP_EINVAL otherwise), negative flips the polarity, 0.0 silences the filter (its
   contribution is exact zeros).  Before finalize: the filter's initial gain (default 1.0; needs no
   reservation).  After finalize: queued like bfhip_nupc_set_coeff; BFHIP_ESTATE without the
   reservation, and while bfhip_nupc_switch_busy (nothing changes) */
int bfhip_nupc_set_filter_gain(bfhip_nupc *n, int filter, double gain);
/* the gain of the newest committed assignment: the new value once the block call that committed
   the switch has returned, the old one before.  NaN on a bad handle / filter */
double bfhip_nupc_get_filter_gain(const bfhip_nupc *n, int filter);
/* ramp length in frames for the bfhip_nupc_set_output_gain calls made from now on, at any time:
   0 = step (default), 1 .. 1048576; else BFHIP_EINVAL */
int bfhip_nupc_set_gain_ramp(bfhip_nupc *n, int frames);
/* bf_reset_peak (bfhip_engine_reset_overflow's counterpart): every output's overflow struct back
   to its initial value, stream-ordered in front of the next block call; no host wait.  Status bits
   are not touched */
int bfhip_nupc_reset_overflow(bfhip_nupc *n);

/* ---- run-time control: per-channel integer delay and mute (delay: / maxdelay:, cid / cod,
 * cmi / cmo) -------------------------------------------------------------------------------
 * io is BFHIP_IN or BFHIP_OUT; channels are the side's raw channels.  The reference does these
 * on dai.c's raw period buffers (dai.c:1386-1390, 1444-1449, 1664-1668; delay.c:229-340); the
 * convolver does the same on the device, so its raw output is what dai.c makes of it.
 *
 * Period.  The delay line's fragment is seg_length[0] (L0) frames and a requested delay is read
 * once per block call: the output is the reference's at a period of L0 frames.
 * Input side.  A muted input's samples are zeroed on the raw block before its delay line; the
 * zeros enter the line and the line keeps advancing (do_mute, then update_delay).  The delay runs
 * in place on the block in the input ring (on the staged period of a side that declares its
 * buffer, in front of the conversion into the ring of reals), so every segment, whatever its
 * length and however late it is launched, reads delayed input.  Every channel's line is sized
 * from its own sample width.
 * Output side.  The delay runs on the quantised raw output, after dither, output gain and the
 * cross-fade; the mute comes after the delay (update_delay, then mute).  The overflow structs and
 * status bits count the undelayed, unmuted samples, as real2raw does before dai.c touches the
 * buffer.
 * Changes follow change_delay (delay.c:283-318) exactly: an increase zero-fills the line, so it
 * makes a gap of silence, and a decrease reuses the line's history.  There is no cross-fade; that
 * is the reference's behaviour.  The delay machine's state transitions do not depend on the
 * samples, so the host keeps them and hands each period's step to one kernel launch per side as
 * kernel arguments: no host wait per period, and a side where no channel is muted or delayed
 * makes no launch at all.  An initial delay above a maxdelay > 0 starts at maxdelay (the
 * reference would overrun its buffer).  Packed 3-byte samples with a delay <= L0 hang the
 * reference (shift_samples); here they get a pure delay.
 */
/* before finalize; < 0: fixed (the reference's maxdelay: -1, the default); BFHIP_ESTATE after */
int bfhip_nupc_set_maxdelay(bfhip_nupc *n, int io, int channel, int maxdelay);
/* before finalize: the initial delay (delay:); after finalize: in force from the first frame of
   the next block call (cid / cod).  delay < 0: BFHIP_EINVAL.  A value above the channel's
   limit, or any change of a fixed channel, is accepted and leaves the delay as it is
   (change_delay, delay.c:289-291; bfhip_engine_set_delay has the same contract) */
int bfhip_nupc_set_delay(bfhip_nupc *n, int io, int channel, int delay_frames);
/* any time; in force from the first frame of the next block call */
int bfhip_nupc_set_mute(bfhip_nupc *n, int io, int channel, int muted);
/* the delay in force (curdelay), for a CLI's "info" */
int bfhip_nupc_get_delay(const bfhip_nupc *n, int io, int channel);

/* ---- run-time control: per-channel sub-sample delay (sdf_length: / subdelay:, bfaccess->
 * set_subdelay) -------------------------------------------------------------------------------
 * The reference filters the time-domain reals of a channel once per period (bfrun.c:1497-1531,
 * 1921-1925, delay.c:416-442); the convolver does the same once per block call of L0 frames, in
 * front of all segments and behind the accumulator ring, so its output is the reference's at a
 * period of L0 frames.  A side "uses sub-delay" when at least one of its channels has a filter.
 *
 * The filter is the causal FIR  y[t] = sum_k h_s[k] x[t - k]  over the channel's whole stream, h_s
 * the reference's 2 * sdf_length + 1 taps for the value s in hundredths of a sample (s = 0: a unit
 * pulse at tap sdf_length; else sample_sinc with its Kaiser window, beta 9, delay.c:56-76), x[t < 0]
 * = 0.  A filtered channel is delayed by sdf_length + s / 100 samples.  A value set between block
 * calls switches h from the next call's first frame and keeps reading the unfiltered history; there
 * is no cross-fade (the reference's behaviour).
 * Channels without a filter on a side that uses sub-delay get sdf_length whole frames of extra
 * delay through their integer delay line (dai.c:205-215, 230-243): added to the delay and to a
 * non-negative maxdelay; a fixed line (maxdelay < 0) stays fixed at delay + sdf_length (DESIGN.md
 * section 7).  bfhip_nupc_get_delay keeps reporting the delay without the extra.
 * Input side: mute and integer delay on the raw block as above, then raw -> real with the channel's
 * format, then the FIR (zeros from a mute enter the filter's history).  One kernel launch per
 * period converts the block into a ring of reals that every segment reads, however long it is and
 * however late it is launched.
 * Output side: cross-fade blend, output gain, the format's 1/scale, then the FIR, then dither,
 * quantisation, and integer delay and mute on the raw block: the FIR's input is the value the
 * output would have been quantised from without it (the dither section's definition), its history
 * holds those scaled values, and the overflow structs and status bits count the filtered samples.
 * Runs inside the emit step: no launch of its own.
 * A side that does not use sub-delay makes no launch, allocates nothing and changes no byte.
 * Limits: the filter block size bs (the smallest power of two >= 2 * sdf_length + 1) is at most
 * 1024, i.e. sdf_length <= 511 (BFHIP_EINVAL above); any L0 is supported, blocks above 2048 frames
 * are filtered 2048 frames at a time; a side that uses sub-delay has at most 256 channels.
 * Cost (configs[4], 64-frame periods, sdf_length 31 on both inputs and both outputs, new values
 * every 300 periods; tools/nupc_latency.py 64 --subdelay, profiles/nupc_subdelay_latency.jsonl):
 * one more launch per period on the input side, none on the output side.  The per-period wall
 * time with the filters (medians 0.057-0.072 ms over seven runs) lies inside the run-to-run band
 * of the convolver without them (0.051-0.085 ms): the added cost is below what the host clock
 * resolves.  Worst period 0.30 ms of the 1.33 ms period.
 */
/* before finalize (BFHIP_ESTATE after).  sdf_length >= 1, 2 * sdf_length + 1 <= L0 and L0 a
   multiple of bs, with the reference's messages (delay.c:458-470); kaiser_beta is accepted and
   ignored, as in the reference (delay.c:73) */
int bfhip_nupc_enable_subdelay(bfhip_nupc *n, int sdf_length, double kaiser_beta);
/* before finalize: BFHIP_UNDEFINED_SUBDELAY (-100, the default) = no filter on this raw channel; a
   value in (-100, 100) = a filter with that initial value (finalize fails with BFHIP_EINVAL if
   enable_subdelay was not called).  After finalize: the value of a channel that has a filter, in
   force from the first frame of the next block call; a channel without a filter or a value outside
   (-100, 100): BFHIP_EINVAL and nothing changes (bfrun.c:520-541) */
int bfhip_nupc_set_subdelay(bfhip_nupc *n, int io, int channel, int subdelay);
/* the value in force, -100 for a channel without a filter */
int bfhip_nupc_get_subdelay(const bfhip_nupc *n, int io, int channel);
/* tests: the 2 * sdf_length + 1 taps (realsize wide) the device filters with for `subdelay` in
   (-100, 100); returns the tap count or a negative error.  Makes no HIP call. */
int bfhip_selftest_subdelay_filter(int sdf_length, int subdelay, int realsize, void *out);

/* ---- linked look-ahead peak limiter on the outputs ---------------------------------------------
 * An extension (the reference's only answers to an over-range sample are the clip-and-count of
 * real2raw.h and safety_limit, which ends the program): a brick-wall peak
 * limiter inside the emit step, behind everything that can change level and in front of dither and
 * quantisation, linked across the channels of a group, wholly on the device.
 *
 * Place in the chain.  Output side: cross-fade blend, output gain(frame) / scale, sub-delay FIR,
 * LIMITER, dither / quantise with overflow accounting, integer delay line, mute.  Call x_c[t] the
 * real of output channel c, frame t, that a convolver without a limiter hands to its quantiser or
 * dither chain (in output units: full scale is 1 / fmt.scale); it is computed by the same device
 * functions in the same order, so it has the same bits.  With a limiter, frame t is quantised or
 * dithered from
 *     y_c[t] = x_c[t - D] * (T) s_g[t]     c in group g   (product in the convolver's real type T)
 *     y_c[t] = x_c[t - D]                  c in no group  (no multiply: the same bits, D frames later)
 *     x_c[t < 0] = 0
 * D is the look-ahead: every output gets D frames of extra delay, grouped or not, so channels stay
 * aligned.  The overflow structs, status bits, safety_limit and the dither input all see y.  A
 * non-finite x contributes nothing to the envelope; it reaches the quantiser as before and is
 * reported as before.
 *
 * Envelope, per group g, float64 for both precisions, frames counted as in the switch section:
 *     ceil_c = thr_g / fmt_c.scale       thr_g: the threshold in force at the block call that receives frame t
 *     p[t]   = max over c in g of |x_c[t]| / ceil_c      (non-finite x_c[t]: 0)
 *     r[t]   = 1 / p[t] if p[t] > 1, else 1              r[t < 0] = 1
 *     m[t]   = min over 0 <= j <= D of r[t - j]
 *     e[t]   = min(m[t], 1 - a (1 - e[t - 1]))           e[t < 0] = 1, a = exp(-1 / release_frames), release_frames == 0: a = 0
 *     s[t]   = (sum over 0 <= j <= D of e[t - j]) / (D + 1)      (a division, not a multiplication by a reciprocal)
 * the sliding-minimum + box-smoothed design: instant attack on the look-ahead minimum, exponential
 * release, then a (D + 1)-frame box.  Two properties follow.
 *   Ceiling.  Every e[t - j], 0 <= j <= D, is <= m[t - j] <= r[t - D], so s[t] <= r[t - D] up to the
 *   rounding of the sum and |y_c[t]| <= ceil_c (1 + (D + 4) eps_T).
 *   Idle exactness.  If no p exceeded 1 in the window every term is exactly 1, the sum exactly D + 1
 *   and s[t] == 1.0: y_c[t] has the bits of x_c[t - D].
 * The device evaluates the release recursion as a prefix scan of the deficit 1 - e and clamps the
 * result to m[t]; it differs from the frame-by-frame evaluation (bfhip_selftest_limiter_envelope) by
 * one rounding per step, which the recursion's decay bounds at about release_frames ulp of 1.0.
 *
 * - A threshold of 1.0 on an integer output still counts a sample of exactly +full scale as an
 *   overflow, because real2raw's range ends at 2^(b-1) - 1.
 * - bfhip_nupc_latency() stays L0; bfhip_nupc_limiter_delay() is what the limiter adds.
 * - Output gain, gain ramps, per-filter gains, switches and cross-fades act in front of the limiter:
 *   a gain raised at run time is caught.
 * - The integer delay line and the mute act behind it, on the raw block.
 * - A limiter with no group is legal: a pure D-frame delay of every output.
 * - A convolver that never enables it allocates, launches and computes exactly as before.
 * State (per output a ring of D + L0 reals; per group the last D values of r and of e and the
 * meter's minimum, float64; the group table) lives on the device and never crosses to the host per
 * period.  Two launches per period instead of the one emit launch; no host wait, no upload and no
 * allocation on the audio path.  Cost: DESIGN.md section 4.
 */
#define BFHIP_NUPC_LIMIT_LOOKAHEAD_MAX 1024
#define BFHIP_NUPC_LIMIT_GROUPS_MAX    32
#define BFHIP_NUPC_LIMIT_GROUP_MAX     8      /* channels per group */
/* before finalize (BFHIP_ESTATE after; twice: BFHIP_ESTATE).  1 <= lookahead_frames <= ..._LOOKAHEAD_MAX, any relation
   to L0; release_frames finite, 0 or >= 1 and <= 1e7 (BFHIP_EINVAL). */
int bfhip_nupc_enable_limiter(bfhip_nupc *n, int lookahead_frames, double release_frames);
/* before finalize, after enable_limiter (BFHIP_ESTATE).  1 <= n_ch <= ..._GROUP_MAX, channels in range, pairwise
   distinct and in no other group; threshold > 0, finite or +INFINITY (a group that never limits: r = 1), linear
   fraction of full scale (float formats: of 1.0) (BFHIP_EINVAL, the message names the channel).  Returns the group index. */
int bfhip_nupc_add_limiter_group(bfhip_nupc *n, const int out_channels[], int n_ch, double threshold);
/* any time after add_limiter_group: in force for the frames x[t] of the next block call on (they leave D frames
   later).  Travels as a kernel argument: no upload, no host wait. */
int bfhip_nupc_set_limiter_threshold(bfhip_nupc *n, int group, double threshold);
double bfhip_nupc_get_limiter_threshold(const bfhip_nupc *n, int group);      /* NaN on a bad handle / group */
int bfhip_nupc_limiter_delay(const bfhip_nupc *n);                            /* D, 0 without a limiter; BFHIP_EINVAL on a bad handle */
/* min of s_g over the frames emitted since the previous call for this group (1.0 if none), then reset; waits for
   the main stream like bfhip_nupc_get_overflow: NOT for the audio thread */
int bfhip_nupc_get_limiter_reduction(bfhip_nupc *n, int group, double *min_gain);
/* host only, no HIP call: s[0..n) of the definition above from p[0..n), fresh state.  For tests and as the
   definition in code. */
int bfhip_selftest_limiter_envelope(int lookahead_frames, double release_frames, long n, const double p[], double s_out[]);

/* ---- true-peak detection for the limiter --------------------------------------------------------
 * The detector above looks at the samples.  What a DAC's reconstruction filter, a sample-rate
 * converter or a lossy codec makes of them can exceed every sample: a sine at fs/4, 45 degrees off
 * the sampling instants, has samples of 0.7071 of its amplitude, a true peak 3 dB above its sample
 * peak.  In true-peak mode the detector looks at the waveform between the samples as well, the way
 * ITU-R BS.1770 and EBU R128 meter it (dBTP): oversample by four, take the peak over all phases.
 *
 * Interpolator.  Four phases per frame, H = BFHIP_NUPC_LIMIT_TP_HALF = 12, Kaiser window, beta = 8;
 * phase 0 is the sample itself:
 *     g_q[k]   = sinc(v) I0(beta sqrt(1 - (v / H)^2)) / I0(beta),   v = k - H + q / 4,   q = 1, 2, 3,   k = 0 .. 2 H - 1
 *     u_c,0[t] = x~_c[t - H]
 *     u_c,q[t] = sum over k = 0 .. 2 H - 1 of g_q[k] x~_c[t - k]      (float64 for both precisions, k ascending)
 *     x~_c[t]  = x_c[t] if finite, else 0;   x~_c[t < 0] = 0
 * u_c,q[t] estimates the waveform at time t - H + q / 4.  The taps are computed on the host in float64
 * (I0 by its power series) and travel to the kernel as an argument.  Interpolation error, measured in
 * float64 on sines at 13 phases: at most 8e-5 of the amplitude up to 0.35 fs, 1.4e-3 at 0.40 fs,
 * 2.1e-2 at 0.42 fs, 0.18 at 0.45 fs.  The droop near Nyquist is that of any short interpolator
 * (BS.1770's own has 12 taps per phase).  Because phase 0 is exact, the true-peak reading is never
 * below the sample peak.
 *
 * Detector and envelope, with D = lookahead_frames and D_e = D - H:
 *     p[t]   = max over c in g, q = 0 .. 3 of |u_c,q[t]| / ceil_c     (ceil_c as above: thr_g in force at the call that receives frame t)
 *     r, m, e, s: the formulas above with D_e in place of D
 *     y_c[t] = x_c[t - D] * (T) s[t]
 * The detector's H frames of latency come out of the look-ahead: every output still leaves exactly D
 * frames late and bfhip_nupc_limiter_delay() still returns D; channels in no group are untouched.
 * s[t] <= r[t - D_e], and r[t - D_e] was formed from the waveform at times t - D .. t - D + 3/4: the
 * gain on sample x[t - D] knows about the inter-sample peak behind it.
 *   Sample ceiling.  |y_c[t]| <= ceil_c (1 + (D_e + 4) eps_T) as above, because phase 0 is the sample.
 *   Idle exactness.  As above: no p above 1 in the window gives s == 1.0 and the bits of x_c[t - D].
 *   True peak.  Measured with the same interpolator applied to y, the true peak of y is held exactly
 *   wherever s is constant over the interpolator's span; while s moves the bound is approximate.  A
 *   float64 model gave 1 + 4.4e-7 of the ceiling over a whole run of the fs/4 sine above and 1.0104
 *   over 60 white-noise bursts: a measured property of the definition, not a guarantee.
 * Sample-peak mode is the default and does not change: a convolver that never selects true-peak mode,
 * or selects SAMPLE_PEAK, allocates, launches and computes exactly as before.  True-peak mode costs
 * one more double of group state and 72 float64 multiply-adds per member and frame; DESIGN.md section 4.
 */
#define BFHIP_NUPC_LIMIT_SAMPLE_PEAK 0      /* default: today's detector, today's bits */
#define BFHIP_NUPC_LIMIT_TRUE_PEAK   1
#define BFHIP_NUPC_LIMIT_TP_HALF     12     /* H: the interpolator spans 2 H frames */
/* before finalize, after enable_limiter (BFHIP_ESTATE).  Any other detector value: BFHIP_EINVAL.  TRUE_PEAK needs
   lookahead_frames >= 2 H = 24: BFHIP_EINVAL, the message names the limit, and nothing changes. */
int bfhip_nupc_set_limiter_detector(bfhip_nupc *n, int detector);
int bfhip_nupc_get_limiter_detector(const bfhip_nupc *n);                    /* BFHIP_EINVAL on a NULL handle */
/* true-peak mode only (BFHIP_ESTATE in sample-peak mode; BFHIP_EINVAL on a bad handle or group): the maximum of
   |u_c,q[t]| * fmt_c.scale over the group's channels, all four phases and all frames detected since the previous
   call for this group, as a fraction of full scale (0 if none), then reset; waits for the main stream like
   bfhip_nupc_get_limiter_reduction: NOT for the audio thread */
int bfhip_nupc_get_limiter_true_peak(bfhip_nupc *n, int group, double *max_peak);
/* host only, no HIP call: the taps g_q[k] above, g_out[(q - 1) * 2 H + k] */
int bfhip_selftest_truepeak_filter(double g_out[3 * 2 * BFHIP_NUPC_LIMIT_TP_HALF]);
/* host only, no HIP call: tp_out[t] = max over q = 0 .. 3 of |u_q[t]| for one channel x[0..n), fresh history,
   evaluated frame by frame.  For tests and as the definition in code. */
int bfhip_selftest_truepeak(long n, const double x[], double tp_out[]);

/* ---- BS.1770 loudness meter on the outputs ------------------------------------------------------
 *
 * The limiter and its true-peak detector say how high the programme may reach; this meter says how loud
 * it is (ITU-R BS.1770-4 / EBU R128: LUFS), per group of output channels, on the device, once per period,
 * with no host wait, upload or allocation on the audio path.  An extension: the reference's only level
 * read-out is the peak field of struct bfoverflow.
 *
 * Tap.  The meter reads the raw output block of the period after everything: the block rawout_dev holds
 * when bfhip_nupc_block_dev returns it -- behind the limiter, dither, quantisation with clipping, the integer
 * delay line and mute.  For output channel c, frame t:
 *     v_c[t] = (double) load_raw<double>(sample of channel c, frame t) * (double) fmt_c.scale     (fraction of full scale)
 *     v_c[t] = 0 where that value is not finite (float formats)
 * The sample's address comes from the channel's own byte_offset, sample_spacing and bytes, as the emit
 * step uses them, so every layout bfhip_nupc_set_format / bfhip_nupc_set_buffer_bytes can declare is
 * metered, in all 13 formats; and a float64 model of the meter needs only the bytes the convolver returned.
 *
 * K-weighting.  Two second-order sections per (group, member), float64 for both precisions, state zero at
 * finalize and kept across periods; the shelf first, then the high-pass, each in transposed direct form II:
 *     o = b0 v + s1;   s1 = b1 v - a1 o + s2;   s2 = b2 v - a2 o
 * The coefficients are for any rate, by the bilinear redesign of the BS.1770 prototype.  K = tan(pi f0 / fs):
 *     shelf:      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *                 Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2
 *                 b0 = (Vh + Vb K/Q + K^2)/a0   b1 = 2 (K^2 - Vh)/a0   b2 = (Vh - Vb K/Q + K^2)/a0
 *                 a1 = 2 (K^2 - 1)/a0           a2 = (1 - K/Q + K^2)/a0
 *     high-pass:  f0 = 38.13547087602444, Q = 0.5003270373238773, a0 = 1 + K/Q + K^2
 *                 b = (1, -2, 1)                a1 = 2 (K^2 - 1)/a0    a2 = (1 - K/Q + K^2)/a0
 * At fs = 48000 these reproduce the table of BS.1770-4 to all 14 printed digits.  Call the output z_c[t].
 *
 * Sub-blocks.  S = sample_rate / 10 frames (100 ms).  Sub-block j covers frames [j S, (j + 1) S), frames
 * counted from finalize as in the switch section; its boundaries bear no relation to L0.  For group g with
 * members c and weights G_c:
 *     E_g[j] = sum over c of G_c * (sum over t in sub-block j of z_c[t]^2)
 * The device keeps the last history_subblocks values of E_g in a ring (cell j mod history_subblocks) and
 * the partial sum of the open sub-block.  Two runs of the same input give the same bits of E: no
 * floating-point atomics, every sum in a fixed order.
 *
 * Read-outs, formed on the host from the ring, with l(m) = -0.691 + 10 log10(m), l(0) = -INFINITY, and J
 * the last complete sub-block:
 *     momentary   = l((E[J-3] + ... + E[J]) / (4 S))        needs 4 complete sub-blocks, else -INFINITY
 *     short_term  = l((E[J-29] + ... + E[J]) / (30 S))      needs 30, else -INFINITY
 *     gating blocks  B_j = (E[j-3] + ... + E[j]) / (4 S)  for every j with j - 3 >= first, where first is the
 *                    later of the reset point and J - history_subblocks + 1 (400 ms blocks, 75 % overlap)
 *     integrated  = l(mean of the B_j with l(B_j) > -70 and l(B_j) > l(mean of the B_j with l(B_j) > -70) - 10)
 *                   -INFINITY if no block passes
 * Loudness range (EBU Tech 3342) is not computed; bfhip_nupc_get_loudness_energy hands a host what it needs.
 *
 * Costs.  One more launch per period, one workgroup per group; per (group, member) four doubles of state, per
 * group 8 bytes per sub-block of history (one hour: 36 000 sub-blocks, 288 kB).  A convolver that never enables
 * the meter allocates, launches and computes exactly as before.  DESIGN.md section 4.
 */
#define BFHIP_NUPC_LOUD_GROUPS_MAX 32
#define BFHIP_NUPC_LOUD_GROUP_MAX  16      /* channels per group: 7.1.4 without its LFE is 11 */
typedef struct {
    double momentary, short_term, integrated;   /* LUFS; -INFINITY where undefined */
    long long subblocks;                        /* complete sub-blocks since finalize (J + 1) */
    long long first;                            /* first sub-block the integrated value covers */
    int wrapped;                                /* 1: the history ring has dropped sub-blocks since the reset */
} bfhip_loudness;

/* before finalize (after: BFHIP_ESTATE; twice: BFHIP_ESTATE).  sample_rate: a multiple of 10 in 8000 .. 768000 (the
   shelf needs fs well above 2 x 1682 Hz); history_subblocks: 30 .. 2^22.  Anything else: BFHIP_EINVAL, the message
   names the limit. */
int bfhip_nupc_enable_loudness(bfhip_nupc *n, int sample_rate, int history_subblocks);
/* before finalize, after enable_loudness (BFHIP_ESTATE).  1 <= n_ch <= ..._GROUP_MAX, channels in range and pairwise
   distinct within the group, weights finite and >= 0 (weight == NULL: all 1.0).  A channel may be in several groups
   (a stereo pair and the whole programme): each (group, member) filters for itself.  Returns the group index. */
int bfhip_nupc_add_loudness_group(bfhip_nupc *n, const int out_channels[], const double weight[], int n_ch);
/* after finalize: wait for the main stream like bfhip_nupc_get_limiter_reduction (NOT for the audio thread), download
   the group's ring and do the rest on the host.  get_loudness_energy copies sub-blocks [first, first + count):
   BFHIP_EINVAL if any of them is not complete yet or has left the ring. */
int bfhip_nupc_get_loudness(bfhip_nupc *n, int group, bfhip_loudness *out);
int bfhip_nupc_get_loudness_energy(bfhip_nupc *n, int group, long long first, int count, double E_out[]);
/* host bookkeeping only, no device work, no wait: the integrated value from now on covers the complete sub-blocks
   whose first frame is at or behind the frame of the next block call.  Filter state, ring, momentary and short_term
   are untouched. */
int bfhip_nupc_reset_loudness(bfhip_nupc *n, int group);
/* On a convolver that never enabled the meter the five calls above return BFHIP_ESTATE; BFHIP_EINVAL on a NULL handle
   or a bad group. */
/* host only, no HIP call: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 */
int bfhip_selftest_kweighting(int sample_rate, double coef_out[10]);
/* host only, one channel, weight 1, fresh state, frame by frame: E_out takes the n / S complete sub-blocks of
   v[0..n); returns their number */
int bfhip_selftest_loudness_energy(int sample_rate, long n, const double v[], double E_out[]);
/* host only: the read-outs of E[0..n_sub), sub-blocks 0 on, nothing dropped, no reset */
int bfhip_selftest_loudness_gate(int sample_rate, long n_sub, const double E[], bfhip_loudness *out);

#ifdef __cplusplus
}
#endif
#endif
