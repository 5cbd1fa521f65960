"""brutefir_amd -- MI355X-native replacement for BruteFIR's filter path.

The product is `libbfhip.so` (HIP kernels + a plain C ABI, `include/bfhip.h`); the C host
(`bfrun`/`bfconf`, bfio and bflogic modules) binds to it directly.  This
package is the thin Python binding used by tests/ and bench.py: it mirrors the C ABI one to
one and adds nothing.  There is no CPU path: if the library or a HIP device is missing every
call raises.
"""
import collections
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libbfhip.so")

IN, OUT = 0, 1
EQ_LINEAR, EQ_MINIMUM = 0, 1                       # include/bfhip_nupc.h: BFHIP_EQ_*
SWITCH_ALIGNED, SWITCH_STAGGERED = 0, 1            # include/bfhip_nupc.h: BFHIP_NUPC_SWITCH_*
EQ_MODES = {"linear": EQ_LINEAR, "minimum": EQ_MINIMUM}
BIQUAD_MAX = 32                                    # BFHIP_BIQUAD_MAX
BIQUAD_OWN, BIQUAD_LINEAR = 0, 1                   # BFHIP_BIQUAD_OWN / _LINEAR: a namespace apart from EQ_*
BIQUAD_PHASES = {"own": BIQUAD_OWN, "linear": BIQUAD_LINEAR}
(BIQUAD_PEAK, BIQUAD_LOW_SHELF, BIQUAD_HIGH_SHELF, BIQUAD_LOW_PASS, BIQUAD_HIGH_PASS, BIQUAD_NOTCH,
 BIQUAD_ALL_PASS) = range(7)                       # bfhip_biquad_design's types
RT_SPIN, RT_NO_GRAPH, RT_COPY_ENGINE, RT_OVERLAP = 1, 2, 4, 8      # bfhip_engine_rt_begin flags
COEFF_WATCH, COEFF_LAZY = 1, 2                                       # bfhip_engine_add_coeff_processed_blocks flags
ST_NONFINITE, ST_SAFETY = 1, 2
UNDEFINED_SUBDELAY = -100                                            # BFHIP_UNDEFINED_SUBDELAY


class BfhipError(RuntimeError):
    pass


class Overflow(C.Structure):
    """struct bfoverflow (bfmod.h:99-104)"""
    _fields_ = [("n_overflows", C.c_uint), ("intlargest", C.c_int32),
                ("largest", C.c_double), ("max", C.c_double)]

    def astuple(self):
        return (self.n_overflows, self.intlargest, self.largest, self.max)


class LoudnessStruct(C.Structure):
    """bfhip_loudness (include/bfhip_nupc.h)"""
    _fields_ = [("momentary", C.c_double), ("short_term", C.c_double), ("integrated", C.c_double),
                ("subblocks", C.c_longlong), ("first", C.c_longlong), ("wrapped", C.c_int)]


# what Nupc.loudness and loudness_gate return: LUFS (-inf where undefined), complete sub-blocks since finalize, the
# first sub-block the integrated value covers, and whether the history ring has dropped sub-blocks since the reset
Loudness = collections.namedtuple("Loudness", "momentary short_term integrated subblocks first wrapped")


def _loudness(s):
    return Loudness(s.momentary, s.short_term, s.integrated, s.subblocks, s.first, bool(s.wrapped))


class Format(C.Structure):
    """struct sample_format + struct buffer_format (dai.h:21-34)"""
    _fields_ = [("isfloat", C.c_int), ("swap", C.c_int), ("bytes", C.c_int),
                ("sbytes", C.c_int), ("scale", C.c_double),
                ("sample_spacing", C.c_int), ("byte_offset", C.c_int)]


# bfconf.c:358-480 (the _NE macro formats are resolved by the host before they get here)
SAMPLE_FORMATS = {
    "S8": (1, 1, 0, True),
    "S16_LE": (2, 2, 0, True), "S16_BE": (2, 2, 0, False),
    "S24_LE": (3, 3, 0, True), "S24_BE": (3, 3, 0, False),
    "S24_4LE": (4, 3, 0, True), "S24_4BE": (4, 3, 0, False),
    "S32_LE": (4, 4, 0, True), "S32_BE": (4, 4, 0, False),
    "FLOAT_LE": (4, 4, 1, True), "FLOAT_BE": (4, 4, 1, False),
    "FLOAT64_LE": (8, 8, 1, True), "FLOAT64_BE": (8, 8, 1, False),
}


def make_format(name, sample_spacing=1, byte_offset=0):
    nbytes, sbytes, isfloat, le = SAMPLE_FORMATS[name]
    scale = 1.0 if isfloat else 1.0 / float(1 << (8 * sbytes - 1))
    return Format(isfloat, 0 if le else 1, nbytes, sbytes, scale, sample_spacing, byte_offset)


def interleaved_formats(name, n_channels):
    """buffer_format of an interleaved device with n_channels open (dai.c:537-576)"""
    nbytes = SAMPLE_FORMATS[name][0]
    return [make_format(name, n_channels, c * nbytes) for c in range(n_channels)]


def period_layout(L0, devices):
    """buffer_format of one side's period buffer of L0 frames for a list of devices laid back to back
    (dai.c:537-576).  A device is (format name, open_channels, channel_selection, interleaved); the
    side's channels are numbered in device order, then selection order.  An interleaved device takes
    L0 frames of open_channels samples and channel i of its selection sits at sample slot
    channel_selection[i] of every frame; a non-interleaved one gives each selected channel a plane of
    L0 samples.  The running size is rounded up to 32 bytes after every device.
    Returns (formats, n_bytes): what Nupc.set_format and Nupc.set_buffer_bytes take."""
    formats, n_bytes = [], 0
    for name, open_channels, selection, interleaved in devices:
        nbytes = SAMPLE_FORMATS[name][0]
        for slot in selection:
            if interleaved:
                formats.append(make_format(name, open_channels, n_bytes + slot * nbytes))
            else:
                formats.append(make_format(name, 1, n_bytes))
                n_bytes += L0 * nbytes
        if interleaved:
            n_bytes += L0 * open_channels * nbytes
        n_bytes = -(-n_bytes // 32) * 32
    return formats, n_bytes


_lib = None


def lib():
    """Load libbfhip.so.  Raises if it has not been built -- never falls back to anything."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BfhipError("%s is missing: build it with `python -m brutefir_amd.build` "
                         "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    ip, dp = C.POINTER(ci), C.POINTER(cd)
    L.bfhip_last_error.restype = C.c_char_p
    L.bfhip_version.restype = C.c_char_p
    L.bfhip_engine_create.restype = vp
    L.bfhip_engine_create.argtypes = [ci] * 6
    L.bfhip_engine_destroy.argtypes = [vp]
    L.bfhip_engine_set_format.argtypes = [vp, ci, ci, C.POINTER(Format)]
    L.bfhip_engine_set_safety_limit.argtypes = [vp, cd]
    L.bfhip_engine_enable_subdelay.argtypes = [vp, ci, cd]
    L.bfhip_engine_set_subdelay.argtypes = [vp, ci, ci, ci]
    L.bfhip_engine_map_channels.argtypes = [vp, ci, ci, ip]
    for f in ("bfhip_engine_set_delay", "bfhip_engine_set_maxdelay", "bfhip_engine_set_mute"):
        getattr(L, f).argtypes = [vp, ci, ci, ci]
    L.bfhip_engine_enable_dither.argtypes = [vp, ip, ci, ci, ci]
    L.bfhip_engine_reserve_coeffs.argtypes = [vp, cd]
    L.bfhip_engine_add_coeff.argtypes = [vp, vp, ci, cd, ci]
    L.bfhip_engine_add_coeff_dev.argtypes = [vp, vp, ci, cd, ci]
    L.bfhip_engine_update_coeff_block.argtypes = [vp, ci, ci, vp]
    L.bfhip_engine_add_coeff_processed.argtypes = [vp, vp, ci]
    L.bfhip_engine_read_coeff_processed.argtypes = [vp, ci, vp]
    L.bfhip_engine_add_coeff_processed_blocks.argtypes = [vp, C.POINTER(vp), ci, ci]
    L.bfhip_engine_refresh_coeff_processed.argtypes = [vp, ci, ci, vp]
    L.bfhip_engine_poll_coeff_changes.argtypes = [vp]
    L.bfhip_coeff_mark_dirty.argtypes = [vp]
    L.bfhip_coeff_mark_dirty.restype = None
    L.bfhip_coeff_dirty_sequence.restype = C.c_ulonglong
    L.bfhip_engine_add_filter.argtypes = [vp, ci, ip, dp, ci, ip, dp, ci, ip, dp, ci, ci, ci]
    L.bfhip_engine_set_filter_active.argtypes = [vp, ci, ci]
    L.bfhip_engine_stage_times.argtypes = [vp, dp]
    L.bfhip_engine_coeff_is_resident.argtypes = [vp, ci]
    L.bfhip_engine_set_output_active.argtypes = [vp, ci, ci]
    L.bfhip_engine_output_is_active.argtypes = [vp, ci]
    L.bfhip_engine_set_filter_name.argtypes = [vp, ci, ci]
    L.bfhip_engine_finalize.argtypes = [vp]
    L.bfhip_engine_set_coeff.argtypes = [vp, ci, ci]
    L.bfhip_engine_set_delayblocks.argtypes = [vp, ci, ci]
    L.bfhip_engine_set_scale.argtypes = [vp, ci, ci, ci, cd]
    L.bfhip_engine_set_fscale.argtypes = [vp, ci, ci, cd]
    L.bfhip_engine_block.argtypes = [vp, vp, vp, C.POINTER(Overflow)]
    L.bfhip_engine_block_dev.argtypes = [vp, vp, vp]
    L.bfhip_engine_block_dev_ev.argtypes = [vp, vp, vp, vp, vp]
    L.bfhip_engine_sync.argtypes = [vp]
    L.bfhip_engine_inputs_dev.argtypes = [vp, vp]
    L.bfhip_engine_mac_dev.argtypes = [vp, vp]
    L.bfhip_engine_outputs_dev.argtypes = [vp, vp, ci, ci, vp]
    L.bfhip_engine_outputs_inputs_dev.argtypes = [vp, vp, ci, ci, vp, vp]
    L.bfhip_engine_advance.argtypes = [vp]
    L.bfhip_engine_set_stream.argtypes = [vp, vp]
    L.bfhip_engine_get_overflow.argtypes = [vp, ci, C.POINTER(Overflow)]
    L.bfhip_engine_reset_overflow.argtypes = [vp]
    L.bfhip_engine_blockcounter.restype = C.c_uint
    L.bfhip_engine_blockcounter.argtypes = [vp]
    L.bfhip_engine_ring_depth.argtypes = [vp]
    L.bfhip_engine_block_mode.argtypes = [vp]
    L.bfhip_selftest_fail_alloc.argtypes = [ci]
    L.bfhip_engine_output_lag.argtypes = [vp]
    L.bfhip_engine_flush.argtypes = [vp]
    L.bfhip_engine_uses_wave_fft.argtypes = [vp]
    L.bfhip_engine_uses_stream_layout.argtypes = [vp]
    L.bfhip_engine_uses_diag_mac.argtypes = [vp]
    L.bfhip_engine_window_blocks.argtypes = [vp]
    L.bfhip_engine_lookahead_blocks.argtypes = [vp]
    L.bfhip_engine_lookahead_far_blocks.argtypes = [vp]
    L.bfhip_engine_mac_counts.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.bfhip_engine_enable_pairs.argtypes = [vp, ci]
    L.bfhip_engine_block_pair_dev.argtypes = [vp, vp, vp, vp, vp]
    L.bfhip_engine_pair_launches.argtypes = [vp]
    L.bfhip_engine_pair_launches.restype = C.c_ulonglong
    L.bfhip_engine_enable_timing.argtypes = [vp, ci]
    L.bfhip_engine_get_timing.argtypes = [vp, dp]
    L.bfhip_engine_algorithmic_bytes.argtypes = [vp, dp]
    L.bfhip_engine_read_output_spectrum.argtypes = [vp, ci, vp]
    L.bfhip_engine_read_ring_slot.argtypes = [vp, ci, ci, vp]
    ull = C.POINTER(C.c_ulonglong)
    L.bfhip_engine_prewarm.argtypes = [vp]
    L.bfhip_engine_set_powersave.argtypes = [vp, cd]
    L.bfhip_engine_rt_begin.argtypes = [vp, ci]
    L.bfhip_engine_rt_end.argtypes = [vp]
    L.bfhip_engine_rt_buffer.restype = vp
    L.bfhip_engine_rt_buffer.argtypes = [vp, ci, ci]
    L.bfhip_engine_rt_submit.argtypes = [vp, vp]
    L.bfhip_engine_rt_wait.argtypes = [vp, vp, C.POINTER(Overflow)]
    L.bfhip_engine_rt_block.argtypes = [vp, vp, vp, C.POINTER(Overflow)]
    L.bfhip_engine_rt_stats.argtypes = [vp, ull, ull, ull]
    # non-uniform partitioned convolver (include/bfhip_nupc.h)
    L.bfhip_nupc_last_error.restype = C.c_char_p
    L.bfhip_nupc_create.restype = vp
    L.bfhip_nupc_create.argtypes = [ci, ci, ci, ci, ci, ip, ip]
    L.bfhip_nupc_destroy.argtypes = [vp]
    L.bfhip_nupc_taps.restype = C.c_long
    L.bfhip_nupc_taps.argtypes = [vp]
    L.bfhip_nupc_latency.argtypes = [vp]
    L.bfhip_nupc_set_format.argtypes = [vp, ci, ci, C.POINTER(Format)]
    L.bfhip_nupc_set_buffer_bytes.argtypes = [vp, ci, C.c_long]
    L.bfhip_nupc_buffer_bytes.restype = C.c_long
    L.bfhip_nupc_buffer_bytes.argtypes = [vp, ci]
    L.bfhip_nupc_set_safety_limit.argtypes = [vp, cd]
    L.bfhip_nupc_add_filter.argtypes = [vp, ci, ci, vp, C.c_long, cd, cd]
    L.bfhip_nupc_finalize.argtypes = [vp]
    L.bfhip_nupc_block.argtypes = [vp, vp, vp, C.POINTER(Overflow)]
    L.bfhip_nupc_block_dev.argtypes = [vp, vp, vp]
    L.bfhip_nupc_sync.argtypes = [vp]
    L.bfhip_nupc_get_overflow.argtypes = [vp, ci, C.POINTER(Overflow)]
    L.bfhip_nupc_add_coeff.argtypes = [vp, ci, vp, C.c_long]
    L.bfhip_nupc_set_crossfade.argtypes = [vp, ci]
    L.bfhip_nupc_set_coeff.argtypes = [vp, ci, ci]
    L.bfhip_nupc_switch_frame.restype = C.c_long
    L.bfhip_nupc_switch_frame.argtypes = [vp]
    L.bfhip_nupc_switch_busy.argtypes = [vp]
    L.bfhip_nupc_set_switch_mode.argtypes = [vp, ci]
    L.bfhip_nupc_get_switch_mode.argtypes = [vp]
    L.bfhip_nupc_switch_frame_segment.restype = C.c_long
    L.bfhip_nupc_switch_frame_segment.argtypes = [vp, ci]
    L.bfhip_nupc_update_coeff.argtypes = [vp, ci, ci, vp, C.c_long]
    L.bfhip_nupc_set_output_gain.argtypes = [vp, ci, cd]
    L.bfhip_nupc_reserve_filter_gain.argtypes = [vp]
    L.bfhip_nupc_set_filter_gain.argtypes = [vp, ci, cd]
    L.bfhip_nupc_get_filter_gain.restype = cd
    L.bfhip_nupc_get_filter_gain.argtypes = [vp, ci]
    L.bfhip_nupc_set_gain_ramp.argtypes = [vp, ci]
    L.bfhip_nupc_reset_overflow.argtypes = [vp]
    L.bfhip_nupc_reserve_update.argtypes = [vp]
    L.bfhip_nupc_update_buffer.restype = vp
    L.bfhip_nupc_update_buffer.argtypes = [vp]
    L.bfhip_nupc_update_coeff_async.argtypes = [vp, ci, ci, vp, C.c_long]
    L.bfhip_nupc_update_coeff_dev_async.argtypes = [vp, ci, ci, vp, C.c_long, vp]
    L.bfhip_nupc_update_busy.argtypes = [vp]
    L.bfhip_nupc_update_result.argtypes = [vp]
    L.bfhip_nupc_update_wait.argtypes = [vp]
    L.bfhip_nupc_reserve_eq.argtypes = [vp, C.c_long]
    L.bfhip_nupc_render_eq_async.argtypes = [vp, ci, ci, C.c_long, ci, dp, dp, dp]
    L.bfhip_nupc_render_eq.argtypes = [vp, C.c_long, ci, dp, dp, dp, vp]
    L.bfhip_nupc_reserve_eq_minimum.argtypes = [vp]
    L.bfhip_nupc_render_eq_mode_async.argtypes = [vp, ci, ci, C.c_long, ci, dp, dp, dp, ci]
    L.bfhip_nupc_render_eq_mode.argtypes = [vp, C.c_long, ci, dp, dp, dp, ci, vp]
    L.bfhip_nupc_reserve_eq_base.argtypes = [vp, ci]
    L.bfhip_nupc_set_eq_base.argtypes = [vp, ci, vp, C.c_long]
    L.bfhip_nupc_render_eq_base_async.argtypes = [vp, ci, ci, C.c_long, ci, dp, dp, dp, ci]
    L.bfhip_nupc_render_eq_base.argtypes = [vp, ci, C.c_long, ci, dp, dp, dp, ci, vp]
    L.bfhip_nupc_reserve_eq_base_long.argtypes = [vp]
    L.bfhip_nupc_reserve_eq_group.argtypes = [vp, ci]
    L.bfhip_nupc_render_eq_group_async.argtypes = [vp, ci, ip, ip, ip, C.c_long, ci, dp, dp, dp, ci]
    L.bfhip_nupc_update_result_member.argtypes = [vp, ci]
    L.bfhip_nupc_render_biquads.argtypes = [vp, C.c_long, ci, dp, ci, vp]
    L.bfhip_nupc_render_biquads_async.argtypes = [vp, ci, ci, C.c_long, ci, dp, ci]
    L.bfhip_nupc_render_biquads_base.argtypes = [vp, ci, C.c_long, ci, dp, ci, vp]
    L.bfhip_nupc_render_biquads_base_async.argtypes = [vp, ci, ci, C.c_long, ci, dp, ci]
    L.bfhip_nupc_render_biquads_group_async.argtypes = [vp, ci, ip, ip, ip, C.c_long, ci, dp, ci]
    L.bfhip_biquad_design.argtypes = [ci, cd, cd, cd, dp]
    L.bfhip_nupc_enable_dither.argtypes = [vp, ip, ci, ci, ci]
    L.bfhip_nupc_set_maxdelay.argtypes = [vp, ci, ci, ci]
    L.bfhip_nupc_set_delay.argtypes = [vp, ci, ci, ci]
    L.bfhip_nupc_set_mute.argtypes = [vp, ci, ci, ci]
    L.bfhip_nupc_get_delay.argtypes = [vp, ci, ci]
    L.bfhip_nupc_enable_subdelay.argtypes = [vp, ci, cd]
    L.bfhip_nupc_set_subdelay.argtypes = [vp, ci, ci, ci]
    L.bfhip_nupc_get_subdelay.argtypes = [vp, ci, ci]
    L.bfhip_selftest_subdelay_filter.argtypes = [ci, ci, ci, vp]
    L.bfhip_nupc_enable_limiter.argtypes = [vp, ci, cd]
    L.bfhip_nupc_add_limiter_group.argtypes = [vp, ip, ci, cd]
    L.bfhip_nupc_set_limiter_threshold.argtypes = [vp, ci, cd]
    L.bfhip_nupc_get_limiter_threshold.restype = cd
    L.bfhip_nupc_get_limiter_threshold.argtypes = [vp, ci]
    L.bfhip_nupc_limiter_delay.argtypes = [vp]
    L.bfhip_nupc_get_limiter_reduction.argtypes = [vp, ci, dp]
    L.bfhip_selftest_limiter_envelope.argtypes = [ci, cd, C.c_long, dp, dp]
    L.bfhip_nupc_set_limiter_detector.argtypes = [vp, ci]
    L.bfhip_nupc_get_limiter_detector.argtypes = [vp]
    L.bfhip_nupc_get_limiter_true_peak.argtypes = [vp, ci, dp]
    L.bfhip_selftest_truepeak_filter.argtypes = [dp]
    L.bfhip_selftest_truepeak.argtypes = [C.c_long, dp, dp]
    L.bfhip_nupc_enable_loudness.argtypes = [vp, ci, ci]
    L.bfhip_nupc_add_loudness_group.argtypes = [vp, ip, dp, ci]
    L.bfhip_nupc_get_loudness.argtypes = [vp, ci, C.POINTER(LoudnessStruct)]
    L.bfhip_nupc_get_loudness_energy.argtypes = [vp, ci, C.c_longlong, ci, dp]
    L.bfhip_nupc_reset_loudness.argtypes = [vp, ci]
    L.bfhip_selftest_kweighting.argtypes = [ci, dp]
    L.bfhip_selftest_loudness_energy.argtypes = [ci, C.c_long, dp, dp]
    L.bfhip_selftest_loudness_gate.argtypes = [ci, C.c_long, dp, C.POINTER(LoudnessStruct)]
    L.bfhip_engine_set_overlap.argtypes = [vp, ci]
    _lib = L
    return L


def _check(r):
    if r < 0:
        raise BfhipError("bfhip error %d: %s" % (r, lib().bfhip_last_error().decode()))
    return r


def _iarr(v):
    return (C.c_int * max(len(v), 1))(*v)


def _darr(v):
    return (C.c_double * max(len(v), 1))(*v)


def _ptr(x):
    """host numpy array, torch tensor (host or device) or raw integer address -> void*"""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return x.ctypes.data_as(C.c_void_p)


class Engine:
    """One filter process worth of device state (bfhip_engine)."""

    def __init__(self, length, n_blocks, realsize, n_in, n_out, device=0):
        self.L, self.N, self.rs, self.n_in, self.n_out = length, n_blocks, realsize, n_in, n_out
        self.dt = np.float32 if realsize == 4 else np.float64
        self.cdt = np.complex64 if realsize == 4 else np.complex128
        self.h = lib().bfhip_engine_create(device, length, n_blocks, realsize, n_in, n_out)
        if not self.h:
            raise BfhipError(lib().bfhip_last_error().decode())
        self.out_bytes = n_out * length * realsize
        self.in_bytes = n_in * length * realsize

    def close(self):
        if getattr(self, "h", None):
            lib().bfhip_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    # ---- construction
    def set_format(self, io, ch, fmt):
        _check(lib().bfhip_engine_set_format(self.h, io, ch, C.byref(fmt)))

    def set_interleaved(self, io, name):
        n = self.n_in if io == IN else self.n_out
        for c, f in enumerate(interleaved_formats(name, n)):
            self.set_format(io, c, f)
        nbytes = n * self.L * SAMPLE_FORMATS[name][0]
        if io == IN:
            self.in_bytes = nbytes
        else:
            self.out_bytes = nbytes

    def set_powersave(self, analog_powersave):
        _check(lib().bfhip_engine_set_powersave(self.h, analog_powersave))

    def set_safety_limit(self, v):
        _check(lib().bfhip_engine_set_safety_limit(self.h, v))

    def map_channels(self, io, virt2phys):
        _check(lib().bfhip_engine_map_channels(self.h, io, max(virt2phys) + 1, _iarr(list(virt2phys))))

    def set_interleaved_phys(self, io, name, n_phys):
        for c, f in enumerate(interleaved_formats(name, n_phys)):
            self.set_format(io, c, f)
        nbytes = n_phys * self.L * SAMPLE_FORMATS[name][0]
        if io == IN:
            self.in_bytes = nbytes
        else:
            self.out_bytes = nbytes

    def set_delay(self, io, ch, delay):
        _check(lib().bfhip_engine_set_delay(self.h, io, ch, delay))

    def set_maxdelay(self, io, ch, maxdelay):
        _check(lib().bfhip_engine_set_maxdelay(self.h, io, ch, maxdelay))

    def set_mute(self, io, ch, muted):
        _check(lib().bfhip_engine_set_mute(self.h, io, ch, int(muted)))

    def enable_subdelay(self, sdf_length, beta=9.0):
        _check(lib().bfhip_engine_enable_subdelay(self.h, sdf_length, beta))

    def set_subdelay(self, io, ch, subdelay):
        _check(lib().bfhip_engine_set_subdelay(self.h, io, ch, subdelay))

    def enable_dither(self, channels, sample_rate, max_size=0):
        _check(lib().bfhip_engine_enable_dither(self.h, _iarr(list(channels)), len(channels),
                                                sample_rate, max_size))

    def reserve_coeffs(self, total_bytes):
        _check(lib().bfhip_engine_reserve_coeffs(self.h, float(total_bytes)))

    def add_coeff(self, taps, scale=1.0, n_blocks=0):
        taps = np.ascontiguousarray(taps, self.dt)
        return _check(lib().bfhip_engine_add_coeff(self.h, _ptr(taps), len(taps), scale, n_blocks))

    def add_coeff_dev(self, taps_dev, n_taps, scale=1.0, n_blocks=0):
        return _check(lib().bfhip_engine_add_coeff_dev(self.h, _ptr(taps_dev), n_taps, scale,
                                                       n_blocks))

    def add_coeff_processed(self, cbufs):
        """cbufs: [n_blocks, 2L] reals in the reference's internal layout"""
        cbufs = np.ascontiguousarray(cbufs, self.dt)
        return _check(lib().bfhip_engine_add_coeff_processed(self.h, _ptr(cbufs), cbufs.shape[0]))

    def add_coeff_processed_blocks(self, addresses, watch=False, lazy=False):
        """addresses: host address of each block's cbuf (separate allocations, the reference's
        bfconf->coeffs_data[c][i]); watch: re-upload blocks another process marks dirty"""
        arr = (C.c_void_p * len(addresses))(*addresses)
        return _check(lib().bfhip_engine_add_coeff_processed_blocks(self.h, arr, len(addresses),
                                                                    (COEFF_WATCH if watch else 0) | (COEFF_LAZY if lazy else 0)))

    def refresh_coeff_processed(self, coeff, block, cbuf=None):
        _check(lib().bfhip_engine_refresh_coeff_processed(self.h, coeff, block, _ptr(cbuf)))

    def poll_coeff_changes(self):
        return _check(lib().bfhip_engine_poll_coeff_changes(self.h))

    def read_coeff_processed(self, coeff, n_blocks):
        out = np.empty((n_blocks, 2 * self.L), self.dt)
        got = _check(lib().bfhip_engine_read_coeff_processed(self.h, coeff, _ptr(out)))
        assert got == n_blocks
        return out

    def update_coeff_block(self, coeff, block, taps):
        taps = np.ascontiguousarray(taps, self.dt)
        assert len(taps) == self.L
        _check(lib().bfhip_engine_update_coeff_block(self.h, coeff, block, _ptr(taps)))

    def add_filter(self, in_ch=(), in_scale=None, in_f=(), in_fscale=None, out_ch=(),
                   out_scale=None, coeff=-1, delayblocks=0, crossfade=False):
        in_scale = [1.0] * len(in_ch) if in_scale is None else list(in_scale)
        in_fscale = [1.0] * len(in_f) if in_fscale is None else list(in_fscale)
        out_scale = [1.0] * len(out_ch) if out_scale is None else list(out_scale)
        return _check(lib().bfhip_engine_add_filter(
            self.h, len(in_ch), _iarr(list(in_ch)), _darr(in_scale),
            len(in_f), _iarr(list(in_f)), _darr(in_fscale),
            len(out_ch), _iarr(list(out_ch)), _darr(out_scale),
            coeff, delayblocks, int(crossfade)))

    # ---- a shard of the configuration (one engine per filter process of the host)
    def set_filter_active(self, f, active):
        _check(lib().bfhip_engine_set_filter_active(self.h, f, int(active)))

    def set_output_active(self, ch, active):
        _check(lib().bfhip_engine_set_output_active(self.h, ch, int(active)))

    def output_is_active(self, ch):
        return bool(lib().bfhip_engine_output_is_active(self.h, ch))

    def coeff_is_resident(self, c):
        return bool(lib().bfhip_engine_coeff_is_resident(self.h, c))

    def set_filter_name(self, f, name):
        _check(lib().bfhip_engine_set_filter_name(self.h, f, name))

    def finalize(self):
        _check(lib().bfhip_engine_finalize(self.h))

    # ---- run-time control
    def set_coeff(self, f, c):
        _check(lib().bfhip_engine_set_coeff(self.h, f, c))

    def set_delayblocks(self, f, d):
        _check(lib().bfhip_engine_set_delayblocks(self.h, f, d))

    def set_scale(self, f, io, idx, v):
        _check(lib().bfhip_engine_set_scale(self.h, f, io, idx, v))

    def set_fscale(self, f, idx, v):
        _check(lib().bfhip_engine_set_fscale(self.h, f, idx, v))

    # ---- per block
    def block(self, rawin, overflow=None, out=None):
        """host buffers in / out; returns (status bits, raw output bytes).  out: write into this
        buffer (the one the engines of several filter processes share)"""
        rawin = np.ascontiguousarray(rawin).view(np.uint8).ravel()
        assert rawin.size >= self.in_bytes, (rawin.size, self.in_bytes)
        if out is None:
            out = np.zeros(self.out_bytes, np.uint8)
        assert out.dtype == np.uint8 and out.size >= self.out_bytes and out.flags.c_contiguous
        st = _check(lib().bfhip_engine_block(self.h, _ptr(rawin), _ptr(out), overflow))
        return st, out

    def block_dev(self, rawin_dev, rawout_dev):
        _check(lib().bfhip_engine_block_dev(self.h, _ptr(rawin_dev), _ptr(rawout_dev)))

    def enable_pairs(self, on=True):
        _check(lib().bfhip_engine_enable_pairs(self.h, int(on)))

    def block_pair_dev(self, rawin0_dev, rawout0_dev, rawin1_dev, rawout1_dev):
        """two consecutive blocks, one pass over the coefficients (after enable_pairs before finalize)"""
        _check(lib().bfhip_engine_block_pair_dev(self.h, _ptr(rawin0_dev), _ptr(rawout0_dev), _ptr(rawin1_dev), _ptr(rawout1_dev)))

    @property
    def pair_launches(self):
        return int(lib().bfhip_engine_pair_launches(self.h))

    def block_dev_ev(self, rawin_dev, rawout_dev, in_ready=None, out_done=None):
        """in_ready / out_done: hipEvent_t handles (ints), e.g. torch.cuda.Event().cuda_event"""
        _check(lib().bfhip_engine_block_dev_ev(self.h, _ptr(rawin_dev), _ptr(rawout_dev),
                                               C.c_void_p(in_ready) if in_ready else None,
                                               C.c_void_p(out_done) if out_done else None))

    def set_overlap(self, mode):
        _check(lib().bfhip_engine_set_overlap(self.h, mode))

    def prewarm(self):
        _check(lib().bfhip_engine_prewarm(self.h))

    # real-time mode (callback I/O): pinned double buffer + graph replay
    def rt_begin(self, flags=0):
        _check(lib().bfhip_engine_rt_begin(self.h, flags))

    def rt_end(self):
        _check(lib().bfhip_engine_rt_end(self.h))

    def rt_submit(self, rawin):
        rawin = np.ascontiguousarray(rawin).view(np.uint8).ravel()
        assert rawin.size >= self.in_bytes, (rawin.size, self.in_bytes)
        _check(lib().bfhip_engine_rt_submit(self.h, _ptr(rawin)))

    def rt_wait(self, overflow=None, out=None):
        if out is None:
            out = np.zeros(self.out_bytes, np.uint8)
        assert out.dtype == np.uint8 and out.size >= self.out_bytes and out.flags.c_contiguous
        st = _check(lib().bfhip_engine_rt_wait(self.h, _ptr(out), overflow))
        return st, out

    def rt_block(self, rawin, overflow=None, out=None):
        self.rt_submit(rawin)
        return self.rt_wait(overflow, out)

    def rt_stats(self):
        a, b, c = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        _check(lib().bfhip_engine_rt_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"graph": a.value, "direct": b.value, "captures": c.value}

    def sync(self):
        return _check(lib().bfhip_engine_sync(self.h))

    def flush(self):
        """launch the output passes still owed (deferred / ping-pong schedule); does not wait"""
        _check(lib().bfhip_engine_flush(self.h))

    @property
    def output_lag(self):
        """block calls that pass before a block's output pass is launched (0, 1 or 2)"""
        return lib().bfhip_engine_output_lag(self.h)

    def inputs_dev(self, rawin_dev):
        _check(lib().bfhip_engine_inputs_dev(self.h, _ptr(rawin_dev)))

    def mac_dev(self, z_dev):
        _check(lib().bfhip_engine_mac_dev(self.h, _ptr(z_dev)))

    def outputs_dev(self, z_dev, first, count, rawout_dev):
        _check(lib().bfhip_engine_outputs_dev(self.h, _ptr(z_dev), first, count, _ptr(rawout_dev)))

    def outputs_inputs_dev(self, z_dev, first, count, rawout_dev, rawin_dev):
        _check(lib().bfhip_engine_outputs_inputs_dev(self.h, _ptr(z_dev), first, count,
                                                     _ptr(rawout_dev), _ptr(rawin_dev)))

    def advance(self):
        _check(lib().bfhip_engine_advance(self.h))

    def set_stream(self, hip_stream):
        _check(lib().bfhip_engine_set_stream(self.h, C.c_void_p(hip_stream)))

    def overflow(self, ch):
        of = Overflow()
        _check(lib().bfhip_engine_get_overflow(self.h, ch, C.byref(of)))
        return of

    def reset_overflow(self):
        _check(lib().bfhip_engine_reset_overflow(self.h))

    @property
    def blockcounter(self):
        return lib().bfhip_engine_blockcounter(self.h)

    @property
    def block_mode(self):
        """0 sequential, 1 pipelined (three streams), 2 deferred output (fused K3|K1 launch),
        3 ping-pong (fused K3|K1 launch on a side stream beside the previous MAC)"""
        return lib().bfhip_engine_block_mode(self.h)

    @property
    def uses_wave_fft(self):
        return bool(lib().bfhip_engine_uses_wave_fft(self.h))

    @property
    def uses_stream_layout(self):
        return bool(lib().bfhip_engine_uses_stream_layout(self.h))

    @property
    def uses_diag_mac(self):
        return bool(lib().bfhip_engine_uses_diag_mac(self.h))

    @property
    def window_blocks(self):
        """4: the plan in force runs long-window overlap-save (4-block windows); 2: standard"""
        return _check(lib().bfhip_engine_window_blocks(self.h))

    @property
    def lookahead_blocks(self):
        """3: the long plan in force runs the look-ahead MAC (tails of the next 3 blocks per call); 0: not"""
        return _check(lib().bfhip_engine_lookahead_blocks(self.h))

    @property
    def lookahead_far_blocks(self):
        """6: the look-ahead MAC runs its far tier (partitions >= 2 of the next 6 blocks per call); 0: not"""
        return _check(lib().bfhip_engine_lookahead_far_blocks(self.h))

    @property
    def mac_counts(self):
        """(MAC kernels launched so far, look-ahead blocks that ran the head pass, look-ahead blocks that ran
        the full long MAC instead)"""
        c = (C.c_ulonglong * 3)()
        _check(lib().bfhip_engine_mac_counts(self.h, c))
        return int(c[0]), int(c[1]), int(c[2])

    @property
    def ring_depth(self):
        return lib().bfhip_engine_ring_depth(self.h)

    # ---- measurement / debug
    def enable_timing(self, on=True):
        _check(lib().bfhip_engine_enable_timing(self.h, int(on)))

    def timing(self):
        ms = (C.c_double * 4)()
        _check(lib().bfhip_engine_get_timing(self.h, ms))
        return {"fft_in_ms": ms[0], "mac_ms": ms[1], "ifft_out_ms": ms[2], "launches": int(ms[3])}

    STAGES = ("raw2real", "time2freq", "mixscale1", "convolve", "mixscale2", "freq2time", "real2raw", "total")

    def stage_times(self):
        """the reference's `benchmark: true` columns (bfrun.c:2035-2078): (blocks averaged, {column: ms})"""
        ms = (C.c_double * 8)()
        n = _check(lib().bfhip_engine_stage_times(self.h, ms))
        return n, dict(zip(self.STAGES, ms))

    def algorithmic_bytes(self):
        b = (C.c_double * 2)()
        _check(lib().bfhip_engine_algorithmic_bytes(self.h, b))
        return {"block": b[0], "mac": b[1]}

    def output_spectrum(self, ch):
        """packed spectrum of output ch: element 0 = (DC, Nyquist), element k = bin k"""
        z = np.empty(self.L, self.cdt)
        _check(lib().bfhip_engine_read_output_spectrum(self.h, ch, _ptr(z)))
        return z

    def ring_slot(self, ch, slot):
        z = np.empty(self.L, self.cdt)
        _check(lib().bfhip_engine_read_ring_slot(self.h, ch, slot, _ptr(z)))
        return z


class Nupc:
    """Non-uniform partitioned convolver (bfhip_nupc): low-latency first block."""

    def __init__(self, seg_length, seg_blocks, realsize, n_in, n_out, device=0):
        self.rs, self.n_in, self.n_out = realsize, n_in, n_out
        self.dt = np.float32 if realsize == 4 else np.float64
        self.h = lib().bfhip_nupc_create(device, realsize, n_in, n_out, len(seg_length),
                                         _iarr(list(seg_length)), _iarr(list(seg_blocks)))
        if not self.h:
            raise BfhipError(lib().bfhip_nupc_last_error().decode())
        self.L0 = lib().bfhip_nupc_latency(self.h)
        self.taps = lib().bfhip_nupc_taps(self.h)
        # raw bytes of one L0-frame period per side: L0 frames of sample_spacing * bytes each (the
        # library copies whole frames, gaps included)
        self.in_bytes = n_in * self.L0 * realsize
        self.out_bytes = n_out * self.L0 * realsize

    def _chk(self, r):
        if r < 0:
            raise BfhipError("bfhip nupc error %d: %s" % (r, lib().bfhip_nupc_last_error().decode()))
        return r

    def close(self):
        if getattr(self, "h", None):
            lib().bfhip_nupc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_buffer_bytes(self, io, nbytes):
        """before finalize, after the side's set_format calls: the side's period buffer is nbytes long
        and every channel is laid out on its own (planes, several devices: period_layout)"""
        self._chk(lib().bfhip_nupc_set_buffer_bytes(self.h, io, nbytes))
        if io == IN:
            self.in_bytes = nbytes
        else:
            self.out_bytes = nbytes

    def buffer_bytes(self, io):
        """after finalize: bytes of one period buffer of the side, whichever way it was declared"""
        return self._chk(lib().bfhip_nupc_buffer_bytes(self.h, io))

    def set_format(self, io, ch, fmt):
        """without set_buffer_bytes every channel of a side must share one frame layout (sample_spacing
        and bytes; checked at finalize); the period size follows the last format set on the side"""
        self._chk(lib().bfhip_nupc_set_format(self.h, io, ch, C.byref(fmt)))
        nbytes = self.L0 * fmt.sample_spacing * fmt.bytes
        if io == IN:
            self.in_bytes = nbytes
        else:
            self.out_bytes = nbytes

    def set_interleaved(self, io, name):
        n = self.n_in if io == IN else self.n_out
        for c, f in enumerate(interleaved_formats(name, n)):
            self.set_format(io, c, f)

    def set_safety_limit(self, v):
        self._chk(lib().bfhip_nupc_set_safety_limit(self.h, v))

    def add_filter(self, in_ch, out_ch, taps, in_scale=1.0, out_scale=1.0):
        taps = np.ascontiguousarray(taps, self.dt)
        self._chk(lib().bfhip_nupc_add_filter(self.h, in_ch, out_ch, _ptr(taps), len(taps), in_scale, out_scale))

    def finalize(self):
        self._chk(lib().bfhip_nupc_finalize(self.h))

    def block(self, rawin, overflow=None):
        """host buffers in / out; returns (status bits, raw output bytes).  overflow: n_out
        Overflow structs (a ctypes array), read-modify-written like Engine.block's"""
        rawin = np.ascontiguousarray(rawin).view(np.uint8).ravel()
        assert rawin.size >= self.in_bytes, (rawin.size, self.in_bytes)
        assert overflow is None or len(overflow) >= self.n_out
        out = np.zeros(self.out_bytes, np.uint8)
        st = self._chk(lib().bfhip_nupc_block(self.h, _ptr(rawin), _ptr(out), overflow))
        return st, out

    def block_dev(self, rawin_dev, rawout_dev):
        self._chk(lib().bfhip_nupc_block_dev(self.h, _ptr(rawin_dev), _ptr(rawout_dev)))

    def sync(self):
        return self._chk(lib().bfhip_nupc_sync(self.h))

    def overflow(self, ch):
        of = Overflow()
        self._chk(lib().bfhip_nupc_get_overflow(self.h, ch, C.byref(of)))
        return of

    # run-time control (include/bfhip_nupc.h): coefficient switches and output gain
    def add_coeff(self, filt, taps):
        """another impulse response for filter `filt` (add_filter order); returns the set index"""
        taps = np.ascontiguousarray(taps, self.dt)
        return self._chk(lib().bfhip_nupc_add_coeff(self.h, filt, _ptr(taps), len(taps)))

    def set_crossfade(self, frames):
        self._chk(lib().bfhip_nupc_set_crossfade(self.h, frames))

    def set_coeff(self, filt, coeff):
        self._chk(lib().bfhip_nupc_set_coeff(self.h, filt, coeff))

    def switch_frame(self):
        """t_sw of the last committed switch, -1 if none yet"""
        r = lib().bfhip_nupc_switch_frame(self.h)
        return self._chk(r) if r != -1 else -1

    def switch_busy(self):
        return bool(self._chk(lib().bfhip_nupc_switch_busy(self.h)))

    # staggered switches: every segment switches at its own next launch (include/bfhip_nupc.h)
    def set_switch_mode(self, mode):
        """SWITCH_ALIGNED (default) or SWITCH_STAGGERED, for the switches committed from now on"""
        self._chk(lib().bfhip_nupc_set_switch_mode(self.h, mode))

    def switch_mode(self):
        return self._chk(lib().bfhip_nupc_get_switch_mode(self.h))

    def switch_frame_segment(self, segment):
        """segment's switch frame t_k of the last committed switch, -1 if none yet"""
        r = lib().bfhip_nupc_switch_frame_segment(self.h, segment)
        return self._chk(r) if r != -1 else -1

    def update_coeff(self, filt, coeff, taps):
        taps = np.ascontiguousarray(taps, self.dt)
        self._chk(lib().bfhip_nupc_update_coeff(self.h, filt, coeff, _ptr(taps), len(taps)))

    # set rewrites without a host wait (include/bfhip_nupc.h)
    def reserve_update(self):
        """before finalize: finalize then allocates what update_coeff_async needs"""
        self._chk(lib().bfhip_nupc_reserve_update(self.h))

    def update_buffer(self):
        """the pinned staging buffer as a numpy view of `taps` reals; None without a reservation"""
        p = lib().bfhip_nupc_update_buffer(self.h)
        if not p:
            return None
        ct = C.c_float if self.rs == 4 else C.c_double
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(self.taps,))

    def update_coeff_async(self, filt, coeff, taps):
        """enqueue the rewrite of an idle set and return; taps may be update_buffer() or a leading
        slice of it (no copy)"""
        if not (isinstance(taps, np.ndarray) and taps.dtype == self.dt and taps.flags.c_contiguous):
            taps = np.ascontiguousarray(taps, self.dt)
        self._chk(lib().bfhip_nupc_update_coeff_async(self.h, filt, coeff, _ptr(taps), len(taps)))

    def update_coeff_dev_async(self, filt, coeff, taps_dev, n_taps, ready=None):
        """the same from device memory (a torch tensor or an address); ready: a hipEvent_t handle
        (torch.cuda.Event().cuda_event) the loader waits on, or None"""
        self._chk(lib().bfhip_nupc_update_coeff_dev_async(self.h, filt, coeff, _ptr(taps_dev), n_taps,
                                                          C.c_void_p(ready) if ready else None))

    def update_busy(self):
        return bool(self._chk(lib().bfhip_nupc_update_busy(self.h)))

    def update_result(self):
        """result of the last completed rewrite (raises on a non-finite tap, and while busy)"""
        return self._chk(lib().bfhip_nupc_update_result(self.h))

    def update_result_member(self, member):
        """result of member `member` of the last completed group (a single rewrite: member 0)"""
        return self._chk(lib().bfhip_nupc_update_result_member(self.h, member))

    def update_wait(self):
        """blocks until the rewrite is done; not for the audio thread"""
        return self._chk(lib().bfhip_nupc_update_wait(self.h))

    # equaliser curves rendered on the device (include/bfhip_nupc.h)
    def reserve_eq(self, max_taps):
        """before finalize, after reserve_update: finalize then allocates what the renders need"""
        self._chk(lib().bfhip_nupc_reserve_eq(self.h, max_taps))

    def reserve_eq_minimum(self):
        """before finalize, after reserve_eq: finalize then also allocates what mode="minimum" needs"""
        self._chk(lib().bfhip_nupc_reserve_eq_minimum(self.h))

    @staticmethod
    def _eq_mode(mode):
        return EQ_MODES[mode] if isinstance(mode, str) else int(mode)

    def render_eq_async(self, filt, coeff, taps, freq, mag, phase, mode="linear"):
        """render the curve (bands: normalised frequency 0 .. 0.5, linear magnitude, phase in radians)
        into `taps` reals on the device and rewrite an idle set with them; returns at once.
        mode: "linear" (the reference's render, R/2 frames of delay) or "minimum" (minimum phase, no
        delay; needs reserve_eq_minimum and magnitudes > 0)"""
        assert len(freq) == len(mag) == len(phase)
        self._chk(lib().bfhip_nupc_render_eq_mode_async(self.h, filt, coeff, taps, len(freq), _darr(list(freq)),
                                                        _darr(list(mag)), _darr(list(phase)), self._eq_mode(mode)))

    def render_eq(self, taps, freq, mag, phase, mode="linear"):
        """the render alone, synchronous: a numpy array of `taps` reals"""
        assert len(freq) == len(mag) == len(phase)
        out = np.zeros(max(int(taps), 0), self.dt)
        self._chk(lib().bfhip_nupc_render_eq_mode(self.h, taps, len(freq), _darr(list(freq)), _darr(list(mag)),
                                                  _darr(list(phase)), self._eq_mode(mode), _ptr(out)))
        return out

    # the render convolved onto a base impulse response (include/bfhip_nupc.h)
    def reserve_eq_base(self, filt):
        """before finalize, after reserve_eq: the filter gets a base of `taps` reals on the device, which
        holds add_filter's taps at finalize"""
        self._chk(lib().bfhip_nupc_reserve_eq_base(self.h, filt))

    def reserve_eq_base_long(self):
        """before finalize, after reserve_eq: render_eq_base* then take eq_taps up to reserve_eq's max_taps
        instead of min(max_taps, 8192); finalize allocates the big-FFT scratch of the long windows"""
        self._chk(lib().bfhip_nupc_reserve_eq_base_long(self.h))

    def set_eq_base(self, filt, taps):
        """replace the filter's base (at most `taps` reals, zero-padded); blocks, not for the audio thread"""
        taps = np.ascontiguousarray(taps, self.dt)
        self._chk(lib().bfhip_nupc_set_eq_base(self.h, filt, _ptr(taps), len(taps)))

    def render_eq_base_async(self, filt, coeff, eq_taps, freq, mag, phase, mode="linear"):
        """render the curve into eq_taps reals (a power of two, at most 8192, or at most reserve_eq's
        max_taps with reserve_eq_base_long), convolve them onto the filter's base, truncated at `taps`, and rewrite an idle set with the result; returns at once"""
        assert len(freq) == len(mag) == len(phase)
        self._chk(lib().bfhip_nupc_render_eq_base_async(self.h, filt, coeff, eq_taps, len(freq), _darr(list(freq)),
                                                        _darr(list(mag)), _darr(list(phase)), self._eq_mode(mode)))

    # one render across a group of filters (include/bfhip_nupc.h)
    def reserve_eq_group(self, max_members):
        """before finalize, after reserve_eq: render_eq_group_async then takes up to max_members (2 .. 16) sets"""
        self._chk(lib().bfhip_nupc_reserve_eq_group(self.h, max_members))

    def render_eq_group_async(self, filters, coeffs, onto_base, eq_taps, freq, mag, phase, mode="linear"):
        """one curve into the idle sets (filters[i], coeffs[i]) at once: onto the filter's base where
        onto_base[i] is true (None: nowhere), the curve's taps alone otherwise; returns at once.  Every set
        gets the bytes of render_eq_base_async / render_eq_async; update_busy / update_wait cover the group"""
        assert len(freq) == len(mag) == len(phase) and len(filters) == len(coeffs)
        assert onto_base is None or len(onto_base) == len(filters)
        iarr = lambda v: (C.c_int * max(len(v), 1))(*[int(x) for x in v])
        self._chk(lib().bfhip_nupc_render_eq_group_async(self.h, len(filters), iarr(filters), iarr(coeffs),
                                                         None if onto_base is None else iarr(onto_base), eq_taps, len(freq),
                                                         _darr(list(freq)), _darr(list(mag)), _darr(list(phase)), self._eq_mode(mode)))

    def render_eq_base(self, filt, eq_taps, freq, mag, phase, mode="linear"):
        """the same computation alone, synchronous: a numpy array of `taps` reals"""
        assert len(freq) == len(mag) == len(phase)
        out = np.zeros(self.taps, self.dt)
        self._chk(lib().bfhip_nupc_render_eq_base(self.h, filt, eq_taps, len(freq), _darr(list(freq)), _darr(list(mag)),
                                                  _darr(list(phase)), self._eq_mode(mode), _ptr(out)))
        return out

    # parametric equaliser sections rendered on the device (include/bfhip_nupc.h): each call is its band
    # counterpart with the curve given as an (n, 5) array of b0, b1, b2, a1, a2 and a phase "own" / "linear"
    @staticmethod
    def _sections(sections, phase):
        s = np.ascontiguousarray(sections, np.float64)
        assert s.ndim == 2 and s.shape[1] == 5, "sections: an (n, 5) array of b0, b1, b2, a1, a2"
        return len(s), s.ctypes.data_as(C.POINTER(C.c_double)), BIQUAD_PHASES[phase] if isinstance(phase, str) else int(phase), s

    def render_biquads(self, taps, sections, phase="own"):
        """the cascade's response rendered into `taps` reals, synchronous: a numpy array.  phase: "own" (the
        sections' own phase, time-aliased at `taps`, no delay) or "linear" (magnitude alone, taps/2 frames of delay)"""
        n, p, ph, _keep = self._sections(sections, phase)
        out = np.zeros(max(int(taps), 0), self.dt)
        self._chk(lib().bfhip_nupc_render_biquads(self.h, taps, n, p, ph, _ptr(out)))
        return out

    def render_biquads_async(self, filt, coeff, taps, sections, phase="own"):
        """render the cascade into `taps` reals on the device and rewrite an idle set with them; returns at once"""
        n, p, ph, _keep = self._sections(sections, phase)
        self._chk(lib().bfhip_nupc_render_biquads_async(self.h, filt, coeff, taps, n, p, ph))

    def render_biquads_base(self, filt, eq_taps, sections, phase="own"):
        """the cascade rendered into eq_taps reals and convolved onto the filter's base, synchronous: `taps` reals"""
        n, p, ph, _keep = self._sections(sections, phase)
        out = np.zeros(self.taps, self.dt)
        self._chk(lib().bfhip_nupc_render_biquads_base(self.h, filt, eq_taps, n, p, ph, _ptr(out)))
        return out

    def render_biquads_base_async(self, filt, coeff, eq_taps, sections, phase="own"):
        """render_eq_base_async with the curve given as sections; returns at once"""
        n, p, ph, _keep = self._sections(sections, phase)
        self._chk(lib().bfhip_nupc_render_biquads_base_async(self.h, filt, coeff, eq_taps, n, p, ph))

    def render_biquads_group_async(self, filters, coeffs, onto_base, eq_taps, sections, phase="own"):
        """render_eq_group_async with the curve given as sections; returns at once"""
        assert len(filters) == len(coeffs) and (onto_base is None or len(onto_base) == len(filters))
        n, p, ph, _keep = self._sections(sections, phase)
        iarr = lambda v: (C.c_int * max(len(v), 1))(*[int(x) for x in v])
        self._chk(lib().bfhip_nupc_render_biquads_group_async(self.h, len(filters), iarr(filters), iarr(coeffs),
                                                              None if onto_base is None else iarr(onto_base), eq_taps, n, p, ph))

    def set_output_gain(self, ch, gain):
        self._chk(lib().bfhip_nupc_set_output_gain(self.h, ch, gain))

    # per-filter gains and ramped output gain (include/bfhip_nupc.h)
    def reserve_filter_gain(self):
        """before finalize: finalize then allocates what a gain-only switch needs"""
        self._chk(lib().bfhip_nupc_reserve_filter_gain(self.h))

    def set_filter_gain(self, filt, gain):
        """before finalize the filter's initial gain; after it part of the next switch, together
        with the set_coeff calls made before the same block call"""
        self._chk(lib().bfhip_nupc_set_filter_gain(self.h, filt, gain))

    def get_filter_gain(self, filt):
        """the gain of the newest committed assignment"""
        g = lib().bfhip_nupc_get_filter_gain(self.h, filt)
        if g != g:
            raise BfhipError("get_filter_gain: bad argument")
        return g

    def set_gain_ramp(self, frames):
        """ramp length of the set_output_gain calls made from now on; 0 = step"""
        self._chk(lib().bfhip_nupc_set_gain_ramp(self.h, frames))

    def reset_overflow(self):
        """every output's overflow struct back to its initial value, in front of the next block call"""
        self._chk(lib().bfhip_nupc_reset_overflow(self.h))

    def enable_dither(self, channels, sample_rate, max_size=0):
        """HP-TPDF dither on the listed (integer-format) outputs; before finalize"""
        self._chk(lib().bfhip_nupc_enable_dither(self.h, _iarr(list(channels)), len(channels),
                                                 sample_rate, max_size))

    # per-channel integer delay and mute on the raw I/O blocks (dai.c's delay: / maxdelay:, cid /
    # cod, cmi / cmo); io is IN or OUT
    def set_maxdelay(self, io, ch, maxdelay):
        """before finalize; < 0: fixed (the default)"""
        self._chk(lib().bfhip_nupc_set_maxdelay(self.h, io, ch, maxdelay))

    def set_delay(self, io, ch, frames):
        """before finalize the initial delay, after it in force from the next block call; a value
        above maxdelay, or a change of a fixed channel, leaves the delay as it is"""
        self._chk(lib().bfhip_nupc_set_delay(self.h, io, ch, frames))

    def set_mute(self, io, ch, muted):
        self._chk(lib().bfhip_nupc_set_mute(self.h, io, ch, 1 if muted else 0))

    def get_delay(self, io, ch):
        """the delay in force (curdelay)"""
        return self._chk(lib().bfhip_nupc_get_delay(self.h, io, ch))

    # per-channel sub-sample delay (sdf_length: / subdelay:), hundredths of a sample in (-100, 100)
    def enable_subdelay(self, sdf_length, beta=9.0):
        """before finalize; filters of 2 * sdf_length + 1 taps"""
        self._chk(lib().bfhip_nupc_enable_subdelay(self.h, sdf_length, beta))

    def set_subdelay(self, io, ch, value):
        """before finalize: which channels have a filter (UNDEFINED_SUBDELAY = none) and its initial
        value; after it: the value, in force from the next block call"""
        self._chk(lib().bfhip_nupc_set_subdelay(self.h, io, ch, value))

    def get_subdelay(self, io, ch):
        """the value in force, UNDEFINED_SUBDELAY for a channel without a filter"""
        if io not in (IN, OUT) or not 0 <= ch < (self.n_out if io == OUT else self.n_in):
            raise BfhipError("get_subdelay: bad argument")     # (a value may be negative: no code to tell by)
        return lib().bfhip_nupc_get_subdelay(self.h, io, ch)

    # linked look-ahead peak limiter on the outputs (include/bfhip_nupc.h)
    def enable_limiter(self, lookahead_frames, release_frames):
        """before finalize: every output leaves lookahead_frames later"""
        self._chk(lib().bfhip_nupc_enable_limiter(self.h, lookahead_frames, release_frames))

    def add_limiter_group(self, out_channels, threshold):
        """before finalize, after enable_limiter: the channels share one envelope; threshold is a linear
        fraction of full scale (inf: never limits).  Returns the group index"""
        chs = list(out_channels)
        return self._chk(lib().bfhip_nupc_add_limiter_group(self.h, _iarr(chs), len(chs), threshold))

    def set_limiter_threshold(self, group, threshold):
        """in force for the frames of the next block call on"""
        self._chk(lib().bfhip_nupc_set_limiter_threshold(self.h, group, threshold))

    def limiter_threshold(self, group):
        v = lib().bfhip_nupc_get_limiter_threshold(self.h, group)
        if v != v:
            raise BfhipError("limiter_threshold: bad group")
        return v

    def limiter_delay(self):
        """the look-ahead D, 0 without a limiter"""
        return lib().bfhip_nupc_limiter_delay(self.h)

    def limiter_reduction(self, group):
        """the smallest gain the group's envelope applied since the previous call (1.0 if none); waits
        for the main stream"""
        v = C.c_double(1.0)
        self._chk(lib().bfhip_nupc_get_limiter_reduction(self.h, group, C.byref(v)))
        return v.value

    # true-peak detection for the limiter (include/bfhip_nupc.h)
    def set_limiter_detector(self, detector):
        """before finalize, after enable_limiter: LIMIT_SAMPLE_PEAK (the default) or LIMIT_TRUE_PEAK, which
        needs a look-ahead of at least 2 * LIMIT_TP_HALF frames"""
        self._chk(lib().bfhip_nupc_set_limiter_detector(self.h, detector))

    def limiter_detector(self):
        return self._chk(lib().bfhip_nupc_get_limiter_detector(self.h))

    def limiter_true_peak(self, group):
        """true-peak mode: the largest inter-sample peak of the group's channels detected since the previous
        call, as a fraction of full scale (0.0 if none); waits for the main stream"""
        v = C.c_double(0.0)
        self._chk(lib().bfhip_nupc_get_limiter_true_peak(self.h, group, C.byref(v)))
        return v.value


    # BS.1770 loudness meter on the outputs (include/bfhip_nupc.h)
    def enable_loudness(self, sample_rate, history_subblocks=36000):
        """before finalize: sub-blocks of sample_rate / 10 frames, the last history_subblocks of them kept per
        group (36 000: one hour)"""
        self._chk(lib().bfhip_nupc_enable_loudness(self.h, sample_rate, history_subblocks))

    def add_loudness_group(self, out_channels, weights=None):
        """before finalize, after enable_loudness: the channels are metered as one programme with BS.1770's channel
        weights G (None: all 1.0).  Returns the group index"""
        chs = list(out_channels)
        w = None if weights is None else _darr([float(v) for v in weights])
        assert weights is None or len(weights) == len(chs)
        return self._chk(lib().bfhip_nupc_add_loudness_group(self.h, _iarr(chs), w, len(chs)))

    def loudness(self, group):
        """momentary, short-term and gated integrated loudness of the group; waits for the main stream"""
        s = LoudnessStruct()
        self._chk(lib().bfhip_nupc_get_loudness(self.h, group, C.byref(s)))
        return _loudness(s)

    def loudness_energy(self, group, first, count):
        """E[first .. first + count) of the group: complete sub-blocks that are still in the ring"""
        e = np.zeros(max(count, 0), np.float64)
        self._chk(lib().bfhip_nupc_get_loudness_energy(self.h, group, first, count, e.ctypes.data_as(C.POINTER(C.c_double))))
        return e

    def reset_loudness(self, group):
        """the integrated value starts afresh with the next block call; no device work"""
        self._chk(lib().bfhip_nupc_reset_loudness(self.h, group))


def kweighting(sample_rate):
    """the K-weighting sections at sample_rate (bfhip_selftest_kweighting: host only): shelf b0 b1 b2 a1 a2,
    high-pass b0 b1 b2 a1 a2"""
    c = np.zeros(10, np.float64)
    r = lib().bfhip_selftest_kweighting(sample_rate, c.ctypes.data_as(C.POINTER(C.c_double)))
    if r < 0:
        raise BfhipError("bfhip nupc error %d: %s" % (r, lib().bfhip_nupc_last_error().decode()))
    return c


def loudness_energy(sample_rate, v):
    """E[j] of the complete sub-blocks of one channel v (fractions of full scale), weight 1, fresh state
    (bfhip_selftest_loudness_energy: host only, frame by frame)"""
    v = np.ascontiguousarray(v, np.float64)
    e = np.zeros(len(v) // max(sample_rate // 10, 1) + 1, np.float64)
    dp = C.POINTER(C.c_double)
    r = lib().bfhip_selftest_loudness_energy(sample_rate, len(v), v.ctypes.data_as(dp), e.ctypes.data_as(dp))
    if r < 0:
        raise BfhipError("bfhip nupc error %d: %s" % (r, lib().bfhip_nupc_last_error().decode()))
    return e[:r]


def loudness_gate(sample_rate, E):
    """the read-outs of sub-block energies E[0..) (bfhip_selftest_loudness_gate: host only) -> Loudness"""
    E = np.ascontiguousarray(E, np.float64)
    s = LoudnessStruct()
    r = lib().bfhip_selftest_loudness_gate(sample_rate, len(E), E.ctypes.data_as(C.POINTER(C.c_double)), C.byref(s))
    if r < 0:
        raise BfhipError("bfhip nupc error %d: %s" % (r, lib().bfhip_nupc_last_error().decode()))
    return _loudness(s)


def limiter_envelope(lookahead_frames, release_frames, p):
    """s of the limiter's definition from p, fresh state (bfhip_selftest_limiter_envelope: host only,
    needs no device)"""
    p = np.ascontiguousarray(p, np.float64)
    s = np.zeros(len(p), np.float64)
    dp = C.POINTER(C.c_double)
    r = lib().bfhip_selftest_limiter_envelope(lookahead_frames, release_frames, len(p), p.ctypes.data_as(dp),
                                              s.ctypes.data_as(dp))
    if r < 0:
        raise BfhipError("bfhip nupc error %d: %s" % (r, lib().bfhip_nupc_last_error().decode()))
    return s


LIMIT_SAMPLE_PEAK, LIMIT_TRUE_PEAK, LIMIT_TP_HALF = 0, 1, 12


def truepeak_filter():
    """the true-peak interpolator's taps g[q - 1][k], q = 1 .. 3 (bfhip_selftest_truepeak_filter: host only)"""
    g = np.zeros((3, 2 * LIMIT_TP_HALF), np.float64)
    r = lib().bfhip_selftest_truepeak_filter(g.ctypes.data_as(C.POINTER(C.c_double)))
    if r < 0:
        raise BfhipError("bfhip nupc error %d: %s" % (r, lib().bfhip_nupc_last_error().decode()))
    return g


def truepeak(x):
    """max over the four phases of |u_q[t]| for one channel, fresh history (bfhip_selftest_truepeak: host only,
    needs no device)"""
    x = np.ascontiguousarray(x, np.float64)
    tp = np.zeros(len(x), np.float64)
    dp = C.POINTER(C.c_double)
    r = lib().bfhip_selftest_truepeak(len(x), x.ctypes.data_as(dp), tp.ctypes.data_as(dp))
    if r < 0:
        raise BfhipError("bfhip nupc error %d: %s" % (r, lib().bfhip_nupc_last_error().decode()))
    return tp


def device_count():
    return lib().bfhip_device_count()


def biquad_design(type, f0, gain_db, q):
    """one audio-EQ-cookbook section (bfhip_biquad_design: host only, needs no device): five float64
    b0, b1, b2, a1, a2; f0 normalised, 0 < f0 < 0.5"""
    coef = np.zeros(5, np.float64)
    r = lib().bfhip_biquad_design(type, f0, gain_db, q, coef.ctypes.data_as(C.POINTER(C.c_double)))
    if r < 0:
        raise BfhipError("bfhip nupc error %d: %s" % (r, lib().bfhip_nupc_last_error().decode()))
    return coef
