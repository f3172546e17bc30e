"""ctypes view of lib/libcoolmic-dsp-hip.so for tests and bench.py.

Two layers, both thin:
  * `Batch` mirrors the C ABI of include/coolmic_hip.h (the MI355X batch engine);
  * `Transform`, `Vumeter`, `Snddev`, `IoHandle` mirror the reference's per-stream
    operator API of include/coolmic-dsp/*.h (same function names underneath, same
    argument meaning and error numbers), so tests read like tests of the reference.

There is no fallback of any kind: if the shared object is missing, import fails.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("COOLMIC_HIP_LIB") or os.path.join(_HERE, "lib", "libcoolmic-dsp-hip.so")
if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {_HERE}` "
        "(or __graft_entry__.build()); there is no CPU fallback")

lib = C.CDLL(LIB_PATH)

MAX_CH = 16
ssize_t = C.c_ssize_t

# error numbers (include/coolmic-dsp/coolmic-dsp.h)
ERROR_NONE, ERROR_GENERIC, ERROR_NOSYS, ERROR_FAULT = 0, -1, -8, -9
ERROR_INVAL, ERROR_NOMEM, ERROR_BUSY = -10, -11, -12

OUT_PCM, OUT_F32, VU, INPLACE, EQ, HOSTPCM, EXTSLOTS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
PLACE_SEARCH = 0x80
GEN_NULL, GEN_SINE, GEN_NOISE = 0, 1, 2
VU_FINISH_HOST, VU_FINISH_DEVICE = 0, 1
NODE_WORDS = 34

READ_FN = C.CFUNCTYPE(ssize_t, C.c_void_p, C.c_void_p, C.c_size_t)
EOF_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
FREE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)
LOG_FN = C.CFUNCTYPE(C.c_int, C.c_int, C.c_char_p)


class VuResult(C.Structure):
    """coolmic_vumeter_result_t (include/coolmic-dsp/vumeter.h)"""
    _fields_ = [("rate", C.c_uint32), ("channels", C.c_uint), ("frames", C.c_size_t),
                ("global_peak", C.c_int16), ("global_power", C.c_double),
                ("channel_peak", C.c_int16 * MAX_CH), ("channel_power", C.c_double * MAX_CH)]

    def as_dict(self):
        ch = self.channels
        return {"rate": self.rate, "channels": ch, "frames": self.frames,
                "global_peak": self.global_peak, "global_power": self.global_power,
                "channel_peak": [self.channel_peak[i] for i in range(ch)],
                "channel_power": [self.channel_power[i] for i in range(ch)]}


class TruePeakResult(C.Structure):
    """coolmic_truepeak_result_t (include/coolmic-dsp/vumeter.h): peaks in units of 2^-28 of full scale"""
    _fields_ = [("rate", C.c_uint32), ("channels", C.c_uint), ("frames", C.c_size_t),
                ("global_peak", C.c_uint32), ("channel_peak", C.c_uint32 * MAX_CH),
                ("global_dbtp", C.c_double), ("channel_dbtp", C.c_double * MAX_CH)]

    def as_dict(self):
        ch = self.channels
        return {"rate": self.rate, "channels": ch, "frames": self.frames,
                "global_peak": self.global_peak, "global_dbtp": self.global_dbtp,
                "channel_peak": [self.channel_peak[i] for i in range(ch)],
                "channel_dbtp": [self.channel_dbtp[i] for i in range(ch)]}


CORR_MAX_PAIRS = 8


class CorrResult(C.Structure):
    """coolmic_correlation_result_t (include/coolmic-dsp/vumeter.h): exact integer sums per channel pair and their
    finish in double"""
    _fields_ = [("rate", C.c_uint32), ("channels", C.c_uint), ("frames", C.c_size_t), ("pairs", C.c_uint),
                ("a", C.c_ubyte * CORR_MAX_PAIRS), ("b", C.c_ubyte * CORR_MAX_PAIRS),
                ("energy_a", C.c_uint64 * CORR_MAX_PAIRS), ("energy_b", C.c_uint64 * CORR_MAX_PAIRS),
                ("cross", C.c_int64 * CORR_MAX_PAIRS), ("correlation", C.c_double * CORR_MAX_PAIRS),
                ("balance_db", C.c_double * CORR_MAX_PAIRS)]

    def as_dict(self):
        n = self.pairs
        d = {"rate": self.rate, "channels": self.channels, "frames": self.frames, "pairs": n}
        for name in ("a", "b", "energy_a", "energy_b", "cross", "correlation", "balance_db"):
            d[name] = [getattr(self, name)[i] for i in range(n)]
        return d


SPEC_MAX_CHANNELS = 8
SPEC_MAX_BANDS = 32
SPEC_DB_REF = 1649267441664.0           # 1.5 * 2^40


class SpecResult(C.Structure):
    """coolmic_spectrum_result_t (include/coolmic-dsp/vumeter.h): exact integer band sums per selected channel and
    their levels in double"""
    _fields_ = [("rate", C.c_uint32), ("channels", C.c_uint), ("frames", C.c_size_t), ("blocks", C.c_size_t),
                ("fft_log2", C.c_uint), ("bands", C.c_uint), ("selected", C.c_uint),
                ("edges", C.c_uint16 * (SPEC_MAX_BANDS + 1)), ("channel", C.c_ubyte * SPEC_MAX_CHANNELS),
                ("power", (C.c_uint64 * SPEC_MAX_BANDS) * SPEC_MAX_CHANNELS),
                ("db", (C.c_double * SPEC_MAX_BANDS) * SPEC_MAX_CHANNELS)]

    def as_dict(self):
        nb, nc = self.bands, self.selected
        return {"rate": self.rate, "channels": self.channels, "frames": self.frames, "blocks": self.blocks,
                "fft_log2": self.fft_log2, "bands": nb, "selected": nc,
                "edges": [self.edges[i] for i in range(nb + 1)], "channel": [self.channel[i] for i in range(nc)],
                "power": [[self.power[c][k] for k in range(nb)] for c in range(nc)],
                "db": [[self.db[c][k] for k in range(nb)] for c in range(nc)]}


class WatchResult(C.Structure):
    """coolmic_watch_result_t (include/coolmic-dsp/vumeter.h): dead air, quiet channels, samples at the rail and the
    channel sums of one window, exact integers, and the DC finish in double"""
    _fields_ = [("rate", C.c_uint32), ("channels", C.c_uint), ("frames", C.c_size_t),
                ("quiet", C.c_uint), ("rail", C.c_uint), ("clip_run", C.c_uint),
                ("dead_frames", C.c_uint64), ("dead_longest", C.c_uint64), ("dead_current", C.c_uint64),
                ("quiet_frames", C.c_uint64 * MAX_CH), ("quiet_longest", C.c_uint64 * MAX_CH),
                ("quiet_current", C.c_uint64 * MAX_CH),
                ("clip_samples", C.c_uint64 * MAX_CH), ("clip_events", C.c_uint64 * MAX_CH),
                ("clip_longest", C.c_uint64 * MAX_CH),
                ("sum", C.c_int64 * MAX_CH), ("dc", C.c_double * MAX_CH)]

    def as_dict(self):
        ch = self.channels
        d = {n: getattr(self, n) for n in ("rate", "channels", "frames", "quiet", "rail", "clip_run", "dead_frames",
                                           "dead_longest", "dead_current")}
        for name in ("quiet_frames", "quiet_longest", "quiet_current", "clip_samples", "clip_events", "clip_longest",
                     "sum", "dc"):
            d[name] = [getattr(self, name)[i] for i in range(ch)]
        return d


class LoudnessResult(C.Structure):
    """coolmic_loudness_result_t (include/coolmic-dsp/vumeter.h): LUFS doubles, -inf while there is nothing to report"""
    _fields_ = [("rate", C.c_uint32), ("channels", C.c_uint), ("frames", C.c_size_t), ("blocks", C.c_size_t),
                ("gated_blocks", C.c_size_t), ("momentary", C.c_double), ("short_term", C.c_double),
                ("integrated", C.c_double), ("relative_threshold", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BatchDesc(C.Structure):
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint),
                ("rate", C.c_uint), ("max_frames", C.c_size_t), ("flags", C.c_uint),
                ("hip_stream", C.c_void_p)]


class SrcDesc(C.Structure):
    """cmhip_src_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("rate_in", C.c_uint),
                ("rate_out", C.c_uint), ("max_in_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


class DriftDesc(C.Structure):
    """cmhip_drift_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("max_in_frames", C.c_size_t),
                ("hip_stream", C.c_void_p)]


class DriftServo(C.Structure):
    """cmhip_drift_servo_t (include/coolmic_hip.h)"""
    _fields_ = [("target", C.c_int64), ("integ", C.c_int64), ("kp_log2", C.c_uint32), ("ki_log2", C.c_uint32),
                ("limit", C.c_int32), ("delta", C.c_int32), ("clamped", C.c_uint32)]


class MixDesc(C.Structure):
    """cmhip_mix_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels_in", C.c_uint), ("channels_out", C.c_uint),
                ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


class BusDesc(C.Structure):
    """cmhip_bus_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("buses", C.c_uint), ("channels_in", C.c_uint),
                ("channels_out", C.c_uint), ("max_frames", C.c_size_t), ("max_sends", C.c_size_t),
                ("hip_stream", C.c_void_p)]


class LimDesc(C.Structure):
    """cmhip_lim_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("lookahead_log2", C.c_uint),
                ("hold", C.c_uint), ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


class DynDesc(C.Structure):
    """cmhip_dyn_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("detector_log2", C.c_uint),
                ("smooth_log2", C.c_uint), ("hold", C.c_uint), ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


class SplitDesc(C.Structure):
    """cmhip_split_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("bands", C.c_uint),
                ("taps", C.c_uint), ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


class DelayDesc(C.Structure):
    """cmhip_delay_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("max_delay", C.c_size_t),
                ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


class AgcDesc(C.Structure):
    """cmhip_agc_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("window_log2", C.c_uint),
                ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


AGC_PARAM_NAMES = ("target", "gate", "gain_min", "gain_max", "rise", "fall", "initial")


class AgcParams(C.Structure):
    """cmhip_agc_params_t (include/coolmic_hip.h)"""
    _fields_ = [(n, C.c_uint16) for n in AGC_PARAM_NAMES]

    def as_dict(self):
        return {n: getattr(self, n) for n in AGC_PARAM_NAMES}


class AgcLawDesc(C.Structure):
    """cmhip_agc_law_desc_t (include/coolmic_hip.h)"""
    _fields_ = [(n, C.c_double) for n in ("rate", "window_log2", "target_db", "gate_db", "max_gain_db", "min_gain_db",
                                          "initial_gain_db", "rise_db_per_s", "fall_db_per_s")]


class DenoiseDesc(C.Structure):
    """cmhip_denoise_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("fft_log2", C.c_uint),
                ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


DENOISE_PARAM_NAMES = ("floor", "over", "rise_shift", "fall_shift")


class DenoiseParams(C.Structure):
    """cmhip_denoise_params_t (include/coolmic_hip.h)"""
    _fields_ = [("floor", C.c_uint16), ("over", C.c_uint8), ("rise_shift", C.c_uint8), ("fall_shift", C.c_uint8)]

    def as_dict(self):
        return {n: getattr(self, n) for n in DENOISE_PARAM_NAMES}


class DenoiseLawDesc(C.Structure):
    """cmhip_denoise_law_desc_t (include/coolmic_hip.h)"""
    _fields_ = [(n, C.c_double) for n in ("rate", "fft_log2", "reduction_db", "over_db", "attack_ms", "release_ms")]


class AutomixDesc(C.Structure):
    """cmhip_automix_desc_t (include/coolmic_hip.h)"""
    _fields_ = AgcDesc._fields_


AUTOMIX_PARAM_NAMES = ("weight", "floor", "attack", "release", "initial")


class AutomixParams(C.Structure):
    """cmhip_automix_params_t (include/coolmic_hip.h)"""
    _fields_ = [(n, C.c_uint16) for n in AUTOMIX_PARAM_NAMES]

    def as_dict(self):
        return {n: getattr(self, n) for n in AUTOMIX_PARAM_NAMES}


class AutomixLawDesc(C.Structure):
    """cmhip_automix_law_desc_t (include/coolmic_hip.h)"""
    _fields_ = [(n, C.c_double) for n in ("rate", "window_log2", "weight_db", "floor_db", "initial_db", "attack_ms",
                                          "release_ms")]


class FailoverDesc(C.Structure):
    """cmhip_failover_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("outputs", C.c_uint), ("channels", C.c_uint),
                ("window_log2", C.c_uint), ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


class FailoverParams(C.Structure):
    """cmhip_failover_params_t (include/coolmic_hip.h)"""
    _fields_ = [("quiet", C.c_uint16 * 4), ("fail_windows", C.c_uint16), ("return_windows", C.c_uint16),
                ("fade_log2", C.c_uint16), ("force", C.c_int16)]

    def as_dict(self):
        return {"quiet": tuple(self.quiet), "fail_windows": self.fail_windows, "return_windows": self.return_windows,
                "fade_log2": self.fade_log2, "force": self.force}


class FailoverLawDesc(C.Structure):
    """cmhip_failover_law_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("rate", C.c_double), ("window_log2", C.c_double), ("quiet_db", C.c_double * 4), ("fail_s", C.c_double),
                ("return_s", C.c_double), ("fade_ms", C.c_double)]


class IirDesc(C.Structure):
    """cmhip_iir_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("device", C.c_int), ("streams", C.c_uint), ("channels", C.c_uint), ("sections", C.c_uint),
                ("max_frames", C.c_size_t), ("hip_stream", C.c_void_p)]


IIR_ONE = 1 << 26
IIR_COEF_NAMES = ("b0", "b1", "b2", "a1", "a2")
IIR_KINDS = ("BYPASS", "HIGHPASS", "LOWPASS", "LOWSHELF", "HIGHSHELF", "PEAK", "NOTCH", "HIGHPASS1", "LOWPASS1")
(IIR_BYPASS, IIR_HIGHPASS, IIR_LOWPASS, IIR_LOWSHELF, IIR_HIGHSHELF, IIR_PEAK, IIR_NOTCH, IIR_HIGHPASS1,
 IIR_LOWPASS1) = range(9)


class IirSection(C.Structure):
    """cmhip_iir_section_t (include/coolmic_hip.h): b0, b1, b2, a1, a2 in units of 2^-26"""
    _fields_ = [(n, C.c_int32) for n in IIR_COEF_NAMES]

    def as_tuple(self):
        return tuple(getattr(self, n) for n in IIR_COEF_NAMES)


class IirDesignDesc(C.Structure):
    """cmhip_iir_design_desc_t (include/coolmic_hip.h)"""
    _fields_ = [("kind", C.c_int), ("rate", C.c_double), ("f0", C.c_double), ("q", C.c_double), ("gain_db", C.c_double)]


class DynCurveDesc(C.Structure):
    """cmhip_dyn_curve_desc_t (include/coolmic_hip.h)"""
    _fields_ = [(n, C.c_double) for n in ("comp_threshold_db", "comp_ratio", "comp_knee_db", "gate_threshold_db",
                                          "gate_ratio", "gate_range_db")]


class DynDuckDesc(C.Structure):
    """cmhip_dyn_duck_desc_t (include/coolmic_hip.h)"""
    _fields_ = [(n, C.c_double) for n in ("threshold_db", "depth_db", "knee_db")]


class Placement(C.Structure):
    """cmhip_placement_t (include/coolmic_hip.h)"""
    _fields_ = [("searched", C.c_int), ("candidates", C.c_int), ("chosen_in", C.c_int),
                ("chosen_out", C.c_int), ("probe_launches", C.c_int), ("first_pair_ms", C.c_double),
                ("best_pair_ms", C.c_double), ("search_ms", C.c_double),
                ("bytes_requested", C.c_uint64), ("bytes_free_before", C.c_uint64)]

    def as_dict(self):
        return {"searched": bool(self.searched), "candidates": self.candidates,
                "chosen": [self.chosen_in, self.chosen_out], "probe_launches": self.probe_launches,
                "first_pair_ms": round(self.first_pair_ms, 4), "best_pair_ms": round(self.best_pair_ms, 4),
                "search_ms": round(self.search_ms, 1),
                "GiB_requested": round(self.bytes_requested / 2**30, 2),
                "GiB_free_before": round(self.bytes_free_before / 2**30, 2)}


def _sig(name, res, args):
    fn = getattr(lib, name)
    fn.restype = res
    fn.argtypes = args
    return fn


_P = C.POINTER
_vp = C.c_void_p
# every symbol include/*.h declares; tests/test_abi.py checks this table against the headers
SIGNATURES = {
    # include/coolmic_hip.h
    "cmhip_device_count": (C.c_int, []),
    "cmhip_device_synchronize": (C.c_int, [C.c_int]),
    "cmhip_device_mem_info": (C.c_int, [C.c_int, _P(C.c_size_t), _P(C.c_size_t)]),
    "cmhip_device_alloc": (_vp, [C.c_int, C.c_size_t]),
    "cmhip_device_free": (None, [C.c_int, _vp]),
    "cmhip_device_read": (C.c_int, [C.c_int, _vp, _vp, C.c_size_t]),
    "cmhip_last_error": (C.c_char_p, []),
    "cmhip_version": (C.c_char_p, []),
    "cmhip_batch_new": (_vp, [_P(BatchDesc)]),
    "cmhip_batch_free": (None, [_vp]),
    "cmhip_batch_placement": (C.c_int, [_vp, _P(Placement)]),
    "cmhip_batch_set_gain": (C.c_int, [_vp, C.c_long, C.c_uint, C.c_uint16, _P(C.c_uint16)]),
    "cmhip_batch_set_chmap": (C.c_int, [_vp, C.c_long, _vp]),
    "cmhip_batch_set_eq": (C.c_int, [_vp, C.c_long, C.c_uint, _vp]),
    "cmhip_batch_eq_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_design_biquad": (None, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, _vp]),
    "cmhip_batch_stride": (C.c_size_t, [_vp]),
    "cmhip_batch_max_frames": (C.c_size_t, [_vp]),
    "cmhip_batch_dev_in": (_vp, [_vp]),
    "cmhip_batch_dev_out": (_vp, [_vp]),
    "cmhip_batch_dev_f32": (_vp, [_vp]),
    "cmhip_batch_hip_stream": (_vp, [_vp]),
    "cmhip_batch_upload": (C.c_int, [_vp, C.c_uint, _vp, C.c_size_t]),
    "cmhip_batch_download": (C.c_int, [_vp, C.c_uint, _vp, C.c_size_t]),
    "cmhip_batch_upload_all": (C.c_int, [_vp, _vp, C.c_size_t]),
    "cmhip_batch_download_all": (C.c_int, [_vp, _vp, C.c_size_t]),
    "cmhip_host_alloc": (_vp, [C.c_size_t]),
    "cmhip_host_free": (None, [_vp]),
    "cmhip_batch_download_input": (C.c_int, [_vp, C.c_uint, _vp, C.c_size_t]),
    "cmhip_batch_download_f32": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp, C.c_size_t]),
    "cmhip_batch_generate": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_size_t, C.c_uint64,
                                       C.c_uint64, C.c_uint64]),
    "cmhip_batch_run": (C.c_int, [_vp, C.c_size_t, _vp]),
    "cmhip_batch_sync": (C.c_int, [_vp]),
    "cmhip_batch_vu_result": (C.c_int, [_vp, C.c_uint, _P(VuResult)]),
    "cmhip_batch_vu_results": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_batch_vu_snapshot": (C.c_int, [_vp]),
    "cmhip_batch_vu_collect": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_batch_vu_collect_begin": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_batch_vu_collect_end": (C.c_int, [_vp]),
    "cmhip_batch_vu_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_batch_vu_set_finish": (C.c_int, [_vp, C.c_int]),
    "cmhip_batch_vu_get_finish": (C.c_int, [_vp]),
    "cmhip_batch_vu_raw": (C.c_int, [_vp, C.c_uint, _vp, _vp, _P(C.c_uint64)]),
    "cmhip_batch_set_true_peak": (C.c_int, [_vp, C.c_int]),
    "cmhip_batch_get_true_peak": (C.c_int, [_vp]),
    "cmhip_batch_tp_result": (C.c_int, [_vp, C.c_uint, _P(TruePeakResult)]),
    "cmhip_batch_tp_results": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_batch_tp_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_tp_dbtp": (C.c_double, [C.c_uint32]),
    "cmhip_tp_coefficients": (None, [_vp]),
    "cmhip_batch_set_correlation": (C.c_int, [_vp, C.c_int]),
    "cmhip_batch_get_correlation": (C.c_int, [_vp]),
    "cmhip_batch_corr_set_pairs": (C.c_int, [_vp, C.c_uint, _vp]),
    "cmhip_batch_corr_result": (C.c_int, [_vp, C.c_uint, _P(CorrResult)]),
    "cmhip_batch_corr_results": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_batch_corr_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_batch_set_watch": (C.c_int, [_vp, C.c_int]),
    "cmhip_batch_get_watch": (C.c_int, [_vp]),
    "cmhip_batch_watch_configure": (C.c_int, [_vp, C.c_uint, C.c_uint, C.c_uint]),
    "cmhip_batch_watch_result": (C.c_int, [_vp, C.c_uint, _P(WatchResult)]),
    "cmhip_batch_watch_results": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_batch_watch_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_watch_level": (C.c_uint, [C.c_double]),
    "cmhip_corr_value": (C.c_double, [C.c_uint64, C.c_uint64, C.c_int64]),
    "cmhip_corr_balance_db": (C.c_double, [C.c_uint64, C.c_uint64]),
    "cmhip_batch_set_spectrum": (C.c_int, [_vp, C.c_int]),
    "cmhip_batch_get_spectrum": (C.c_int, [_vp]),
    "cmhip_batch_spec_configure": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp, C.c_uint, _vp]),
    "cmhip_batch_spec_result": (C.c_int, [_vp, C.c_uint, _P(SpecResult)]),
    "cmhip_batch_spec_results": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_batch_spec_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_spec_window": (C.c_int, [C.c_uint, _vp]),
    "cmhip_spec_twiddles": (C.c_int, [C.c_uint, _vp, _vp]),
    "cmhip_spec_design_bands": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, _vp]),
    "cmhip_spec_db": (C.c_double, [C.c_uint64, C.c_uint64]),
    "cmhip_batch_set_loudness": (C.c_int, [_vp, C.c_int]),
    "cmhip_batch_get_loudness": (C.c_int, [_vp]),
    "cmhip_batch_loud_set_weights": (C.c_int, [_vp, C.c_long, _vp]),
    "cmhip_batch_loud_result": (C.c_int, [_vp, C.c_uint, _P(LoudnessResult)]),
    "cmhip_batch_loud_results": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_batch_loud_raw": (C.c_int, [_vp, C.c_uint, _vp, C.c_size_t, _P(C.c_size_t), _P(C.c_ulonglong)]),
    "cmhip_batch_loud_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_loud_coefficients": (None, [C.c_uint, _vp]),
    "cmhip_loud_lufs": (C.c_double, [C.c_double]),
    "cmhip_loud_integrate": (C.c_int, [_vp, C.c_size_t, _P(C.c_double), _P(C.c_double), _P(C.c_size_t)]),
    "cmhip_src_new": (_vp, [_P(SrcDesc)]),
    "cmhip_src_new_table": (_vp, [_P(SrcDesc), C.c_uint, C.c_uint, C.c_uint, _vp]),
    "cmhip_src_free": (None, [_vp]),
    "cmhip_src_geometry": (C.c_int, [_vp, _P(C.c_uint), _P(C.c_uint), _P(C.c_uint)]),
    "cmhip_src_max_out_frames": (C.c_size_t, [_vp]),
    "cmhip_src_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "cmhip_src_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_src_sync": (C.c_int, [_vp]),
    "cmhip_src_hip_stream": (_vp, [_vp]),
    "cmhip_src_design": (C.c_int, [C.c_uint, C.c_uint, _P(C.c_uint), _P(C.c_uint), _P(C.c_uint), _vp, C.c_size_t]),
    "cmhip_src_out_frames": (C.c_uint32, [C.c_uint, C.c_uint, C.c_uint32, C.c_uint32]),
    "cmhip_split_new": (_vp, [_P(SplitDesc), C.c_uint, _P(C.c_double)]),
    "cmhip_split_new_table": (_vp, [_P(SplitDesc), _vp, _vp]),
    "cmhip_split_free": (None, [_vp]),
    "cmhip_split_delay": (C.c_uint, [_vp]),
    "cmhip_split_get_table": (C.c_int, [_vp, _vp, _vp]),
    "cmhip_split_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_split_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_split_clips": (C.c_int, [_vp, _vp, C.c_int]),
    "cmhip_split_sync": (C.c_int, [_vp]),
    "cmhip_split_hip_stream": (_vp, [_vp]),
    "cmhip_split_design": (C.c_int, [C.c_uint, C.c_uint, _P(C.c_double), C.c_uint, _vp, _vp, C.c_size_t]),
    "cmhip_split_check": (C.c_int, [C.c_uint, C.c_uint, _vp, _vp]),
    "cmhip_delay_new": (_vp, [_P(DelayDesc)]),
    "cmhip_delay_free": (None, [_vp]),
    "cmhip_delay_set": (C.c_int, [_vp, C.c_long, C.c_uint32]),
    "cmhip_delay_ramp": (C.c_int, [_vp, C.c_long, C.c_uint32, C.c_uint32]),
    "cmhip_delay_get": (C.c_int, [_vp, C.c_uint, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "cmhip_delay_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_delay_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_delay_sync": (C.c_int, [_vp]),
    "cmhip_delay_hip_stream": (_vp, [_vp]),
    "cmhip_delay_max_delay": (C.c_size_t, [_vp]),
    "cmhip_delay_ms": (C.c_uint32, [C.c_uint, C.c_double]),
    "cmhip_delay_crossfade": (C.c_int16, [C.c_int16, C.c_int16, C.c_uint32]),
    "cmhip_agc_new": (_vp, [_P(AgcDesc)]),
    "cmhip_agc_free": (None, [_vp]),
    "cmhip_agc_set": (C.c_int, [_vp, C.c_long, _P(AgcParams)]),
    "cmhip_agc_get": (C.c_int, [_vp, C.c_uint, _P(AgcParams)]),
    "cmhip_agc_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_agc_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_agc_state": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int]),
    "cmhip_agc_sync": (C.c_int, [_vp]),
    "cmhip_agc_hip_stream": (_vp, [_vp]),
    "cmhip_agc_check": (C.c_int, [C.c_uint, _P(AgcParams)]),
    "cmhip_agc_design": (C.c_int, [_P(AgcLawDesc), _P(AgcParams)]),
    "cmhip_automix_new": (_vp, [_P(AutomixDesc)]),
    "cmhip_automix_free": (None, [_vp]),
    "cmhip_automix_set": (C.c_int, [_vp, C.c_long, _P(AutomixParams)]),
    "cmhip_automix_get": (C.c_int, [_vp, C.c_uint, _P(AutomixParams)]),
    "cmhip_automix_set_group": (C.c_int, [_vp, C.c_long, C.c_long]),
    "cmhip_automix_get_group": (C.c_int, [_vp, C.c_uint, _P(C.c_long)]),
    "cmhip_automix_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_automix_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_automix_state": (C.c_int, [_vp, _vp, _vp, _vp]),
    "cmhip_automix_sync": (C.c_int, [_vp]),
    "cmhip_automix_hip_stream": (_vp, [_vp]),
    "cmhip_automix_check": (C.c_int, [C.c_uint, _P(AutomixParams)]),
    "cmhip_automix_design": (C.c_int, [_P(AutomixLawDesc), _P(AutomixParams)]),
    "cmhip_drift_new": (_vp, [_P(DriftDesc)]),
    "cmhip_drift_new_table": (_vp, [_P(DriftDesc), C.c_uint, C.c_uint, _vp]),
    "cmhip_drift_free": (None, [_vp]),
    "cmhip_drift_geometry": (C.c_int, [_vp, _P(C.c_uint), _P(C.c_uint)]),
    "cmhip_drift_max_out_frames": (C.c_size_t, [_vp]),
    "cmhip_drift_set": (C.c_int, [_vp, C.c_long, C.c_int32]),
    "cmhip_drift_seek": (C.c_int, [_vp, C.c_long, C.c_uint64]),
    "cmhip_drift_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_drift_get": (C.c_int, [_vp, C.c_uint, _P(C.c_int32), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "cmhip_drift_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "cmhip_drift_sync": (C.c_int, [_vp]),
    "cmhip_drift_hip_stream": (_vp, [_vp]),
    "cmhip_drift_design": (C.c_int, [C.c_uint, C.c_uint, _vp, C.c_size_t]),
    "cmhip_drift_out_frames": (C.c_uint32, [C.c_uint64, C.c_int32, C.c_uint32]),
    "cmhip_drift_ppm": (C.c_int32, [C.c_double]),
    "cmhip_drift_to_ppm": (C.c_double, [C.c_int32]),
    "cmhip_drift_servo_init": (C.c_int, [_P(DriftServo), C.c_uint32, C.c_uint, C.c_uint, C.c_int32]),
    "cmhip_drift_servo_step": (C.c_int32, [_P(DriftServo), C.c_int64]),
    "cmhip_drift_servo_reset": (None, [_P(DriftServo)]),
    "cmhip_failover_new": (_vp, [_P(FailoverDesc)]),
    "cmhip_failover_free": (None, [_vp]),
    "cmhip_failover_set_sources": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp]),
    "cmhip_failover_get_sources": (C.c_int, [_vp, C.c_uint, _P(C.c_uint), _vp]),
    "cmhip_failover_set": (C.c_int, [_vp, C.c_long, _P(FailoverParams)]),
    "cmhip_failover_get": (C.c_int, [_vp, C.c_uint, _P(FailoverParams)]),
    "cmhip_failover_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_failover_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_failover_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "cmhip_failover_sync": (C.c_int, [_vp]),
    "cmhip_failover_hip_stream": (_vp, [_vp]),
    "cmhip_failover_check": (C.c_int, [C.c_uint, C.c_uint, _P(FailoverParams)]),
    "cmhip_failover_design": (C.c_int, [_P(FailoverLawDesc), _P(FailoverParams)]),
    "cmhip_failover_step": (C.c_uint32, [C.c_uint, _P(FailoverParams), C.c_uint32, _vp, _vp]),
    "cmhip_iir_new": (_vp, [_P(IirDesc)]),
    "cmhip_iir_free": (None, [_vp]),
    "cmhip_iir_set": (C.c_int, [_vp, C.c_long, C.c_uint, _P(IirSection)]),
    "cmhip_iir_get": (C.c_int, [_vp, C.c_uint, C.c_uint, _P(IirSection)]),
    "cmhip_iir_ramp": (C.c_int, [_vp, C.c_long, C.c_uint, _P(IirSection), C.c_uint32]),
    "cmhip_iir_ramp_state": (C.c_int, [_vp, C.c_uint, C.c_uint, _P(C.c_uint32), _P(C.c_uint32)]),
    "cmhip_iir_ramp_section": (None, [_P(IirSection), _P(IirSection), C.c_uint32, _P(IirSection)]),
    "cmhip_iir_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_iir_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_iir_state": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "cmhip_iir_sync": (C.c_int, [_vp]),
    "cmhip_iir_hip_stream": (_vp, [_vp]),
    "cmhip_iir_check": (C.c_int, [_P(IirSection)]),
    "cmhip_iir_design": (C.c_int, [_P(IirDesignDesc), _P(IirSection)]),
    "cmhip_iir_response_db": (C.c_double, [_P(IirSection), C.c_uint, C.c_double, C.c_double]),
    "cmhip_denoise_new": (_vp, [_P(DenoiseDesc)]),
    "cmhip_denoise_free": (None, [_vp]),
    "cmhip_denoise_set": (C.c_int, [_vp, C.c_long, _P(DenoiseParams)]),
    "cmhip_denoise_get": (C.c_int, [_vp, C.c_uint, _P(DenoiseParams)]),
    "cmhip_denoise_learn": (C.c_int, [_vp, C.c_long, C.c_int]),
    "cmhip_denoise_set_profile": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp]),
    "cmhip_denoise_get_profile": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp, _vp]),
    "cmhip_denoise_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_denoise_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_denoise_state": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int]),
    "cmhip_denoise_sync": (C.c_int, [_vp]),
    "cmhip_denoise_hip_stream": (_vp, [_vp]),
    "cmhip_denoise_delay": (C.c_size_t, [_vp]),
    "cmhip_denoise_check": (C.c_int, [C.c_uint, _P(DenoiseParams)]),
    "cmhip_denoise_window": (C.c_int, [C.c_uint, _vp]),
    "cmhip_denoise_design": (C.c_int, [_P(DenoiseLawDesc), _P(DenoiseParams)]),
    "cmhip_denoise_gain": (C.c_uint32, [C.c_uint64, C.c_uint64, C.c_uint, C.c_uint]),
    "cmhip_mix_new": (_vp, [_P(MixDesc)]),
    "cmhip_mix_free": (None, [_vp]),
    "cmhip_mix_set_matrix": (C.c_int, [_vp, C.c_long, _vp]),
    "cmhip_mix_get_matrix": (C.c_int, [_vp, C.c_uint, _vp]),
    "cmhip_mix_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_mix_sync": (C.c_int, [_vp]),
    "cmhip_mix_hip_stream": (_vp, [_vp]),
    "cmhip_mix_check": (C.c_int, [C.c_uint, C.c_uint, _vp]),
    "cmhip_mix_preset": (C.c_int, [C.c_uint, _P(C.c_uint), _P(C.c_uint), _vp, C.c_size_t]),
    "cmhip_mix_ramp_matrix": (C.c_int, [_vp, C.c_long, _vp, C.c_uint32]),
    "cmhip_mix_ramp_state": (C.c_int, [_vp, C.c_uint, _P(C.c_uint32), _P(C.c_uint32), _vp]),
    "cmhip_mix_ramp_position": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "cmhip_mix_ramp_weight": (C.c_int16, [C.c_int16, C.c_int16, C.c_uint32]),
    "cmhip_bus_new": (_vp, [_P(BusDesc)]),
    "cmhip_bus_free": (None, [_vp]),
    "cmhip_bus_set_routing": (C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp]),
    "cmhip_bus_sends": (C.c_size_t, [_vp]),
    "cmhip_bus_get_routing": (C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp]),
    "cmhip_bus_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _vp]),
    "cmhip_bus_sync": (C.c_int, [_vp]),
    "cmhip_bus_hip_stream": (_vp, [_vp]),
    "cmhip_bus_check": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_size_t, _vp, _vp, _vp]),
    "cmhip_bus_mix_minus": (C.c_int, [C.c_uint, C.c_int16, _vp, _vp, _vp, C.c_size_t, C.c_uint]),
    "cmhip_bus_ramp_sends": (C.c_int, [_vp, C.c_size_t, C.c_size_t, _vp, C.c_uint32]),
    "cmhip_bus_ramp_state": (C.c_int, [_vp, C.c_size_t, _P(C.c_uint32), _P(C.c_uint32), _vp]),
    "cmhip_lim_new": (_vp, [_P(LimDesc)]),
    "cmhip_lim_free": (None, [_vp]),
    "cmhip_lim_delay": (C.c_uint, [_vp]),
    "cmhip_lim_set": (C.c_int, [_vp, C.c_long, C.c_uint, C.c_uint]),
    "cmhip_lim_get": (C.c_int, [_vp, C.c_uint, _P(C.c_uint), _P(C.c_uint)]),
    "cmhip_lim_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_lim_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_lim_min_gain": (C.c_int, [_vp, _vp, C.c_int]),
    "cmhip_lim_sync": (C.c_int, [_vp]),
    "cmhip_lim_hip_stream": (_vp, [_vp]),
    "cmhip_lim_check": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "cmhip_lim_new_detector": (_vp, [_P(LimDesc), C.c_uint]),
    "cmhip_lim_detector": (C.c_uint, [_vp]),
    "cmhip_lim_check_detector": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "cmhip_lim_threshold_dbtp": (C.c_uint, [C.c_double]),
    "cmhip_lim_new_release": (_vp, [_P(LimDesc), C.c_uint, C.c_uint]),
    "cmhip_lim_release": (C.c_uint, [_vp]),
    "cmhip_lim_check_release": (C.c_int, [C.c_uint] * 6),
    "cmhip_dyn_new": (_vp, [_P(DynDesc)]),
    "cmhip_dyn_free": (None, [_vp]),
    "cmhip_dyn_delay": (C.c_uint, [_vp]),
    "cmhip_dyn_set_curve": (C.c_int, [_vp, C.c_long, _vp]),
    "cmhip_dyn_get_curve": (C.c_int, [_vp, C.c_uint, _vp]),
    "cmhip_dyn_run": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t]),
    "cmhip_dyn_reset": (C.c_int, [_vp, C.c_long]),
    "cmhip_dyn_min_gain": (C.c_int, [_vp, _vp, C.c_int]),
    "cmhip_dyn_sync": (C.c_int, [_vp]),
    "cmhip_dyn_hip_stream": (_vp, [_vp]),
    "cmhip_dyn_check": (C.c_int, [C.c_uint, C.c_uint, C.c_uint]),
    "cmhip_dyn_design": (C.c_int, [_P(DynCurveDesc), _vp]),
    "cmhip_dyn_set_key": (C.c_int, [_vp, C.c_long, C.c_long]),
    "cmhip_dyn_get_key": (C.c_int, [_vp, C.c_uint, _P(C.c_long)]),
    "cmhip_dyn_design_duck": (C.c_int, [_P(DynDuckDesc), _vp]),
    "cmhip_dyn_new_detector": (_vp, [_P(DynDesc), C.c_uint]),
    "cmhip_dyn_detector": (C.c_uint, [_vp]),
    "cmhip_dyn_check_detector": (C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "cmhip_batch_vu_node_partial": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64]),
    "cmhip_batch_vu_node_record": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64]),
    "cmhip_node_finish": (C.c_int, [_vp, C.c_uint, C.c_uint, _P(VuResult)]),
    "cmhip_batch_run_slots": (C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp]),
    "cmhip_host_alloc_mapped": (_vp, [C.c_size_t, _P(_vp)]),
    "cmhip_node_unique_id": (C.c_int, [_vp]),
    "cmhip_node_new": (_vp, [C.c_int, C.c_int, C.c_int, _vp, C.c_uint]),
    "cmhip_node_free": (None, [_vp]),
    "cmhip_node_ranks": (C.c_int, [_vp]),
    "cmhip_node_runtime": (C.c_char_p, []),
    "cmhip_node_partial": (C.c_int, [_vp, _vp, C.c_uint, C.c_uint, C.c_uint64, C.c_uint64]),
    "cmhip_node_allreduce": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp]),
    "cmhip_node_fetch": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp]),
    "cmhip_node_merge_host": (C.c_int, [_vp, C.c_uint, _vp]),
    "cmhip_batch_timing": (C.c_int, [_vp, C.c_int]),
    "cmhip_batch_timing_read": (C.c_int, [_vp, _P(C.c_double), _P(C.c_uint)]),
    "cmhip_batch_ceiling": (C.c_double, [_vp, C.c_int, C.c_size_t, C.c_int]),
    # include/coolmic-dsp/ro-compat.h
    "coolmic_ro_new_raw": (_vp, [_vp, C.c_char_p, _vp]),
    "coolmic_ro_ref": (C.c_int, [_vp]),
    "coolmic_ro_unref": (C.c_int, [_vp]),
    "coolmic_ro_refcount": (C.c_uint, [_vp]),
    # include/coolmic-dsp/coolmic-dsp.h
    "coolmic_error2string": (C.c_char_p, [C.c_int]),
    "coolmic_features": (C.c_char_p, []),
    "coolmic_feature_check": (C.c_int, [C.c_char_p]),
    # include/coolmic-dsp/logging.h
    "coolmic_logging_level2string": (C.c_char_p, [C.c_int]),
    "coolmic_logging_log_real": (C.c_int, None),
    "coolmic_logging_set_cb_simple": (C.c_int, [LOG_FN]),
    # include/coolmic-dsp/iohandle.h
    "coolmic_iohandle_new": (_vp, [C.c_char_p, _vp, _vp, FREE_FN, READ_FN, EOF_FN]),
    "coolmic_iohandle_read": (ssize_t, [_vp, _vp, C.c_size_t]),
    "coolmic_iohandle_eof": (C.c_int, [_vp]),
    # include/coolmic-dsp/transform.h
    "coolmic_transform_new": (_vp, [C.c_char_p, _vp, C.c_uint32, C.c_uint]),
    "coolmic_transform_attach_iohandle": (C.c_int, [_vp, _vp]),
    "coolmic_transform_get_iohandle": (_vp, [_vp]),
    "coolmic_transform_set_master_gain": (C.c_int, [_vp, C.c_uint, C.c_uint16, _P(C.c_uint16)]),
    "coolmic_transform_set_channel_map": (C.c_int, [_vp, _vp]),
    "coolmic_transform_set_eq": (C.c_int, [_vp, C.c_uint, _vp]),
    # include/coolmic-dsp/vumeter.h
    "coolmic_vumeter_new": (_vp, [C.c_char_p, _vp, C.c_uint32, C.c_uint]),
    "coolmic_vumeter_reset": (C.c_int, [_vp]),
    "coolmic_vumeter_attach_iohandle": (C.c_int, [_vp, _vp]),
    "coolmic_vumeter_read": (ssize_t, [_vp, ssize_t]),
    "coolmic_vumeter_result": (C.c_int, [_vp, _P(VuResult)]),
    # include/coolmic-dsp/snddev.h
    "coolmic_snddev_new": (_vp, [C.c_char_p, _vp, C.c_char_p, _vp, C.c_uint32, C.c_uint, C.c_int,
                                 ssize_t]),
    "coolmic_snddev_get_iohandle": (_vp, [_vp]),
    "coolmic_snddev_attach_iohandle": (C.c_int, [_vp, _vp]),
    "coolmic_snddev_iter": (C.c_int, [_vp]),
    # include/coolmic-dsp/tee.h
    "coolmic_tee_new": (_vp, [C.c_char_p, _vp, C.c_size_t]),
    "coolmic_tee_attach_iohandle": (C.c_int, [_vp, _vp]),
    "coolmic_tee_get_iohandle": (_vp, [_vp, ssize_t]),
    # include/coolmic-dsp/util.h
    "coolmic_util_ahsv2argb": (C.c_uint32, [C.c_double, C.c_double, C.c_double, C.c_double]),
    "coolmic_util_power2hue": (C.c_double, [C.c_double, C.c_char_p]),
    "coolmic_util_peak2hue": (C.c_double, [C.c_int16, C.c_char_p]),
    "coolmic_util_vu_argb": (None, [_vp, C.c_size_t, C.c_char_p, _vp, _vp]),
    # include/coolmic-dsp/group.h
    "coolmic_group_new": (_vp, [C.c_char_p, _vp, C.c_uint32, C.c_uint, C.c_uint, C.c_size_t, C.c_uint]),
    "coolmic_group_new_on": (_vp, [C.c_int, C.c_char_p, _vp, C.c_uint32, C.c_uint, C.c_uint, C.c_size_t, C.c_uint]),
    "coolmic_group_device": (C.c_int, [_vp]),
    "coolmic_group_engine": (_vp, [_vp]),
    "coolmic_transform_set_device": (C.c_int, [_vp, C.c_int]),
    "coolmic_vumeter_set_device": (C.c_int, [_vp, C.c_int]),
    "cmhip_host_alloc_mapped_on": (_vp, [C.c_int, C.c_size_t, _P(_vp)]),
    "coolmic_group_add_stream": (C.c_int, [_vp, _vp]),
    "coolmic_group_set_master_gain": (C.c_int, [_vp, C.c_uint, C.c_uint, C.c_uint16, _P(C.c_uint16)]),
    "coolmic_group_set_channel_map": (C.c_int, [_vp, C.c_uint, _vp]),
    "coolmic_group_set_eq": (C.c_int, [_vp, C.c_int, C.c_uint, _vp]),
    "coolmic_group_get_iohandle": (_vp, [_vp, C.c_uint]),
    "coolmic_group_pump": (C.c_int, [_vp]),
    "coolmic_group_set_pull_threads": (C.c_int, [_vp, C.c_uint]),
    "coolmic_group_vumeter_result": (C.c_int, [_vp, C.c_uint, _P(VuResult)]),
    "coolmic_group_vumeter_results": (C.c_int, [_vp, _vp, _vp]),
    "coolmic_group_set_vu_finish": (C.c_int, [_vp, C.c_int]),
    "coolmic_group_set_true_peak": (C.c_int, [_vp, C.c_int]),
    "coolmic_group_true_peak": (C.c_int, [_vp, C.c_uint, _P(TruePeakResult)]),
    "coolmic_group_true_peaks": (C.c_int, [_vp, _vp, _vp]),
    "coolmic_group_set_loudness": (C.c_int, [_vp, C.c_int]),
    "coolmic_group_loudness": (C.c_int, [_vp, C.c_uint, _P(LoudnessResult)]),
    "coolmic_group_loudnesses": (C.c_int, [_vp, _vp, _vp]),
    "coolmic_group_loudness_set_weights": (C.c_int, [_vp, C.c_long, _vp]),
    "coolmic_group_loudness_reset": (C.c_int, [_vp, C.c_long]),
    "coolmic_group_set_watch": (C.c_int, [_vp, C.c_int]),
    "coolmic_group_watch_configure": (C.c_int, [_vp, C.c_uint, C.c_uint, C.c_uint]),
    "coolmic_group_watch": (C.c_int, [_vp, C.c_uint, _P(WatchResult)]),
    "coolmic_group_watches": (C.c_int, [_vp, _vp, _vp]),
    "coolmic_group_watch_reset": (C.c_int, [_vp, C.c_long]),
    "coolmic_group_set_correlation": (C.c_int, [_vp, C.c_int]),
    "coolmic_group_correlation_set_pairs": (C.c_int, [_vp, C.c_uint, _vp]),
    "coolmic_group_correlation": (C.c_int, [_vp, C.c_uint, _P(CorrResult)]),
    "coolmic_group_correlations": (C.c_int, [_vp, _vp, _vp]),
    "coolmic_group_correlation_reset": (C.c_int, [_vp, C.c_long]),
    "coolmic_group_set_spectrum": (C.c_int, [_vp, C.c_int]),
    "coolmic_group_spectrum_configure": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp, C.c_uint, _vp]),
    "coolmic_group_spectrum": (C.c_int, [_vp, C.c_uint, _P(SpecResult)]),
    "coolmic_group_spectra": (C.c_int, [_vp, _vp, _vp]),
    "coolmic_group_spectrum_reset": (C.c_int, [_vp, C.c_long]),
    "coolmic_group_streams": (C.c_uint, [_vp]),
}
MISSING = []        # entry points this build of the library lacks (an older build under tools/ab_two_libs.py)
for _name, (_res, _args) in SIGNATURES.items():
    if not hasattr(lib, _name):
        MISSING.append(_name)
        continue
    _fn = getattr(lib, _name)
    _fn.restype = _res
    if _args is not None:
        _fn.argtypes = _args

# not in a public header: host-logic test hooks
if hasattr(lib, "cmhip_test_gain_consts"):      # (an older build loaded by tools/ab_two_libs.py has another hook)
    lib.cmhip_test_gain_consts.restype = None
    lib.cmhip_test_gain_consts.argtypes = [C.c_uint16, C.c_uint16, _P(C.c_uint16), _P(C.c_uint32)]
if hasattr(lib, "cmhip_test_plan_run"):         # (not in builds older than the launcher's plan)
    lib.cmhip_test_plan_run.restype = None
    lib.cmhip_test_plan_run.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p]
if hasattr(lib, "cmhip_test_iohandle_root"):    # (not in builds older than the group's roots of shared sources)
    lib.cmhip_test_iohandle_root.restype = C.c_void_p
    lib.cmhip_test_iohandle_root.argtypes = [_vp]
    lib.cmhip_test_group_shared_source.restype = C.c_int
    lib.cmhip_test_group_shared_source.argtypes = [_vp, C.c_uint]
lib.cmhip_test_merge_windows.restype = C.c_int
lib.cmhip_test_merge_windows.argtypes = [_P(C.c_uint64), C.c_uint, C.c_uint, C.c_uint, _P(VuResult)]
if hasattr(lib, "cmhip_test_unpack_finished"):  # (not in builds older than the device-side dB finish)
    lib.cmhip_test_unpack_finished.restype = C.c_int
    lib.cmhip_test_unpack_finished.argtypes = [_vp, C.c_uint, C.c_uint, C.c_uint, _vp, _vp]
    lib.cmhip_test_power_db_device.restype = C.c_int
    lib.cmhip_test_power_db_device.argtypes = [_vp, _vp, C.c_uint, _vp, _vp]
if hasattr(lib, "cmhip_test_plan_tpeak"):       # (not in builds older than true peak)
    lib.cmhip_test_plan_tpeak.restype = None
    lib.cmhip_test_plan_tpeak.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.cmhip_debug_tp_count.restype = C.c_ulonglong
    lib.cmhip_debug_tp_count.argtypes = []
if hasattr(lib, "cmhip_test_plan_corr"):        # (not in builds older than phase correlation)
    lib.cmhip_test_plan_corr.restype = None
    lib.cmhip_test_plan_corr.argtypes = [C.c_uint32] * 4 + [C.c_void_p]
    lib.cmhip_debug_corr_count.restype = C.c_ulonglong
    lib.cmhip_debug_corr_count.argtypes = []
if hasattr(lib, "cmhip_test_plan_spec"):        # (not in builds older than the spectrum)
    lib.cmhip_test_plan_spec.restype = None
    lib.cmhip_test_plan_spec.argtypes = [C.c_uint32] * 7 + [C.c_void_p]
    lib.cmhip_test_spec_block.restype = C.c_int
    lib.cmhip_test_spec_block.argtypes = [C.c_uint, _vp, _vp]
    lib.cmhip_debug_spec_count.restype = C.c_ulonglong
    lib.cmhip_debug_spec_count.argtypes = []
if hasattr(lib, "cmhip_test_plan_watch"):       # (not in builds older than the signal watch)
    lib.cmhip_test_plan_watch.restype = None
    lib.cmhip_test_plan_watch.argtypes = [C.c_uint32] * 3 + [C.c_void_p]
    lib.cmhip_debug_watch_count.restype = C.c_ulonglong
    lib.cmhip_debug_watch_count.argtypes = []
    lib.cmhip_test_watch_time.restype = C.c_int
    lib.cmhip_test_watch_time.argtypes = [_vp, C.c_size_t, _vp]
if hasattr(lib, "cmhip_test_plan_loud"):        # (not in builds older than loudness)
    lib.cmhip_test_plan_loud.restype = None
    lib.cmhip_test_plan_loud.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.cmhip_debug_loud_count.restype = C.c_ulonglong
    lib.cmhip_debug_loud_count.argtypes = []
if hasattr(lib, "cmhip_test_plan_src"):         # (not in builds older than sample-rate conversion)
    lib.cmhip_test_plan_src.restype = None
    lib.cmhip_test_plan_src.argtypes = [C.c_uint32] * 6 + [C.c_void_p]
if hasattr(lib, "cmhip_test_plan_mix"):         # (not in builds older than channel mixing)
    lib.cmhip_test_plan_mix.restype = None
    lib.cmhip_test_plan_mix.argtypes = [C.c_uint32] * 4 + [C.c_void_p]
if hasattr(lib, "cmhip_test_plan_bus"):         # (not in builds older than the mix bus)
    lib.cmhip_test_plan_bus.restype = None
    lib.cmhip_test_plan_bus.argtypes = [C.c_uint32] * 4 + [C.c_void_p]
    lib.cmhip_test_bus_compile.restype = C.c_int
    lib.cmhip_test_bus_compile.argtypes = [C.c_uint] * 4 + [C.c_size_t] + [_vp] * 7
    lib.cmhip_test_bus_nt_loads.restype = None
    lib.cmhip_test_bus_nt_loads.argtypes = [_vp, C.c_int]
if hasattr(lib, "cmhip_test_plan_busramp"):     # (not in builds older than the send ramps)
    lib.cmhip_test_plan_busramp.restype = None
    lib.cmhip_test_plan_busramp.argtypes = [C.c_uint32] * 4 + [C.c_void_p]
if hasattr(lib, "cmhip_test_plan_lim"):         # (not in builds older than the peak limiter)
    lib.cmhip_test_plan_lim.restype = None
    lib.cmhip_test_plan_lim.argtypes = [C.c_uint32] * 5 + [C.c_void_p]
if hasattr(lib, "cmhip_test_plan_limtp"):       # (not in builds older than the limiter's true-peak detector)
    lib.cmhip_test_plan_limtp.restype = None
    lib.cmhip_test_plan_limtp.argtypes = [C.c_uint32] * 5 + [C.c_void_p]
if hasattr(lib, "cmhip_test_plan_limrel"):      # (not in builds older than the limiter's release stage)
    lib.cmhip_test_plan_limrel.restype = None
    lib.cmhip_test_plan_limrel.argtypes = [C.c_uint32] * 7 + [C.c_void_p]
if hasattr(lib, "cmhip_test_plan_dyn"):         # (not in builds older than the dynamics stage)
    lib.cmhip_test_plan_dyn.restype = None
    lib.cmhip_test_plan_dyn.argtypes = [C.c_uint32] * 6 + [C.c_void_p]
    lib.cmhip_test_dyn_curve_ok.restype = C.c_int
    lib.cmhip_test_dyn_curve_ok.argtypes = [_vp]
if hasattr(lib, "cmhip_test_plan_dynrms"):      # (not in builds older than the dynamics stage's RMS detector)
    lib.cmhip_test_plan_dynrms.restype = None
    lib.cmhip_test_plan_dynrms.argtypes = [C.c_uint32] * 6 + [C.c_void_p]
    lib.cmhip_test_dyn_isqrt.restype = C.c_uint32
    lib.cmhip_test_dyn_isqrt.argtypes = [C.c_uint32]
if hasattr(lib, "cmhip_test_plan_split"):       # (not in builds older than the band split)
    lib.cmhip_test_plan_split.restype = None
    lib.cmhip_test_plan_split.argtypes = [C.c_uint32] * 5 + [C.c_void_p]
    lib.cmhip_test_split_compile.restype = C.c_int
    lib.cmhip_test_split_compile.argtypes = [C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_size_t]
if hasattr(lib, "cmhip_test_plan_delay"):       # (not in builds older than the delay stage)
    lib.cmhip_test_plan_delay.restype = None
    lib.cmhip_test_plan_delay.argtypes = [C.c_uint32] * 5 + [C.c_void_p]
    lib.cmhip_test_delay_new_dry.restype = _vp
    lib.cmhip_test_delay_new_dry.argtypes = [_P(DelayDesc)]
    lib.cmhip_test_delay_tap.restype = None
    lib.cmhip_test_delay_tap.argtypes = [C.c_uint32] * 5 + [_P(C.c_uint32), _P(C.c_uint32)]
if hasattr(lib, "cmhip_test_plan_agc"):         # (not in builds older than the leveller)
    lib.cmhip_test_plan_agc.restype = None
    lib.cmhip_test_plan_agc.argtypes = [C.c_uint32] * 3 + [C.c_uint64, C.c_uint32, C.c_void_p]
    lib.cmhip_test_agc_run.restype = None
    lib.cmhip_test_agc_run.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.cmhip_test_agc_tile.restype = None
    lib.cmhip_test_agc_tile.argtypes = [C.c_uint32] * 6 + [C.c_void_p, C.c_void_p]
    lib.cmhip_test_agc_new_dry.restype = _vp
    lib.cmhip_test_agc_new_dry.argtypes = [_P(AgcDesc)]
    lib.cmhip_test_agc_step.restype = C.c_uint32
    lib.cmhip_test_agc_step.argtypes = [C.c_uint32, C.c_uint32, _P(AgcParams)]
    lib.cmhip_test_agc_run_events.restype = C.c_int
    lib.cmhip_test_agc_run_events.argtypes = [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _P(C.c_void_p)]
if hasattr(lib, "cmhip_test_denoise_new_dry"):  # (not in builds older than the noise suppressor)
    lib.cmhip_test_denoise_new_dry.restype = _vp
    lib.cmhip_test_denoise_new_dry.argtypes = [_P(DenoiseDesc)]
if hasattr(lib, "cmhip_test_plan_iir"):         # (not in builds older than the filter)
    lib.cmhip_test_plan_iir.restype = None
    lib.cmhip_test_plan_iir.argtypes = [C.c_uint32] * 4 + [C.c_void_p]
    lib.cmhip_test_iir_tile_vec.restype = None
    lib.cmhip_test_iir_tile_vec.argtypes = [C.c_uint32] * 4 + [_P(C.c_uint32), _P(C.c_uint32)]
    lib.cmhip_test_iir_section.restype = C.c_int32
    lib.cmhip_test_iir_section.argtypes = [_P(C.c_int32), C.c_int32, _P(C.c_int32), _P(C.c_uint32)]
    lib.cmhip_test_iir_output.restype = C.c_int32
    lib.cmhip_test_iir_output.argtypes = [C.c_int32, _P(C.c_uint32)]
    lib.cmhip_test_iir_new_dry.restype = _vp
    lib.cmhip_test_iir_new_dry.argtypes = [_P(IirDesc)]
    lib.cmhip_test_iir_rows.restype = C.c_int
    lib.cmhip_test_iir_rows.argtypes = [_vp, _vp]
if hasattr(lib, "cmhip_test_iir_ramp_at"):      # (not in builds older than the filter's ramps)
    lib.cmhip_test_iir_ramp_at.restype = None
    lib.cmhip_test_iir_ramp_at.argtypes = [_P(C.c_int32), _P(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32,
                                           _P(C.c_int32), _P(C.c_uint32)]
lib.cmhip_debug_run_count.restype = C.c_ulonglong
lib.cmhip_debug_run_count.argtypes = []
lib.coolmic_debug_vumeter_mode.restype = C.c_int
lib.coolmic_debug_vumeter_mode.argtypes = [_vp]
lib.coolmic_sine_period.restype = C.c_int
lib.coolmic_sine_period.argtypes = [C.c_uint32, _vp, _P(C.c_size_t)]


class CoolmicError(RuntimeError):
    def __init__(self, what, code):
        text = lib.coolmic_error2string(code).decode()
        detail = lib.cmhip_last_error().decode()
        super().__init__(f"{what}: {code} ({text}) {detail}")
        self.code = code


def _check(what, rc):
    if rc != ERROR_NONE:
        raise CoolmicError(what, rc)


def device_count():
    return lib.cmhip_device_count()


def device_synchronize(device=0):
    _check("device_synchronize", lib.cmhip_device_synchronize(device))


def device_mem_info(device=0):
    f, t = C.c_size_t(), C.c_size_t()
    _check("device_mem_info", lib.cmhip_device_mem_info(device, C.byref(f), C.byref(t)))
    return f.value, t.value


def last_error():
    return lib.cmhip_last_error().decode()


def gain_consts(gain, scale):
    """Test hook: the division constants the kernels use for gain / scale -- integer part mi and fraction mf with
    floor(|x| * gain / scale) == |x| * mi + ((|x| * mf) >> 32) for every |x| <= 32768 (StreamParam, cmhip_internal.h)."""
    mi, mf = C.c_uint16(), C.c_uint32()
    lib.cmhip_test_gain_consts(gain, scale, C.byref(mi), C.byref(mf))
    return mi.value, mf.value


class RunPlan(C.Structure):
    """cmhip::RunPlan (csrc/cmhip_internal.h): what the block-kernel launcher launches for a run"""
    _fields_ = [(name, C.c_int if name == "err" else C.c_uint32)
                for name in ("err", "family", "channels", "tile_u", "waves", "map", "stage", "grid", "block",
                             "chunks", "W", "rows_per_tile", "keep_flag")]


class TpPlan(C.Structure):
    """cmhip::TpPlan (csrc/cmhip_internal.h): what the true-peak launcher launches for a run"""
    _fields_ = [("err", C.c_int), ("fast", C.c_uint32), ("grid", C.c_uint32), ("block", C.c_uint32),
                ("chunks", C.c_uint32)]


def plan_tpeak(streams, channels, frames):
    """Test hook: the true-peak launcher's plan for a run (host logic, needs no GPU)"""
    p = TpPlan()
    lib.cmhip_test_plan_tpeak(streams, channels, frames, C.addressof(p))
    return p


def tp_dbtp(peak):
    """the host finish of a true-peak value: 20 * log10(peak / 2^28), -inf for 0"""
    return lib.cmhip_tp_dbtp(peak)


def tp_coefficients():
    """the 4 x 12 int16 coefficients of the true-peak filter, in units of 2^-13"""
    h = np.zeros(48, dtype=np.int16)
    lib.cmhip_tp_coefficients(h.ctypes.data)
    return h.reshape(4, 12)


def _spec_geometry(edges, channels):
    """(nb, edges array or None, nch, channels array or None) as cmhip_batch_spec_configure takes them"""
    e = (C.c_uint16 * len(edges))(*[int(v) for v in edges]) if edges is not None else None
    c = (C.c_ubyte * len(channels))(*[int(v) for v in channels]) if channels is not None else None
    return (len(edges) - 1 if edges is not None else 0, e, len(channels) if channels is not None else 0, c)


class CorrPlan(C.Structure):
    """cmhip::CorrPlan (csrc/cmhip_internal.h): what the correlation launcher launches for a run"""
    _fields_ = [("err", C.c_int), ("fast", C.c_uint32), ("grid", C.c_uint32), ("block", C.c_uint32),
                ("chunks", C.c_uint32)]


def plan_corr(streams, channels, frames, npairs=1):
    """Test hook: the correlation launcher's plan for a run (host logic, needs no GPU)"""
    p = CorrPlan()
    lib.cmhip_test_plan_corr(streams, channels, frames, npairs, C.addressof(p))
    return p


class WatchPlan(C.Structure):
    """cmhip::WatchPlan (csrc/watch_plan.h): what the watch's launcher launches for a run"""
    _fields_ = [("refused", C.c_int32), ("fast", C.c_uint32), ("tile_frames", C.c_uint32), ("chunks", C.c_uint32),
                ("grid", C.c_uint32), ("block", C.c_uint32), ("fold_grid", C.c_uint32), ("fold_block", C.c_uint32),
                ("scratch", C.c_uint64)]


def plan_watch(streams, channels, frames):
    """Test hook: the watch launcher's plan for a run (host logic, needs no GPU)"""
    p = WatchPlan()
    lib.cmhip_test_plan_watch(streams, channels, frames, C.addressof(p))
    return p


def watch_time(batch, frames):
    """Measurement hook (tools/bench_watch.py): the watch's two kernels alone over the batch's own input slots, timed
    between events -> (tile pass ms, fold ms).  The frames are accounted as a run's are: reset afterwards."""
    ms = (C.c_float * 2)()
    _check("watch_time", lib.cmhip_test_watch_time(batch.h, frames, ms))
    return ms[0], ms[1]


def watch_level(db):
    """a threshold for watch_configure from a level in dBFS: lround(32768 * 10^(db / 20)) clamped to 0..32767"""
    return lib.cmhip_watch_level(db)


def corr_value(energy_a, energy_b, cross):
    """the host finish of a correlation window: cross / sqrt(energy_a * energy_b) in [-1, 1], 0.0 for a silent leg"""
    return lib.cmhip_corr_value(energy_a, energy_b, cross)


def corr_balance_db(energy_a, energy_b):
    """the host finish of a window's balance: 10 * log10(energy_a / energy_b), 0.0 when both are 0"""
    return lib.cmhip_corr_balance_db(energy_a, energy_b)


def _corr_pairs(pairs):
    flat = [int(c) for p in pairs for c in p]
    if len(flat) != 2 * len(pairs):
        raise ValueError("corr_set_pairs: every pair is two channels")
    return (C.c_ubyte * max(len(flat), 2))(*flat)


class SpecPlan(C.Structure):
    """cmhip::SpecPlan (csrc/cmhip_internal.h): what the spectrum launcher launches for a run"""
    _fields_ = [("err", C.c_int), ("grid", C.c_uint32), ("block", C.c_uint32), ("chunks", C.c_uint32)]


def plan_spec(streams, channels, frames, fft_log2=10, nch=1, nb=10, max_blocks=0):
    """Test hook: the spectrum launcher's plan for a run whose streams complete at most max_blocks blocks (host logic,
    needs no GPU)"""
    p = SpecPlan()
    lib.cmhip_test_plan_spec(streams, channels, frames, fft_log2, nch, nb, max_blocks, C.addressof(p))
    return p


def spec_window(fft_log2):
    """the spectrum's Hann window, int16 [N]"""
    w = np.zeros(1 << fft_log2, dtype=np.int16)
    _check("spec_window", lib.cmhip_spec_window(fft_log2, w.ctypes.data))
    return w


def spec_twiddles(fft_log2):
    """the spectrum's twiddles in units of 2^-30 -> (wr, wi), int32 [N / 2] each"""
    wr = np.zeros(1 << (fft_log2 - 1), dtype=np.int32)
    wi = np.zeros_like(wr)
    _check("spec_twiddles", lib.cmhip_spec_twiddles(fft_log2, wr.ctypes.data, wi.ctypes.data))
    return wr, wi


def spec_design_bands(rate, fft_log2, per_octave):
    """fractional-octave bands around 1 kHz -> the list of nb + 1 bin edges, or the negative error number"""
    e = np.zeros(SPEC_MAX_BANDS + 1, dtype=np.uint16)
    nb = lib.cmhip_spec_design_bands(rate, fft_log2, per_octave, e.ctypes.data)
    return nb if nb < 0 else [int(v) for v in e[:nb + 1]]


def spec_db(power, blocks):
    """the host finish of a band: 10 * log10(power / (blocks * 1.5 * 2^40)), -inf for power 0, 0.0 for blocks 0"""
    return lib.cmhip_spec_db(power, blocks)


def spec_block(fft_log2, x):
    """Test hook: the library's plain reference of one block, int16 x[N] -> uint64 p[N / 2 + 1] (needs no GPU)"""
    x = np.ascontiguousarray(x, dtype=np.int16)
    if x.shape != (1 << fft_log2,):
        raise ValueError("spec_block: x holds N samples")
    p = np.zeros((1 << (fft_log2 - 1)) + 1, dtype=np.uint64)
    _check("spec_block", lib.cmhip_test_spec_block(fft_log2, x.ctypes.data, p.ctypes.data))
    return p


class LoudPlan(C.Structure):
    """cmhip::LoudPlan (csrc/cmhip_internal.h): what the loudness launcher launches for a run"""
    _fields_ = [("err", C.c_int), ("vec", C.c_uint32), ("grid", C.c_uint32), ("block", C.c_uint32)]


def plan_loud(streams, channels, frames):
    """Test hook: the loudness launcher's plan for a run (host logic, needs no GPU)"""
    p = LoudPlan()
    lib.cmhip_test_plan_loud(streams, channels, frames, C.addressof(p))
    return p


def loud_coefficients(rate):
    """the K-weighting biquads for a rate: {b0, b1, b2, a1, a2} of section 1, then of section 2"""
    c = (C.c_double * 10)()
    lib.cmhip_loud_coefficients(rate, c)
    return list(c)


def loud_lufs(mean_square):
    """-0.691 + 10 * log10(mean_square), -inf for 0"""
    return lib.cmhip_loud_lufs(mean_square)


def loud_integrate(z):
    """gated integrated loudness of sub-block mean squares z -> (integrated, relative threshold, gated blocks)"""
    arr = (C.c_double * len(z))(*z)
    i, t, g = C.c_double(), C.c_double(), C.c_size_t()
    _check("loud_integrate", lib.cmhip_loud_integrate(arr, len(z), C.byref(i), C.byref(t), C.byref(g)))
    return i.value, t.value, g.value


class SrcPlan(C.Structure):
    """cmhip::SrcPlan (csrc/cmhip_internal.h): what the resampler's launcher launches for a run"""
    _fields_ = [("err", C.c_int)] + [(n, C.c_uint32) for n in ("fast", "grid", "block", "chunks", "tile_out", "tile_in",
                                                               "row", "table_lds", "lds_bytes")]


def plan_src(streams, channels, L, M, T, out_frames):
    """Test hook: the resampler launcher's plan for a run that gives its longest stream out_frames frames (host
    logic, needs no GPU)"""
    p = SrcPlan()
    lib.cmhip_test_plan_src(streams, channels, L, M, T, out_frames, C.addressof(p))
    return p


def src_design(rate_in, rate_out):
    """the designed resampling table for a pair of rates -> (L, M, T, int16 array [L][T]); CoolmicError when the pair
    has none"""
    L, M, T = C.c_uint(), C.c_uint(), C.c_uint()
    _check("src_design", lib.cmhip_src_design(rate_in, rate_out, C.byref(L), C.byref(M), C.byref(T), None, 0))
    h = np.zeros(L.value * T.value, dtype=np.int16)
    _check("src_design", lib.cmhip_src_design(rate_in, rate_out, None, None, None, h.ctypes.data, h.size))
    return L.value, M.value, T.value, h.reshape(L.value, T.value)


def src_out_frames(L, M, r, frames):
    """output frames of a run of `frames` input frames for a stream at position r = (frames so far) mod M"""
    return lib.cmhip_src_out_frames(L, M, r, frames)


if hasattr(lib, "cmhip_test_drift_new_dry"):    # (not in builds older than the drift stage)
    lib.cmhip_test_drift_new_dry.restype = _vp
    lib.cmhip_test_drift_new_dry.argtypes = [_P(DriftDesc), C.c_uint, C.c_uint, _vp]
    lib.cmhip_test_drift_advance.restype = C.c_int
    lib.cmhip_test_drift_advance.argtypes = [_vp, C.c_size_t, _vp, _vp]
    lib.cmhip_test_plan_drift.restype = None
    lib.cmhip_test_plan_drift.argtypes = [C.c_uint32] * 5 + [C.c_void_p]

DRIFT_DELTA_MAX = 1 << 24


class DriftPlan(C.Structure):
    """cmhip::DriftPlan (csrc/drift_plan.h): what the drift stage's launcher launches for a run"""
    _fields_ = [("err", C.c_int)] + [(n, C.c_uint32) for n in ("fast", "grid", "block", "chunks", "tile_out", "tile_in",
                                                               "row", "table_lds", "table_words", "lds_bytes")]


def plan_drift(streams, channels, phase_log2, taps, out_frames):
    """Test hook: the drift launcher's plan for a run that gives its longest stream out_frames frames (host logic,
    needs no GPU)"""
    p = DriftPlan()
    lib.cmhip_test_plan_drift(streams, channels, phase_log2, taps, out_frames, C.addressof(p))
    return p


def drift_design_rc(phase_log2, taps, cap=None):
    """cmhip_drift_design as it is -> (error number, int16 array of `cap` entries, default the table's)"""
    h = np.zeros(max(1, (taps << phase_log2) if cap is None else cap), dtype=np.int16)
    return lib.cmhip_drift_design(phase_log2, taps, h.ctypes.data, h.size if cap is None else cap), h


def drift_design(phase_log2=7, taps=32):
    """the designed drift table -> int16 array [2^phase_log2][taps]"""
    rc, h = drift_design_rc(phase_log2, taps)
    _check("drift_design", rc)
    return h.reshape(1 << phase_log2, taps)


def drift_out_frames(pos, delta, frames):
    """output frames of a run of `frames` input frames for a stream at position pos with step 2^32 + delta"""
    return lib.cmhip_drift_out_frames(pos, delta, frames)


def drift_ppm(ppm):
    """cmhip_drift_ppm: parts per million -> delta"""
    return lib.cmhip_drift_ppm(ppm)


def drift_to_ppm(delta):
    """cmhip_drift_to_ppm: delta -> parts per million"""
    return lib.cmhip_drift_to_ppm(delta)


class Servo:
    """cmhip_drift_servo_t: the PI controller that turns an elastic buffer's fill into the next delta"""

    def __init__(self, target_frames, kp_log2, ki_log2, limit=DRIFT_DELTA_MAX):
        self.s = DriftServo()
        _check("drift_servo_init", lib.cmhip_drift_servo_init(C.byref(self.s), target_frames, kp_log2, ki_log2, limit))

    def step(self, fill_frames):
        return lib.cmhip_drift_servo_step(C.byref(self.s), fill_frames)

    def reset(self):
        lib.cmhip_drift_servo_reset(C.byref(self.s))


def test_drift_without_device(streams, channels, max_in_frames, table=None):
    """Test hook (cmhip_test_drift_new_dry): a Drift with the host mirror and every check but no device behind it"""
    return Drift(streams, channels, max_in_frames, table=table, _dry=True)


class SplitPlan(C.Structure):
    """cmhip::SplitPlan (csrc/split_plan.h): what the band split's launcher launches for a run"""
    _fields_ = [(name, C.c_int if name == "err" else C.c_uint32)
                for name in ("err", "fast", "grid", "block", "chunks", "tile_frames", "tp", "row", "table_words",
                             "lds_bytes")]


def plan_split(streams, channels, bands, taps, frames):
    """Test hook: the launch plan of a band-split run whose longest stream has `frames` frames (host logic, needs no
    GPU)."""
    p = SplitPlan()
    lib.cmhip_test_plan_split(streams, channels, bands, taps, frames, C.addressof(p))
    return p


class DelayPlan(C.Structure):
    """cmhip::DelayPlan (csrc/delay_plan.h): what the delay's launcher launches for a run"""
    _fields_ = [(name, C.c_int if name == "err" else C.c_uint32)
                for name in ("err", "fast", "grid", "block", "chunks", "tile_frames", "tile_vecs", "ring_frames")]


DELAY_BEHIND, DELAY_FRONT, DELAY_MIXED = 0, 1, 2     # cmhip::DelayClass


def plan_delay(streams, channels, max_delay, max_frames, frames):
    """Test hook: the launch plan of a delay run whose longest stream has `frames` frames, and the ring's frames (host
    logic, needs no GPU)."""
    p = DelayPlan()
    lib.cmhip_test_plan_delay(streams, channels, max_delay, max_frames, frames, C.addressof(p))
    return p


def delay_tap(e0, length, D, P, CAP):
    """Test hook: cmhip::delay_tap (csrc/delay_plan.h), everything in samples -> (class, first source sample)"""
    cls, q = C.c_uint32(0), C.c_uint32(0)
    lib.cmhip_test_delay_tap(e0, length, D, P, CAP, C.byref(cls), C.byref(q))
    return cls.value, q.value


def test_delay_without_device(streams, channels, max_delay, max_frames):
    """Test hook (cmhip_test_delay_new_dry): a Delay with the host mirror and every check but no device behind it, for
    the refusals on a machine without a GPU; a run that would launch is refused."""
    return Delay(streams, channels, max_delay, max_frames, _new=lib.cmhip_test_delay_new_dry)


if hasattr(lib, "cmhip_test_automix_new_dry"):  # (not in builds older than the automixer)
    lib.cmhip_test_automix_new_dry.restype = _vp
    lib.cmhip_test_automix_new_dry.argtypes = [_P(AutomixDesc)]
    lib.cmhip_test_automix_power.restype = C.c_uint64
    lib.cmhip_test_automix_power.argtypes = [C.c_uint64, C.c_uint32, _P(AutomixParams)]
    lib.cmhip_test_automix_share.restype = C.c_uint32
    lib.cmhip_test_automix_share.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    lib.cmhip_test_automix_run_events.restype = C.c_int
    lib.cmhip_test_automix_run_events.argtypes = [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _P(C.c_void_p)]


class AgcPlan(C.Structure):
    """cmhip::AgcPlan (csrc/agc_plan.h): what the leveller's launcher launches for a run"""
    _fields_ = [("err", C.c_int)] + [(n, C.c_uint32) for n in ("fast", "grid", "block", "chunks", "tile_log2", "nw",
                                                                "step_grid")]


class AgcRun(C.Structure):
    """cmhip::AgcRun (csrc/agc_plan.h): the windows a stream's run touches"""
    _fields_ = [("first", C.c_uint64)] + [(n, C.c_uint32) for n in ("nwin", "complete", "head", "tail")]


class AgcTile(C.Structure):
    """cmhip::AgcTile (csrc/agc_plan.h)"""
    _fields_ = [(n, C.c_uint32) for n in ("fa", "fb", "win", "j")]


class AgcSpan(C.Structure):
    """cmhip::AgcSpan (csrc/agc_plan.h)"""
    _fields_ = [(n, C.c_uint32) for n in ("sa", "hend", "vb", "ve", "tb", "sb")]


def plan_agc(streams, channels, window_log2, max_frames, frames):
    """Test hook: the launch plan of a leveller run whose longest stream has `frames` frames (host logic, no GPU)"""
    p = AgcPlan()
    lib.cmhip_test_plan_agc(streams, channels, window_log2, max_frames, frames, C.addressof(p))
    return p


def agc_run(pos, count, window_log2):
    """Test hook: cmhip::agc_run (csrc/agc_plan.h), the windows of a run of `count` frames from position `pos`"""
    r = AgcRun()
    lib.cmhip_test_agc_run(pos, count, window_log2, C.addressof(r))
    return r


def agc_tile(pos_lo, count, window_log2, tile_log2, t, channels):
    """Test hook: cmhip::agc_tile and agc_tile_span (csrc/agc_plan.h) -> (AgcTile, AgcSpan)"""
    tl, sp = AgcTile(), AgcSpan()
    lib.cmhip_test_agc_tile(pos_lo, count, window_log2, tile_log2, t, channels, C.addressof(tl), C.addressof(sp))
    return tl, sp


def agc_params(**kw):
    """an AgcParams: the creation defaults (a copy) with `kw` over them"""
    f = dict(target=3277, gate=33, gain_min=4096, gain_max=4096, rise=0, fall=0, initial=4096)
    f.update(kw)
    return AgcParams(**f)


def agc_step(A, L, params):
    """Test hook (cmhip_test_agc_step): the header's step(A, L) as code"""
    return lib.cmhip_test_agc_step(A, L, C.byref(params))


def agc_check(window_log2, params=None):
    """cmhip_agc_check -> error number"""
    return lib.cmhip_agc_check(window_log2, C.byref(params) if params is not None else None)


def agc_design(rate, window_log2, target_db, gate_db, max_gain_db, min_gain_db, initial_gain_db, rise_db_per_s,
               fall_db_per_s):
    """cmhip_agc_design -> AgcParams"""
    law = AgcLawDesc(rate, window_log2, target_db, gate_db, max_gain_db, min_gain_db, initial_gain_db, rise_db_per_s,
                     fall_db_per_s)
    p = AgcParams()
    _check("agc_design", lib.cmhip_agc_design(C.byref(law), C.byref(p)))
    return p


if hasattr(lib, "cmhip_test_failover_new_dry"):  # (not in builds older than the failover switch)
    lib.cmhip_test_failover_new_dry.restype = _vp
    lib.cmhip_test_failover_new_dry.argtypes = [_P(FailoverDesc)]
    lib.cmhip_test_failover_edge.restype = C.c_uint32
    lib.cmhip_test_failover_edge.argtypes = [C.c_uint32, C.c_uint, _P(FailoverParams), C.c_uint, _vp, _vp, _vp,
                                             _P(C.c_uint32)]
    lib.cmhip_test_failover_first.restype = C.c_uint32
    lib.cmhip_test_failover_first.argtypes = [_P(FailoverParams)]
    lib.cmhip_test_failover_fade.restype = C.c_int32
    lib.cmhip_test_failover_fade.argtypes = [C.c_int16, C.c_int16, C.c_uint32, C.c_uint32]
    lib.cmhip_test_failover_run_events.restype = C.c_int
    lib.cmhip_test_failover_run_events.argtypes = [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, _P(C.c_void_p)]


def failover_params(window_log2, **kw):
    """a FailoverParams: the creation defaults of an object with this window_log2, with `kw` over them"""
    f = dict(quiet=(33, 33, 33, 33), fail_windows=1, return_windows=1, fade_log2=window_log2, force=-1)
    f.update(kw)
    q = f.pop("quiet")
    q = (q,) * 4 if np.isscalar(q) else tuple(q)
    return FailoverParams((C.c_uint16 * 4)(*q), **f)


def failover_check(window_log2, n_sources, params=None):
    """cmhip_failover_check -> error number"""
    return lib.cmhip_failover_check(window_log2, n_sources, C.byref(params) if params is not None else None)


def failover_design(rate, window_log2, quiet_db=-60.0, fail_s=0.0, return_s=0.0, fade_ms=0.0):
    """cmhip_failover_design -> FailoverParams (quiet_db: one value for every candidate, or four)"""
    q = (quiet_db,) * 4 if np.isscalar(quiet_db) else tuple(quiet_db)
    law = FailoverLawDesc(rate, window_log2, (C.c_double * 4)(*q), fail_s, return_s, fade_ms)
    p = FailoverParams()
    _check("failover_design", lib.cmhip_failover_design(C.byref(law), C.byref(p)))
    return p


def failover_step(n_sources, params, cur, live_run, dead_run):
    """cmhip_failover_step: the candidate wanted at a window edge outside a fade, the specification as code"""
    lv = np.ascontiguousarray(live_run, dtype=np.uint32)
    dd = np.ascontiguousarray(dead_run, dtype=np.uint32)
    assert lv.size == 4 and dd.size == 4
    return lib.cmhip_failover_step(n_sources, C.byref(params), cur, lv.ctypes.data, dd.ctypes.data)


def failover_edge(plan, n_sources, params, window_log2, level, live_run, dead_run):
    """Test hook (cmhip_test_failover_edge): one window edge as k_failover_step takes it: the counters take `level`,
    then the plan word moves on -> (plan word, live_run [4], dead_run [4], switched)"""
    lv = np.array(live_run, dtype=np.uint32)
    dd = np.array(dead_run, dtype=np.uint32)
    m = np.ascontiguousarray(level, dtype=np.uint32)
    assert lv.size == 4 and dd.size == 4 and m.size == 4
    sw = C.c_uint32(0)
    pl = lib.cmhip_test_failover_edge(plan, n_sources, C.byref(params), window_log2, m.ctypes.data, lv.ctypes.data,
                                      dd.ctypes.data, C.byref(sw))
    return pl, [int(v) for v in lv], [int(v) for v in dd], sw.value


def failover_first(params):
    """Test hook (cmhip_test_failover_first): the plan word of window 0"""
    return lib.cmhip_test_failover_first(C.byref(params))


def failover_fade(a, b, d, phi):
    """Test hook (cmhip_test_failover_fade): frame d of a fade over 2^phi frames from sample a to sample b"""
    return lib.cmhip_test_failover_fade(a, b, d, phi)


def test_failover_without_device(streams, outputs, channels, window_log2, max_frames):
    """Test hook (cmhip_test_failover_new_dry): a Failover with the host mirror and every check but no device behind
    it"""
    return Failover(streams, outputs, channels, window_log2, max_frames, _new=lib.cmhip_test_failover_new_dry)


def automix_params(**kw):
    """an AutomixParams: the creation defaults with `kw` over them"""
    f = dict(weight=4096, floor=0, attack=0, release=0, initial=4096)
    f.update(kw)
    return AutomixParams(**f)


def automix_power(P, m, params):
    """Test hook (cmhip_test_automix_power): the header's P[k] from P[k-1] and the window's m, as code"""
    return lib.cmhip_test_automix_power(P, m, C.byref(params))


def automix_share(P, total, floor, D_before):
    """Test hook (cmhip_test_automix_share): the header's D[k] from P[k], the group's sum, the floor and D[k-1]"""
    return lib.cmhip_test_automix_share(P, total, floor, D_before)


def automix_check(window_log2, params=None):
    """cmhip_automix_check -> error number"""
    return lib.cmhip_automix_check(window_log2, C.byref(params) if params is not None else None)


def automix_design(rate, window_log2, weight_db=0.0, floor_db=-100.0, initial_db=0.0, attack_ms=0.0, release_ms=0.0):
    """cmhip_automix_design -> AutomixParams"""
    law = AutomixLawDesc(rate, window_log2, weight_db, floor_db, initial_db, attack_ms, release_ms)
    p = AutomixParams()
    _check("automix_design", lib.cmhip_automix_design(C.byref(law), C.byref(p)))
    return p


def test_automix_without_device(streams, channels, window_log2, max_frames):
    """Test hook (cmhip_test_automix_new_dry): an Automixer with the host mirror and every check but no device behind
    it, for the refusals and the mirror's answers on a machine without a GPU"""
    return Automixer(streams, channels, window_log2, max_frames, _new=lib.cmhip_test_automix_new_dry)


def test_agc_without_device(streams, channels, window_log2, max_frames):
    """Test hook (cmhip_test_agc_new_dry): a Leveller with the host mirror and every check but no device behind it, for
    the refusals on a machine without a GPU"""
    return Leveller(streams, channels, window_log2, max_frames, _new=lib.cmhip_test_agc_new_dry)


class IirPlan(C.Structure):
    """cmhip::IirPlan (csrc/iir_plan.h): what the filter's launcher launches for a run"""
    _fields_ = [("err", C.c_int)] + [(n, C.c_uint32) for n in ("fast", "np", "spw", "grid", "block", "tile", "tiles",
                                                                "lds_bytes")]


def plan_iir(streams, channels, sections, frames):
    """Test hook: the launch plan of a filter run whose longest stream has `frames` frames (host logic, no GPU)"""
    p = IirPlan()
    lib.cmhip_test_plan_iir(streams, channels, sections, frames, C.addressof(p))
    return p


def iir_tile_vec(count, channels, t, q):
    """Test hook: cmhip::iir_tile_vec (csrc/iir_plan.h) -> (first sample in the slot, samples below the count)"""
    off, n = C.c_uint32(), C.c_uint32()
    lib.cmhip_test_iir_tile_vec(count, channels, t, q, C.byref(off), C.byref(n))
    return off.value, n.value


def iir_section_step(sec, u, state):
    """Test hook: cmhip::iir_section (csrc/iir_plan.h): one frame through one section.  sec: five ints, state: a list
    [u1, u2, v1, v2, e] updated in place -> (v, over)"""
    cs, st, over = (C.c_int32 * 5)(*sec), (C.c_int32 * 5)(*state), C.c_uint32()
    v = lib.cmhip_test_iir_section(cs, u, st, C.byref(over))
    state[:] = list(st)
    return v, over.value


def iir_output(v):
    """Test hook: cmhip::iir_output (csrc/iir_plan.h) -> (y, clip)"""
    clip = C.c_uint32()
    y = lib.cmhip_test_iir_output(v, C.byref(clip))
    return y, clip.value


def iir_section(b0=IIR_ONE, b1=0, b2=0, a1=0, a2=0):
    """an IirSection: unity with the arguments over it"""
    return IirSection(b0, b1, b2, a1, a2)


def iir_check(section):
    """cmhip_iir_check -> error number"""
    return lib.cmhip_iir_check(C.byref(section))


def iir_design(kind, rate, f0, q=0.7071067811865476, gain_db=0.0):
    """cmhip_iir_design -> IirSection"""
    d = IirDesignDesc(kind, rate, f0, q, gain_db)
    s = IirSection()
    _check("iir_design", lib.cmhip_iir_design(C.byref(d), C.byref(s)))
    return s


def iir_response_db(sections, rate, f):
    """cmhip_iir_response_db: the magnitude in dB at f of the cascade of the sections' integers"""
    arr = (IirSection * len(sections))(*sections)
    return lib.cmhip_iir_response_db(arr, len(sections), rate, f)


IIR_RAMP_MAX = 1 << 20


def iir_ramp_section(c0, c1, p):
    """cmhip_iir_ramp_section: the section at position p (0..32768) between two IirSections -> IirSection"""
    out = IirSection()
    lib.cmhip_iir_ramp_section(C.byref(c0), C.byref(c1), p, C.byref(out))
    return out


def iir_ramp_at(c0, c1, done, R, f):
    """Test hook: the section and the position that the ramp kernels compute for frame f of a run that a section with
    the ends c0, c1 (five ints each), `done` and R enters -> (five ints, p)"""
    a, b, out, p = (C.c_int32 * 5)(*c0), (C.c_int32 * 5)(*c1), (C.c_int32 * 5)(), C.c_uint32()
    lib.cmhip_test_iir_ramp_at(a, b, done, R, f, out, C.byref(p))
    return tuple(out), p.value


def test_iir_without_device(streams, channels, sections, max_frames):
    """Test hook (cmhip_test_iir_new_dry): a Filter with the host mirror and every check but no device behind it, for
    the refusals on a machine without a GPU"""
    return Filter(streams, channels, sections, max_frames, _new=lib.cmhip_test_iir_new_dry)


def test_denoise_without_device(streams, channels, fft_log2, max_frames):
    """Test hook (cmhip_test_denoise_new_dry): a Denoiser with the host mirror and every check but no device behind it,
    for the refusals and the mirror's answers on a machine without a GPU"""
    return Denoiser(streams, channels, fft_log2, max_frames, _new=lib.cmhip_test_denoise_new_dry)


def denoise_params(**kw):
    """a DenoiseParams: the creation defaults (a pure delay) with `kw` over them"""
    f = dict(floor=32768, over=16, rise_shift=0, fall_shift=0)
    f.update(kw)
    return DenoiseParams(**f)


def denoise_check(fft_log2, params=None):
    """cmhip_denoise_check -> error number"""
    return lib.cmhip_denoise_check(fft_log2, C.byref(params) if params is not None else None)


def denoise_window(fft_log2):
    """cmhip_denoise_window -> int16 [N]"""
    w = np.zeros(1 << fft_log2, dtype=np.int16)
    _check("denoise_window", lib.cmhip_denoise_window(fft_log2, w.ctypes.data))
    return w


def denoise_design(rate, fft_log2, reduction_db, over_db, attack_ms, release_ms):
    """cmhip_denoise_design -> DenoiseParams"""
    law = DenoiseLawDesc(rate, fft_log2, reduction_db, over_db, attack_ms, release_ms)
    p = DenoiseParams()
    _check("denoise_design", lib.cmhip_denoise_design(C.byref(law), C.byref(p)))
    return p


def denoise_gain(p, np_, over, floor):
    """cmhip_denoise_gain: the target rule of a bin, the specification as code"""
    return lib.cmhip_denoise_gain(p, np_, over, floor)


def delay_ms(rate, ms):
    """cmhip_delay_ms: rint(rate * ms / 1000) frames"""
    return lib.cmhip_delay_ms(rate, ms)


def delay_crossfade(a, b, p):
    """cmhip_delay_crossfade: the crossfade of two samples at position p, the specification as code"""
    return lib.cmhip_delay_crossfade(a, b, p)


def _crossovers(crossover_hz, bands):
    f = [float(v) for v in crossover_hz]
    assert len(f) == bands - 1
    return (C.c_double * len(f))(*f)


def split_design(rate, bands, crossover_hz, taps):
    """cmhip_split_design -> (int16 [B-1][T] filters, uint8 [B-1] scales)"""
    g = np.zeros((bands - 1, taps), dtype=np.int16)
    q = np.zeros(bands - 1, dtype=np.uint8)
    _check("split_design", lib.cmhip_split_design(rate, bands, _crossovers(crossover_hz, bands), taps, g.ctypes.data,
                                                  q.ctypes.data, g.size))
    return g, q


def split_check(bands, taps, g, q):
    """cmhip_split_check as it is -> error number"""
    g = None if g is None else np.ascontiguousarray(g, dtype=np.int16)
    q = None if q is None else np.ascontiguousarray(q, dtype=np.uint8)
    return lib.cmhip_split_check(bands, taps, None if g is None else g.ctypes.data, None if q is None else q.ctypes.data)


def split_compile(g, q):
    """Test hook: the filters in the kernel's form (csrc/split_plan.h) -> (pairs uint32 [B-1][Tp/2], masks uint32
    [B-1][Tp/8], q uint32 [B-1])"""
    g = np.ascontiguousarray(g, dtype=np.int16)
    q = np.ascontiguousarray(q, dtype=np.uint8)
    nf, T = g.shape
    tp = (T + 8) & ~7
    out = np.zeros(nf * (tp // 2 + tp // 8 + 1), dtype=np.uint32)
    n = lib.cmhip_test_split_compile(nf + 1, T, g.ctypes.data, q.ctypes.data, out.ctypes.data, out.size)
    assert n == out.size, n
    a, b = nf * (tp // 2), nf * (tp // 2 + tp // 8)
    return out[:a].reshape(nf, tp // 2), out[a:b].reshape(nf, tp // 8), out[b:]


class MixPlan(C.Structure):
    """cmhip::MixPlan (csrc/cmhip_internal.h): what the mixer's launcher launches for a run"""
    _fields_ = [("err", C.c_int)] + [(n, C.c_uint32) for n in ("fast", "grid", "block", "chunks", "tile_frames",
                                                               "lds_bytes")]


def plan_mix(streams, channels_in, channels_out, frames):
    """Test hook: the mixer launcher's plan for a run whose longest stream has `frames` frames (host logic, needs no
    GPU)"""
    p = MixPlan()
    lib.cmhip_test_plan_mix(streams, channels_in, channels_out, frames, C.addressof(p))
    return p


MIX_MONO_TO_STEREO, MIX_STEREO_TO_MONO, MIX_STEREO_TO_MS, MIX_51_TO_STEREO, MIX_51_TO_STEREO_NORM = range(5)


def mix_preset(preset):
    """a preset matrix -> (channels_in, channels_out, int16 array [C_out][C_in]); CoolmicError for an unknown one"""
    ci, co = C.c_uint(), C.c_uint()
    _check("mix_preset", lib.cmhip_mix_preset(preset, C.byref(ci), C.byref(co), None, 0))
    w = np.zeros(ci.value * co.value, dtype=np.int16)
    _check("mix_preset", lib.cmhip_mix_preset(preset, None, None, w.ctypes.data, w.size))
    return ci.value, co.value, w.reshape(co.value, ci.value)


def mix_check(channels_in, channels_out, W):
    """cmhip_mix_check as it is -> error number (0: the matrix is valid); W None is passed as NULL"""
    if W is None:
        return lib.cmhip_mix_check(channels_in, channels_out, None)
    w = np.ascontiguousarray(W, dtype=np.int16)
    return lib.cmhip_mix_check(channels_in, channels_out, w.ctypes.data)


def mix_ramp_position(n, ramp_frames):
    """cmhip_mix_ramp_position: p(n) of a ramp of ramp_frames frames, in units of 2^-15"""
    return lib.cmhip_mix_ramp_position(n, ramp_frames)


def mix_ramp_weight(w0, w1, p):
    """cmhip_mix_ramp_weight: the entry between w0 and w1 at position p"""
    return lib.cmhip_mix_ramp_weight(w0, w1, p)


class BusPlan(C.Structure):
    """cmhip::BusPlan (csrc/cmhip_internal.h): what the mix bus's launcher launches for a run"""
    _fields_ = MixPlan._fields_


def plan_bus(buses, channels_in, channels_out, frames):
    """Test hook: the bus launcher's plan for a run whose longest stream has `frames` frames (host logic, needs no
    GPU)"""
    p = BusPlan()
    lib.cmhip_test_plan_bus(buses, channels_in, channels_out, frames, C.addressof(p))
    return p


def plan_busramp(buses, channels_in, channels_out, frames):
    """Test hook: the plan of a bus run at which a send ramps (host logic, needs no GPU) -> BusPlan"""
    p = BusPlan()
    lib.cmhip_test_plan_busramp(buses, channels_in, channels_out, frames, C.addressof(p))
    return p


def _bus_table(bus, stream, W, channels_in, channels_out):
    """a routing table as three contiguous arrays (uint32 [n], uint32 [n], int16 [n][C_out][C_in]) and n"""
    b = np.ascontiguousarray(bus, dtype=np.uint32).reshape(-1)
    s = np.ascontiguousarray(stream, dtype=np.uint32).reshape(-1)
    w = np.ascontiguousarray(W, dtype=np.int16).reshape(-1, channels_out, channels_in)
    assert b.size == s.size == w.shape[0]
    return b, s, w, b.size


def bus_check(buses, streams, channels_in, channels_out, bus, stream, W, n=None):
    """cmhip_bus_check as it is -> error number (0: the table is valid).  n: the send count handed over when it is not
    the arrays' (they are not read when the sizes alone decide)"""
    if bus is None:
        return lib.cmhip_bus_check(buses, streams, channels_in, channels_out, n or 0, None, None, None)
    b, s, w = (np.ascontiguousarray(bus, dtype=np.uint32), np.ascontiguousarray(stream, dtype=np.uint32),
               np.ascontiguousarray(W, dtype=np.int16))
    return lib.cmhip_bus_check(buses, streams, channels_in, channels_out, b.size if n is None else n, b.ctypes.data,
                               s.ctypes.data, w.ctypes.data)


def bus_mix_minus(n, w, channels=1, cap_sends=None):
    """cmhip_bus_mix_minus -> (bus uint32 [n(n-1)], stream uint32 [n(n-1)], W int16 [n(n-1)][channels][channels]);
    CoolmicError when it is refused"""
    sends = n * (n - 1) if cap_sends is None else cap_sends
    b, s = np.zeros(max(sends, 1), dtype=np.uint32), np.zeros(max(sends, 1), dtype=np.uint32)
    W = np.zeros((max(sends, 1), channels, channels), dtype=np.int16)
    _check("bus_mix_minus", lib.cmhip_bus_mix_minus(n, w, b.ctypes.data, s.ctypes.data, W.ctypes.data, sends, channels))
    k = n * (n - 1)
    return b[:k], s[:k], W[:k]


def bus_compile(buses, streams, channels_in, channels_out, bus, stream, W):
    """Test hook: the routing compiler (csrc/bus_route.h) on a table -> (first uint32 [B+1], stream uint32 [n],
    flag uint32 [n], wk uint32 [n][C_out][CP]); host logic, needs no GPU"""
    b, s, w, n = _bus_table(bus, stream, W, channels_in, channels_out)
    cp = (channels_in + 1) // 2
    first = np.zeros(buses + 1, dtype=np.uint32)
    so, fl = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    wk = np.zeros((max(n, 1), channels_out, cp), dtype=np.uint32)
    _check("bus_compile", lib.cmhip_test_bus_compile(buses, streams, channels_in, channels_out, n, b.ctypes.data,
                                                     s.ctypes.data, w.ctypes.data, first.ctypes.data, so.ctypes.data,
                                                     fl.ctypes.data, wk.ctypes.data))
    return first, so[:n], fl[:n], wk[:n]


class LimPlan(C.Structure):
    """cmhip::LimPlan (csrc/lim_plan.h): what the limiter's launcher launches for a run"""
    _fields_ = [("err", C.c_int)] + [(n, C.c_uint32) for n in ("fast", "grid", "block", "chunks", "tile_frames",
                                                               "lds_bytes", "halo")]


def plan_lim(streams, channels, lookahead_log2, hold, frames):
    """Test hook: the limiter launcher's plan for a run whose longest stream has `frames` frames (host logic, needs no
    GPU)"""
    p = LimPlan()
    lib.cmhip_test_plan_lim(streams, channels, lookahead_log2, hold, frames, C.addressof(p))
    return p


def lim_check(lookahead_log2, hold, threshold, drive):
    """cmhip_lim_check as it is -> error number (0: valid)"""
    return lib.cmhip_lim_check(lookahead_log2, hold, threshold, drive)


LIM_DETECT_SAMPLE, LIM_DETECT_TRUE_PEAK = 0, 1     # CMHIP_LIM_DETECT_*


def plan_limtp(streams, channels, lookahead_log2, hold, frames):
    """Test hook: plan_lim for a limiter with the true-peak detector (host logic, needs no GPU)"""
    p = LimPlan()
    lib.cmhip_test_plan_limtp(streams, channels, lookahead_log2, hold, frames, C.addressof(p))
    return p


def lim_check_detector(detector, lookahead_log2, hold, threshold, drive):
    """cmhip_lim_check_detector as it is -> error number (0: valid)"""
    return lib.cmhip_lim_check_detector(detector, lookahead_log2, hold, threshold, drive)


def plan_limrel(detector, streams, channels, lookahead_log2, hold, release_log2, frames):
    """Test hook: the plan of a run of a limiter with a release stage, for either detector (host logic, needs no GPU);
    release_log2 0 gives plan_lim's or plan_limtp's plan"""
    p = LimPlan()
    lib.cmhip_test_plan_limrel(detector, streams, channels, lookahead_log2, hold, release_log2, frames, C.addressof(p))
    return p


def lim_check_release(detector, lookahead_log2, hold, release_log2, threshold, drive):
    """cmhip_lim_check_release as it is -> error number (0: valid)"""
    return lib.cmhip_lim_check_release(detector, lookahead_log2, hold, release_log2, threshold, drive)


def lim_threshold_dbtp(dbtp):
    """cmhip_lim_threshold_dbtp: the threshold for a ceiling in dBTP (0 for NaN)"""
    return lib.cmhip_lim_threshold_dbtp(dbtp)


DYN_CURVE = 128     # CMHIP_DYN_CURVE


class DynPlan(C.Structure):
    """cmhip::DynPlan (csrc/dyn_plan.h): what the dynamics stage's launcher launches for a run"""
    _fields_ = [("err", C.c_int)] + [(n, C.c_uint32) for n in ("fast", "grid", "block", "chunks", "tile_frames",
                                                               "lds_bytes", "halo", "passes")]


def plan_dyn(streams, channels, detector_log2, smooth_log2, hold, frames):
    """Test hook: the dynamics launcher's plan for a run whose longest stream has `frames` frames (host logic, needs no
    GPU)"""
    p = DynPlan()
    lib.cmhip_test_plan_dyn(streams, channels, detector_log2, smooth_log2, hold, frames, C.addressof(p))
    return p


def dyn_check(detector_log2, smooth_log2, hold):
    """cmhip_dyn_check as it is -> error number (0: valid)"""
    return lib.cmhip_dyn_check(detector_log2, smooth_log2, hold)


DYN_DETECT_MEAN, DYN_DETECT_RMS = 0, 1     # CMHIP_DYN_DETECT_*


def plan_dynrms(streams, channels, detector_log2, smooth_log2, hold, frames):
    """Test hook: plan_dyn for a stage with the RMS detector (host logic, needs no GPU)"""
    p = DynPlan()
    lib.cmhip_test_plan_dynrms(streams, channels, detector_log2, smooth_log2, hold, frames, C.addressof(p))
    return p


def dyn_check_detector(detector, detector_log2, smooth_log2, hold):
    """cmhip_dyn_check_detector as it is -> error number (0: valid)"""
    return lib.cmhip_dyn_check_detector(detector, detector_log2, smooth_log2, hold)


def dyn_isqrt(v):
    """Test hook: the RMS detector's root of a 32-bit value, as the kernels take it (csrc/dyn_plan.h)"""
    return lib.cmhip_test_dyn_isqrt(v)


def _dyn_table(curve):
    t = np.ascontiguousarray(curve, dtype=np.uint16)
    assert t.size == DYN_CURVE
    return t


def dyn_curve_ok(curve):
    """Test hook: what cmhip_dyn_set_curve asks of a table of 128 entries (host logic, needs no GPU)"""
    return bool(lib.cmhip_test_dyn_curve_ok(_dyn_table(curve).ctypes.data))


def dyn_design_rc(comp_threshold_db=0.0, comp_ratio=1.0, comp_knee_db=0.0, gate_threshold_db=-96.0, gate_ratio=1.0,
                  gate_range_db=0.0):
    """cmhip_dyn_design as it is -> (error number, uint16 [128])"""
    d = DynCurveDesc(comp_threshold_db, comp_ratio, comp_knee_db, gate_threshold_db, gate_ratio, gate_range_db)
    t = np.zeros(DYN_CURVE, dtype=np.uint16)
    return lib.cmhip_dyn_design(C.byref(d), t.ctypes.data), t


def dyn_design(**kw):
    """a curve of 128 entries from a compressor (threshold dBFS, ratio, knee dB) and a gate (threshold dBFS, expander
    ratio, range dB; range 0: no gate); host only"""
    rc, t = dyn_design_rc(**kw)
    _check("dyn_design", rc)
    return t


def dyn_design_duck_rc(threshold_db=0.0, depth_db=0.0, knee_db=0.0):
    """cmhip_dyn_design_duck as it is -> (error number, uint16 [128])"""
    d = DynDuckDesc(threshold_db, depth_db, knee_db)
    t = np.zeros(DYN_CURVE, dtype=np.uint16)
    return lib.cmhip_dyn_design_duck(C.byref(d), t.ctypes.data), t


def dyn_design_duck(**kw):
    """a curve of 128 entries for a keyed stream: unity below the key's threshold (dBFS), depth dB down above it, a
    knee of knee dB between; host only"""
    rc, t = dyn_design_duck_rc(**kw)
    _check("dyn_design_duck", rc)
    return t


RUN_FAMILIES = ("none", "fast", "fast_ro", "wide", "rows")     # RunPlan::family


def plan_run(streams, channels, frames, out=False, f32=False, vu=False, identity_maps=True):
    """Test hook: the block-kernel launcher's plan for a run (plan_run in k_block.hip; host logic, needs no GPU).
    A dict of the RunPlan's fields, with the family by name; the completion flag is offered to every run, so
    keep_flag tells the launches of one workgroup."""
    p = RunPlan()
    lib.cmhip_test_plan_run(streams, channels, frames, int(bool(out)), int(bool(f32)), int(bool(vu)),
                            int(bool(identity_maps)), C.byref(p))
    d = {name: getattr(p, name) for name, _ in RunPlan._fields_}
    d["family"] = RUN_FAMILIES[d["family"]]
    return d


def merge_windows(windows, channels, rate=48000):
    """Test hook: raw VU windows (rows of 33 uint64: 16 sums of squares, 16 peak keys, samples accounted), one
    per launch in stream order, merged on the host as a meter behind a tee merges them, and finished."""
    import numpy as np
    w = np.ascontiguousarray(windows, dtype=np.uint64).reshape(-1, 33)
    r = VuResult()
    rc = lib.cmhip_test_merge_windows(w.ctypes.data_as(_P(C.c_uint64)), w.shape[0], channels, rate, C.byref(r))
    return rc, r


def unpack_finished(words, streams, channels, rate=48000, out=None):
    """Test hook (host logic, needs no GPU): the collect's unpack of a device-finished snapshot record, uint64
    [word][stream] as k_vu_finish writes it (csrc/k_misc.hip) -> (results, rc list).  `out`: a VuResult array to
    unpack into (to see what is left alone)."""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
    out = out if out is not None else (VuResult * streams)()
    rc = (C.c_int * streams)()
    _check("unpack_finished", lib.cmhip_test_unpack_finished(w.ctypes.data, streams, channels, rate, out, rc))
    return out, list(rc)


def power_db_device(sums, counts, want_log=False):
    """Test hook: the kernels' own dB finish (vu_power_db, csrc/k_misc.hip) over (sum, count) pairs on the GPU ->
    float64 array of dB values (and, with want_log, the log10 values before the * 20)."""
    s = np.ascontiguousarray(sums, dtype=np.uint64)
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    assert s.shape == c.shape and s.ndim == 1
    db = np.empty(s.size, dtype=np.float64)
    lg = np.empty(s.size, dtype=np.float64) if want_log else None
    _check("power_db_device", lib.cmhip_test_power_db_device(s.ctypes.data, c.ctypes.data, s.size, db.ctypes.data,
                                                             lg.ctypes.data if want_log else None))
    return (db, lg) if want_log else db


def sine_period(rate):
    buf = np.zeros(96, dtype=np.int16)
    n = C.c_size_t()
    rc = lib.coolmic_sine_period(rate, buf.ctypes.data, C.byref(n))
    return rc, buf[: n.value].copy()


def design_biquad(kind, rate, freq, gain_db, q=0.0):
    out = np.zeros(5, dtype=np.float32)
    lib.cmhip_design_biquad(kind, rate, freq, gain_db, q, out.ctypes.data)
    return out


def eq3(rate=48000.0):
    """the 3-band EQ of BASELINE config 3"""
    return np.concatenate([design_biquad(0, rate, 200.0, 3.0),
                           design_biquad(1, rate, 1000.0, -2.0, 1.0),
                           design_biquad(2, rate, 6000.0, 2.0)]).astype(np.float32)


# ---------------------------------------------------------------------------
# the batch engine


def _one_result(fn, handle, index, T, out=None):
    """one stream's (slot's) window through `fn` -> (error number, T); `out`: the T to fill"""
    r = out if out is not None else T()
    return fn(handle, index, C.byref(r)), r


def _all_results(what, fn, handle, n, T, out=None):
    """every stream's (slot's) window at once through `fn` -> (T array, rc list); `out`: the array to fill"""
    out = out if out is not None else (T * n)()
    rc = (C.c_int * n)()
    _check(what, fn(handle, out, rc))
    return out, list(rc)


class Batch:
    def __init__(self, streams, channels, max_frames, flags=OUT_PCM | VU, rate=48000, device=0,
                 hip_stream=None):
        d = BatchDesc(device, streams, channels, rate, max_frames, flags, hip_stream)
        self.h = lib.cmhip_batch_new(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_batch_new", ERROR_GENERIC)
        self.streams, self.channels, self.max_frames, self.flags = streams, channels, max_frames, flags
        self.rate = rate

    def close(self):
        if self.h:
            lib.cmhip_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def placement(self):
        """what the placement search of CMHIP_PLACE_SEARCH did at creation (a dict)"""
        p = Placement()
        _check("placement", lib.cmhip_batch_placement(self.h, C.byref(p)))
        return p.as_dict()

    # parameters
    def set_gain(self, stream, channels, scale, gains):
        arr = (C.c_uint16 * len(gains))(*gains) if gains is not None and len(gains) else None
        return lib.cmhip_batch_set_gain(self.h, stream, channels, scale, arr)

    def set_chmap(self, stream, cmap):
        if cmap is None:
            return lib.cmhip_batch_set_chmap(self.h, stream, None)
        m = np.asarray(cmap, dtype=np.uint8)
        return lib.cmhip_batch_set_chmap(self.h, stream, m.ctypes.data)

    def set_eq(self, stream, coef):
        c = np.ascontiguousarray(coef, dtype=np.float32).reshape(-1)
        return lib.cmhip_batch_set_eq(self.h, stream, c.size // 5, c.ctypes.data if c.size else None)

    def eq_reset(self, stream=-1):
        _check("eq_reset", lib.cmhip_batch_eq_reset(self.h, stream))

    # data
    def upload(self, stream, pcm):
        a = np.ascontiguousarray(pcm, dtype=np.int16)
        _check("upload", lib.cmhip_batch_upload(self.h, stream, a.ctypes.data, a.size // self.channels))

    def download(self, stream, frames):
        out = np.empty(frames * self.channels, dtype=np.int16)
        _check("download", lib.cmhip_batch_download(self.h, stream, out.ctypes.data, frames))
        return out

    def download_f32(self, stream, channel, frames):
        out = np.empty(frames, dtype=np.float32)
        _check("download_f32", lib.cmhip_batch_download_f32(self.h, stream, channel,
                                                            out.ctypes.data, frames))
        return out

    def upload_all(self, host_ptr, frames):
        _check("upload_all", lib.cmhip_batch_upload_all(self.h, host_ptr, frames))

    def download_all(self, host_ptr, frames):
        _check("download_all", lib.cmhip_batch_download_all(self.h, host_ptr, frames))

    def generate(self, mode, seed, frames, first_global=0, global_step=1, frame_offset=0):
        _check("generate", lib.cmhip_batch_generate(self.h, mode, seed & 0xFFFFFFFF, frames,
                                                    first_global, global_step, frame_offset))

    def download_input(self, stream, frames):
        out = np.empty(frames * self.channels, dtype=np.int16)
        _check("download_input", lib.cmhip_batch_download_input(self.h, stream, out.ctypes.data,
                                                                frames))
        return out

    # hot path
    def run(self, frames, frames_per_stream=None):
        if frames_per_stream is None:
            _check("run", lib.cmhip_batch_run(self.h, frames, None))
        else:
            a = np.ascontiguousarray(frames_per_stream, dtype=np.uint32)
            assert a.size == self.streams
            _check("run", lib.cmhip_batch_run(self.h, frames, a.ctypes.data))

    def run_slots(self, frames, slots_in, slots_out, frames_per_stream=None):
        """one pass over PCM arrays named for this run (device pointers; MappedPcm.dev)"""
        fps = None
        if frames_per_stream is not None:
            fps = np.ascontiguousarray(frames_per_stream, dtype=np.uint32)
            assert fps.size == self.streams
        _check("run_slots", lib.cmhip_batch_run_slots(self.h, frames, fps.ctypes.data if fps is not None else None,
                                                      slots_in, slots_out))

    def hip_stream(self):
        """the hipStream_t (as an integer) this batch launches on"""
        return lib.cmhip_batch_hip_stream(self.h) or 0

    def sync(self):
        _check("sync", lib.cmhip_batch_sync(self.h))

    # VU
    def vu_result(self, stream):
        return _one_result(lib.cmhip_batch_vu_result, self.h, stream, VuResult)

    def vu_results(self):
        return _all_results("vu_results", lib.cmhip_batch_vu_results, self.h, self.streams, VuResult)

    def vu_snapshot(self):
        _check("vu_snapshot", lib.cmhip_batch_vu_snapshot(self.h))

    def vu_collect(self, out=None, rc=None):
        out = out if out is not None else (VuResult * self.streams)()
        rc = rc if rc is not None else (C.c_int * self.streams)()
        _check("vu_collect", lib.cmhip_batch_vu_collect(self.h, out, rc))
        return out, rc

    def vu_collect_begin(self, out, rc):
        """first half of vu_collect: the helper threads finish the oldest snapshot into out / rc (ctypes arrays
        that must stay alive) while the caller goes on; vu_collect_end() returns when they are complete"""
        _check("vu_collect_begin", lib.cmhip_batch_vu_collect_begin(self.h, out, rc))

    def vu_collect_end(self):
        _check("vu_collect_end", lib.cmhip_batch_vu_collect_end(self.h))

    def vu_set_finish(self, where):
        """VU_FINISH_HOST / VU_FINISH_DEVICE for the snapshots to come; the error number (BUSY while one is pending)"""
        return lib.cmhip_batch_vu_set_finish(self.h, where)

    def vu_get_finish(self):
        return lib.cmhip_batch_vu_get_finish(self.h)

    def vu_reset(self, stream=-1):
        _check("vu_reset", lib.cmhip_batch_vu_reset(self.h, stream))

    # true peak (opt-in)
    def set_true_peak(self, on):
        """the error number (INVAL while the equaliser has sections)"""
        return lib.cmhip_batch_set_true_peak(self.h, int(bool(on)))

    def get_true_peak(self):
        return lib.cmhip_batch_get_true_peak(self.h)

    def tp_result(self, stream):
        return _one_result(lib.cmhip_batch_tp_result, self.h, stream, TruePeakResult)

    def tp_results(self):
        return _all_results("tp_results", lib.cmhip_batch_tp_results, self.h, self.streams, TruePeakResult)

    def tp_reset(self, stream=-1):
        _check("tp_reset", lib.cmhip_batch_tp_reset(self.h, stream))

    # phase correlation (opt-in)
    def set_correlation(self, on):
        """the error number (INVAL for a mono batch and while the equaliser has sections)"""
        return lib.cmhip_batch_set_correlation(self.h, int(bool(on)))

    def get_correlation(self):
        return lib.cmhip_batch_get_correlation(self.h)

    def corr_set_pairs(self, pairs):
        """pairs: [(a, b), ...] -> the error number (BUSY while a window holds frames)"""
        return lib.cmhip_batch_corr_set_pairs(self.h, len(pairs), _corr_pairs(pairs))

    def corr_result(self, stream, out=None):
        return _one_result(lib.cmhip_batch_corr_result, self.h, stream, CorrResult, out)

    def corr_results(self, out=None):
        return _all_results("corr_results", lib.cmhip_batch_corr_results, self.h, self.streams, CorrResult, out)

    def corr_reset(self, stream=-1):
        _check("corr_reset", lib.cmhip_batch_corr_reset(self.h, stream))

    # spectrum (opt-in)
    def set_spectrum(self, on):
        """the error number (INVAL while the equaliser has sections)"""
        return lib.cmhip_batch_set_spectrum(self.h, int(bool(on)))

    def get_spectrum(self):
        return lib.cmhip_batch_get_spectrum(self.h)

    def spec_configure(self, fft_log2=10, edges=None, channels=None):
        """edges: the nb + 1 bin edges (None: the bin octaves), channels: the transformed channels (None: 0, and 1
        where the batch has it) -> the error number (BUSY while the meter is on)"""
        return lib.cmhip_batch_spec_configure(self.h, fft_log2, *_spec_geometry(edges, channels))

    def spec_result(self, stream, out=None):
        return _one_result(lib.cmhip_batch_spec_result, self.h, stream, SpecResult, out)

    def spec_results(self, out=None):
        return _all_results("spec_results", lib.cmhip_batch_spec_results, self.h, self.streams, SpecResult, out)

    def spec_reset(self, stream=-1):
        _check("spec_reset", lib.cmhip_batch_spec_reset(self.h, stream))

    # signal watch (opt-in)
    def set_watch(self, on):
        """the error number (INVAL while the equaliser has sections)"""
        return lib.cmhip_batch_set_watch(self.h, int(bool(on)))

    def get_watch(self):
        return lib.cmhip_batch_get_watch(self.h)

    def watch_configure(self, quiet=32, rail=32767, clip_run=3):
        """the thresholds of all streams -> the error number (BUSY while a window holds frames)"""
        return lib.cmhip_batch_watch_configure(self.h, quiet, rail, clip_run)

    def watch_result(self, stream, out=None):
        return _one_result(lib.cmhip_batch_watch_result, self.h, stream, WatchResult, out)

    def watch_results(self, out=None):
        return _all_results("watch_results", lib.cmhip_batch_watch_results, self.h, self.streams, WatchResult, out)

    def watch_reset(self, stream=-1):
        _check("watch_reset", lib.cmhip_batch_watch_reset(self.h, stream))

    # loudness (opt-in)
    def set_loudness(self, on):
        """the error number (INVAL while the equaliser has sections or for a rate outside 8000..384000)"""
        return lib.cmhip_batch_set_loudness(self.h, int(bool(on)))

    def get_loudness(self):
        return lib.cmhip_batch_get_loudness(self.h)

    def loud_set_weights(self, stream, weights):
        """the error number (BUSY while the stream holds completed sub-blocks)"""
        if len(weights) != self.channels:
            raise ValueError("loud_set_weights: %d weights for %d channels" % (len(weights), self.channels))
        w = (C.c_double * self.channels)(*weights)
        return lib.cmhip_batch_loud_set_weights(self.h, stream, w)

    def loud_result(self, stream):
        return _one_result(lib.cmhip_batch_loud_result, self.h, stream, LoudnessResult)

    def loud_results(self):
        return _all_results("loud_results", lib.cmhip_batch_loud_results, self.h, self.streams, LoudnessResult)

    def loud_raw(self, stream, cap=30):
        """the trailing min(cap, 30) complete sub-blocks' per-channel sums, oldest first -> ([n][channels] array,
        sub-blocks completed in all)"""
        sums = np.zeros((max(cap, 1), self.channels), dtype=np.float64)
        n, done = C.c_size_t(), C.c_ulonglong()
        _check("loud_raw", lib.cmhip_batch_loud_raw(self.h, stream, sums.ctypes.data, cap, C.byref(n), C.byref(done)))
        return sums[:n.value].copy(), done.value

    def loud_reset(self, stream=-1):
        _check("loud_reset", lib.cmhip_batch_loud_reset(self.h, stream))

    def vu_raw(self, stream):
        power = np.zeros(MAX_CH, dtype=np.int64)
        peak = np.zeros(MAX_CH, dtype=np.int16)
        frames = C.c_uint64()
        _check("vu_raw", lib.cmhip_batch_vu_raw(self.h, stream, power.ctypes.data, peak.ctypes.data,
                                                C.byref(frames)))
        return power, peak, frames.value

    def node_partial(self, dst_device_ptr, first_global=0, global_step=1):
        _check("node_partial", lib.cmhip_batch_vu_node_partial(self.h, dst_device_ptr, first_global,
                                                               global_step))

    def node_record(self, first_global=0, global_step=1):
        """this batch's un-reduced node record in host memory (waits for the last run)"""
        out = np.zeros(NODE_WORDS, dtype=np.int64)
        _check("node_record", lib.cmhip_batch_vu_node_record(self.h, out.ctypes.data, first_global, global_step))
        return out

    # measurement
    def timing(self, enable):
        """True / 1: every run carries events; n > 1: every n-th run; False / 0: off"""
        _check("timing", lib.cmhip_batch_timing(self.h, int(enable)))

    def timing_read(self):
        ms, n = C.c_double(), C.c_uint()
        _check("timing_read", lib.cmhip_batch_timing_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def ceiling(self, mode, iters=10):
        return lib.cmhip_batch_ceiling(self.h, mode, self.max_frames, iters)

    @property
    def stride(self):
        return lib.cmhip_batch_stride(self.h)

    @property
    def dev_in(self):
        return lib.cmhip_batch_dev_in(self.h)

    @property
    def dev_out(self):
        return lib.cmhip_batch_dev_out(self.h)


class _Stage:
    """What the stage objects beside a batch share (Resampler, Mixer, Bus, Dynamics, Limiter, BandSplit, Delay,
    Leveller, Filter, Automixer, Failover, Drift, Denoiser): the end of the handle `h`, its stream, a run and its counts, and reset.  `_stem` names the
    object's C functions: cmhip_<stem>_free, _sync, _hip_stream, _run, _reset.  The Mixer and the Bus have no state to
    reset and the library no cmhip_mix_reset or cmhip_bus_reset: their reset() raises AttributeError, as the lookup of
    any symbol the library lacks does."""

    _stem = None

    def close(self):
        if self.h:
            getattr(lib, "cmhip_%s_free" % self._stem)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(self._stem + "_sync", getattr(lib, "cmhip_%s_sync" % self._stem)(self.h))

    def hip_stream(self):
        return getattr(lib, "cmhip_%s_hip_stream" % self._stem)(self.h) or 0

    def run_rc(self, src, in_stride, frames, dst, out_stride, frames_per_stream=None):
        """cmhip_<stem>_run as it is -> error number"""
        return getattr(lib, "cmhip_%s_run" % self._stem)(self.h, src, in_stride, frames, self._counts(frames_per_stream),
                                                         dst, out_stride)

    def run(self, src, in_stride, frames, dst, out_stride, frames_per_stream=None):
        """one run over device arrays (src, dst: device pointers; the band split's dst: B * S slots, band-major)"""
        _check(self._stem + "_run", self.run_rc(src, in_stride, frames, dst, out_stride, frames_per_stream))

    def reset(self, stream=-1):
        """the stream's state as at creation (stream -1: every stream); ordered with the runs"""
        _check(self._stem + "_reset", getattr(lib, "cmhip_%s_reset" % self._stem)(self.h, stream))

    def _counts(self, frames_per_stream):
        """-> the run's frames_per_stream argument: None, or the uint32 array as ctypes passes it (it holds the array)"""
        if frames_per_stream is None:
            return None
        fps = np.ascontiguousarray(frames_per_stream, dtype=np.uint32)
        assert fps.size == self.streams
        return fps.ctypes


class Resampler(_Stage):
    """cmhip_src_t: sample-rate conversion of S streams beside a batch.  Without `table` the library designs one for
    the rates; with it, table = (L, M, int16 array [L][T])."""

    _stem = "src"

    def __init__(self, streams, channels, rate_in, rate_out, max_in_frames, table=None, device=0, hip_stream=None):
        d = SrcDesc(device, streams, channels, rate_in, rate_out, max_in_frames, hip_stream)
        if table is None:
            self.h = lib.cmhip_src_new(C.byref(d))
        else:
            L, M, h = table
            h = np.ascontiguousarray(h, dtype=np.int16)
            assert h.ndim == 2 and h.shape[0] == L
            self.h = lib.cmhip_src_new_table(C.byref(d), L, M, h.shape[1], h.ctypes.data)
        if not self.h:
            raise CoolmicError("cmhip_src_new", ERROR_INVAL)
        self.streams, self.channels, self.max_in_frames = streams, channels, max_in_frames

    def geometry(self):
        L, M, T = C.c_uint(), C.c_uint(), C.c_uint()
        _check("src_geometry", lib.cmhip_src_geometry(self.h, C.byref(L), C.byref(M), C.byref(T)))
        return L.value, M.value, T.value

    def max_out_frames(self):
        return lib.cmhip_src_max_out_frames(self.h)

    def run_rc(self, src, in_stride, frames, dst, out_stride, frames_per_stream=None):
        """cmhip_src_run as it is -> (error number, uint32 array of the streams' output counts)"""
        got = np.zeros(self.streams, dtype=np.uint32)
        rc = lib.cmhip_src_run(self.h, src, in_stride, frames, self._counts(frames_per_stream), dst, out_stride,
                               got.ctypes.data)
        return rc, got

    def run(self, src, in_stride, frames, dst, out_stride, frames_per_stream=None):
        """one run over device arrays (src, dst: device pointers) -> the streams' output counts"""
        rc, got = self.run_rc(src, in_stride, frames, dst, out_stride, frames_per_stream)
        _check("src_run", rc)
        return got


class Drift(_Stage):
    """cmhip_drift_t: clock-drift compensation of S streams beside a batch, a resampler whose step 2^32 + delta is set
    per stream between runs.  Without `table` the library designs one (phase_log2 7, 32 taps); with it, table is the
    int16 array [2^phase_log2][taps]."""

    _stem = "drift"

    def __init__(self, streams, channels, max_in_frames, table=None, device=0, hip_stream=None, _dry=False):
        d = DriftDesc(device, streams, channels, max_in_frames, hip_stream)
        if _dry or table is not None:
            phi = taps = 0
            if table is not None:
                table = np.ascontiguousarray(table, dtype=np.int16)
                assert table.ndim == 2
                phi, taps = max(table.shape[0].bit_length() - 1, 0), table.shape[1]
                assert table.shape[0] == 1 << phi
        if _dry:
            self.h = lib.cmhip_test_drift_new_dry(C.byref(d), phi, taps, table.ctypes.data if table is not None else None)
        elif table is None:
            self.h = lib.cmhip_drift_new(C.byref(d))
        else:
            self.h = lib.cmhip_drift_new_table(C.byref(d), phi, taps, table.ctypes.data)
        if not self.h:
            raise CoolmicError("cmhip_drift_new", ERROR_INVAL)
        self.streams, self.channels, self.max_in_frames = streams, channels, max_in_frames

    def geometry(self):
        phi, taps = C.c_uint(), C.c_uint()
        _check("drift_geometry", lib.cmhip_drift_geometry(self.h, C.byref(phi), C.byref(taps)))
        return phi.value, taps.value

    def max_out_frames(self):
        return lib.cmhip_drift_max_out_frames(self.h)

    def set_rc(self, stream, delta):
        """cmhip_drift_set as it is -> error number"""
        return lib.cmhip_drift_set(self.h, stream, delta)

    def set(self, stream, delta):
        _check("drift_set", self.set_rc(stream, delta))

    def seek_rc(self, stream, frac):
        """cmhip_drift_seek as it is -> error number"""
        return lib.cmhip_drift_seek(self.h, stream, frac)

    def seek(self, stream, frac):
        _check("drift_seek", self.seek_rc(stream, frac))

    def get(self, stream):
        """-> (delta, pos, total input frames, total output frames) of the host's mirror"""
        d, p, i, o = C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check("drift_get", lib.cmhip_drift_get(self.h, stream, C.byref(d), C.byref(p), C.byref(i), C.byref(o)))
        return d.value, p.value, i.value, o.value

    def advance_rc(self, frames, frames_per_stream=None):
        """Test hook (cmhip_test_drift_advance): the mirror's part of a run -> (error number, output counts)"""
        got = np.zeros(self.streams, dtype=np.uint32)
        rc = lib.cmhip_test_drift_advance(self.h, frames, self._counts(frames_per_stream), got.ctypes.data)
        return rc, got

    def run_rc(self, src, in_stride, frames, dst, out_stride, frames_per_stream=None):
        """cmhip_drift_run as it is -> (error number, uint32 array of the streams' output counts)"""
        got = np.zeros(self.streams, dtype=np.uint32)
        rc = lib.cmhip_drift_run(self.h, src, in_stride, frames, self._counts(frames_per_stream), dst, out_stride,
                                 got.ctypes.data)
        return rc, got

    def run(self, src, in_stride, frames, dst, out_stride, frames_per_stream=None):
        """one run over device arrays (src, dst: device pointers) -> the streams' output counts"""
        rc, got = self.run_rc(src, in_stride, frames, dst, out_stride, frames_per_stream)
        _check("drift_run", rc)
        return got


class BandSplit(_Stage):
    """cmhip_split_t: a linear-phase FIR crossover of S streams beside a batch: B bands that add up to the input delayed
    by delay() frames.  Either `rate` and `crossover_hz` (the library designs the filters) or table = (int16 [B-1][T],
    uint8 [B-1])."""

    _stem = "split"

    def __init__(self, streams, channels, bands, taps, max_frames, rate=None, crossover_hz=None, table=None, device=0,
                 hip_stream=None):
        d = SplitDesc(device, streams, channels, bands, taps, max_frames, hip_stream)
        if table is None:
            self.h = lib.cmhip_split_new(C.byref(d), rate, _crossovers(crossover_hz, bands))
        else:
            g = np.ascontiguousarray(table[0], dtype=np.int16)
            q = np.ascontiguousarray(table[1], dtype=np.uint8)
            assert g.shape == (bands - 1, taps) and q.shape == (bands - 1,)
            self.h = lib.cmhip_split_new_table(C.byref(d), g.ctypes.data, q.ctypes.data)
        if not self.h:
            raise CoolmicError("cmhip_split_new", ERROR_INVAL)
        self.streams, self.channels, self.bands, self.taps, self.max_frames = streams, channels, bands, taps, max_frames

    def delay(self):
        return lib.cmhip_split_delay(self.h)

    def get_table(self):
        g = np.zeros((self.bands - 1, self.taps), dtype=np.int16)
        q = np.zeros(self.bands - 1, dtype=np.uint8)
        _check("split_get_table", lib.cmhip_split_get_table(self.h, g.ctypes.data, q.ctypes.data))
        return g, q

    def clips(self, clear=False):
        """-> uint32 [S][B]: the saturated samples per stream and band (a synchronous round trip)"""
        c = np.zeros((self.streams, self.bands), dtype=np.uint32)
        _check("split_clips", lib.cmhip_split_clips(self.h, c.ctypes.data, 1 if clear else 0))
        return c


class Delay(_Stage):
    """cmhip_delay_t: a delay line of S streams beside a batch, a delay of 0..max_delay frames per stream (0 at
    creation), moved by steps or by click-free crossfades."""

    _stem = "delay"

    def __init__(self, streams, channels, max_delay, max_frames, delay=None, device=0, hip_stream=None, _new=None):
        d = DelayDesc(device, streams, channels, max_delay, max_frames, hip_stream)
        self.h = (_new or lib.cmhip_delay_new)(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_delay_new", ERROR_INVAL)
        self.streams, self.channels, self.max_frames = streams, channels, max_frames
        if delay is not None:
            self.set(-1, delay)

    def max_delay(self):
        return lib.cmhip_delay_max_delay(self.h)

    def set_rc(self, stream, delay):
        """cmhip_delay_set as it is -> error number"""
        return lib.cmhip_delay_set(self.h, stream, delay)

    def set(self, stream, delay):
        """a step between two frames (stream -1: every stream)"""
        _check("delay_set", self.set_rc(stream, delay))

    def ramp_rc(self, stream, delay, ramp_frames):
        """cmhip_delay_ramp as it is -> error number"""
        return lib.cmhip_delay_ramp(self.h, stream, delay, ramp_frames)

    def ramp(self, stream, delay, ramp_frames):
        """a click-free move to `delay` over ramp_frames of the stream's frames (stream -1: every stream)"""
        _check("delay_ramp", self.ramp_rc(stream, delay, ramp_frames))

    def get(self, stream):
        """-> (delay, from, done, ramp_frames); (delay, delay, 0, 0) when nothing ramps"""
        v = [C.c_uint32(0) for _ in range(4)]
        _check("delay_get", lib.cmhip_delay_get(self.h, stream, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)


class Leveller(_Stage):
    """cmhip_agc_t: slow automatic gain control of S streams beside a batch: the gain moves once per window of
    2^window_log2 frames towards target / level.  `params` (an AgcParams): set for every stream at creation (default:
    a copy)."""

    _stem = "agc"

    def __init__(self, streams, channels, window_log2, max_frames, params=None, device=0, hip_stream=None, _new=None):
        d = AgcDesc(device, streams, channels, window_log2, max_frames, hip_stream)
        self.h = (_new or lib.cmhip_agc_new)(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_agc_new", ERROR_INVAL)
        self.streams, self.channels, self.window_log2, self.max_frames = streams, channels, window_log2, max_frames
        if params is not None:
            self.set(-1, params)

    def set_rc(self, stream, params):
        """cmhip_agc_set as it is -> error number"""
        return lib.cmhip_agc_set(self.h, stream, C.byref(params))

    def set(self, stream, params):
        """the stream's parameters from its next window edge on (stream -1: every stream)"""
        _check("agc_set", self.set_rc(stream, params))

    def get(self, stream):
        p = AgcParams()
        _check("agc_get", lib.cmhip_agc_get(self.h, stream, C.byref(p)))
        return p

    def state(self, clear_clips=False):
        """-> (gain uint32 [S], level uint32 [S], clips uint64 [S]); a synchronous round trip"""
        g = np.zeros(self.streams, dtype=np.uint32)
        lv = np.zeros(self.streams, dtype=np.uint32)
        c = np.zeros(self.streams, dtype=np.uint64)
        _check("agc_state", lib.cmhip_agc_state(self.h, g.ctypes.data, lv.ctypes.data, c.ctypes.data,
                                                1 if clear_clips else 0))
        return g, lv, c


class Denoiser(_Stage):
    """cmhip_denoise_t: a noise suppressor of S streams beside a batch: a spectral gate over blocks of 2^fft_log2 frames
    with a learned noise profile per (stream, channel).  `params` (a DenoiseParams): set for every stream at creation
    (default: a pure delay of N - 1 frames)."""

    _stem = "denoise"

    def __init__(self, streams, channels, fft_log2, max_frames, params=None, device=0, hip_stream=None, _new=None):
        d = DenoiseDesc(device, streams, channels, fft_log2, max_frames, hip_stream)
        self.h = (_new or lib.cmhip_denoise_new)(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_denoise_new", ERROR_INVAL)
        self.streams, self.channels, self.fft_log2, self.max_frames = streams, channels, fft_log2, max_frames
        self.bins = (1 << fft_log2) // 2 + 1
        if params is not None:
            self.set(-1, params)

    def delay(self):
        return lib.cmhip_denoise_delay(self.h)

    def set_rc(self, stream, params):
        """cmhip_denoise_set as it is -> error number"""
        return lib.cmhip_denoise_set(self.h, stream, C.byref(params))

    def set(self, stream, params):
        """the stream's parameters from the next block completed on (stream -1: every stream)"""
        _check("denoise_set", self.set_rc(stream, params))

    def get(self, stream):
        p = DenoiseParams()
        _check("denoise_get", lib.cmhip_denoise_get(self.h, stream, C.byref(p)))
        return p

    def learn(self, stream, on):
        """learning of the noise profile on or off (stream -1: every stream); ordered with the runs"""
        _check("denoise_learn", lib.cmhip_denoise_learn(self.h, stream, 1 if on else 0))

    def set_profile_rc(self, stream, channel, profile):
        """cmhip_denoise_set_profile as it is -> error number"""
        q = np.ascontiguousarray(profile, dtype=np.uint64)
        assert q.shape == (self.bins,)
        return lib.cmhip_denoise_set_profile(self.h, stream, channel, q.ctypes.data)

    def set_profile(self, stream, channel, profile):
        """the row's noise profile, uint64 [N/2 + 1]; ordered with the runs"""
        _check("denoise_set_profile", self.set_profile_rc(stream, channel, profile))

    def get_profile(self, stream, channel):
        """-> (profile uint64 [N/2 + 1], gain uint32 [N/2 + 1]) of the row; a synchronous round trip"""
        q = np.zeros(self.bins, dtype=np.uint64)
        g = np.zeros(self.bins, dtype=np.uint32)
        _check("denoise_get_profile", lib.cmhip_denoise_get_profile(self.h, stream, channel, q.ctypes.data, g.ctypes.data))
        return q, g

    def state(self, clear=False):
        """-> (clips uint64 [S], sat uint64 [S], learned_blocks uint32 [S]); a synchronous round trip"""
        c = np.zeros(self.streams, dtype=np.uint64)
        t = np.zeros(self.streams, dtype=np.uint64)
        b = np.zeros(self.streams, dtype=np.uint32)
        _check("denoise_state", lib.cmhip_denoise_state(self.h, c.ctypes.data, t.ctypes.data, b.ctypes.data,
                                                        1 if clear else 0))
        return c, t, b


class Automixer(_Stage):
    """cmhip_automix_t: gain sharing among the streams of a group (Dugan style) beside a batch: every window of
    2^window_log2 frames each member gets the share of one unit of gain that its level earns.  Every stream starts in no
    group (a copy).  `params` (an AutomixParams): set for every stream at creation."""

    _stem = "automix"

    def __init__(self, streams, channels, window_log2, max_frames, params=None, device=0, hip_stream=None, _new=None):
        d = AutomixDesc(device, streams, channels, window_log2, max_frames, hip_stream)
        self.h = (_new or lib.cmhip_automix_new)(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_automix_new", ERROR_INVAL)
        self.streams, self.channels, self.window_log2, self.max_frames = streams, channels, window_log2, max_frames
        if params is not None:
            self.set(-1, params)

    def set_rc(self, stream, params):
        """cmhip_automix_set as it is -> error number"""
        return lib.cmhip_automix_set(self.h, stream, C.byref(params))

    def set(self, stream, params):
        """the stream's parameters from the next run on (stream -1: every stream)"""
        _check("automix_set", self.set_rc(stream, params))

    def get(self, stream):
        p = AutomixParams()
        _check("automix_get", lib.cmhip_automix_get(self.h, stream, C.byref(p)))
        return p

    def set_group_rc(self, stream, group):
        """cmhip_automix_set_group as it is -> error number"""
        return lib.cmhip_automix_set_group(self.h, stream, group)

    def set_group(self, stream, group):
        """the stream joins `group` (-1: leaves its group); the group left and the group joined start afresh"""
        _check("automix_set_group", self.set_group_rc(stream, group))

    def get_group(self, stream):
        g = C.c_long()
        _check("automix_get_group", lib.cmhip_automix_get_group(self.h, stream, C.byref(g)))
        return g.value

    def state(self):
        """-> (gain uint32 [S], power uint64 [S], share uint32 [S]); a synchronous round trip"""
        g = np.zeros(self.streams, dtype=np.uint32)
        pw = np.zeros(self.streams, dtype=np.uint64)
        sh = np.zeros(self.streams, dtype=np.uint32)
        _check("automix_state", lib.cmhip_automix_state(self.h, g.ctypes.data, pw.ctypes.data, sh.ctypes.data))
        return g, pw, sh


class Failover(_Stage):
    """cmhip_failover_t: a silence-triggered source changeover beside a batch: each of `outputs` outputs is a copy of one
    of up to four candidate input streams, judged once per window of 2^window_log2 frames, with a crossfade at every
    changeover.  Output o starts with the one candidate min(o, streams - 1).  `params` (a FailoverParams): set for every
    output at creation.  Counts of a run are per OUTPUT."""

    _stem = "failover"

    def __init__(self, streams, outputs, channels, window_log2, max_frames, params=None, device=0, hip_stream=None,
                 _new=None):
        d = FailoverDesc(device, streams, outputs, channels, window_log2, max_frames, hip_stream)
        self.h = (_new or lib.cmhip_failover_new)(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_failover_new", ERROR_INVAL)
        self.inputs, self.outputs, self.channels, self.window_log2, self.max_frames = (streams, outputs, channels,
                                                                                        window_log2, max_frames)
        self.streams = outputs                       # (what _Stage._counts holds a run's counts against)
        if params is not None:
            self.set(-1, params)

    def set_rc(self, output, params):
        """cmhip_failover_set as it is -> error number"""
        return lib.cmhip_failover_set(self.h, output, C.byref(params))

    def set(self, output, params):
        """the output's parameters from the next run on (output -1: every output)"""
        _check("failover_set", self.set_rc(output, params))

    def get(self, output):
        p = FailoverParams()
        _check("failover_get", lib.cmhip_failover_get(self.h, output, C.byref(p)))
        return p

    def set_sources_rc(self, output, streams):
        """cmhip_failover_set_sources as it is -> error number"""
        s = np.ascontiguousarray(streams, dtype=np.uint32)
        return lib.cmhip_failover_set_sources(self.h, output, s.size, s.ctypes.data)

    def set_sources(self, output, streams):
        """the output's candidate list, main source first; the output starts afresh and is automatic again"""
        _check("failover_set_sources", self.set_sources_rc(output, streams))

    def get_sources(self, output):
        n = C.c_uint(0)
        s = np.zeros(4, dtype=np.uint32)
        _check("failover_get_sources", lib.cmhip_failover_get_sources(self.h, output, C.byref(n), s.ctypes.data))
        return [int(v) for v in s[:n.value]]

    def state(self, clear=False):
        """-> dict of from, to, fade_window (uint32 [O]), switches (uint64 [O]), live_run, dead_run, level (uint32
        [O][4]); a synchronous round trip"""
        O = self.outputs
        r = {k: np.zeros(O, dtype=np.uint32) for k in ("from", "to", "fade_window")}
        r["switches"] = np.zeros(O, dtype=np.uint64)
        r.update({k: np.zeros((O, 4), dtype=np.uint32) for k in ("live_run", "dead_run", "level")})
        _check("failover_state", lib.cmhip_failover_state(self.h, r["from"].ctypes.data, r["to"].ctypes.data,
                                                          r["fade_window"].ctypes.data, r["switches"].ctypes.data,
                                                          1 if clear else 0, r["live_run"].ctypes.data,
                                                          r["dead_run"].ctypes.data, r["level"].ctypes.data))
        return r


class Filter(_Stage):
    """cmhip_iir_t: a cascade of `sections` biquads in exact integers over S streams beside a batch; every section is
    unity (a copy) until set."""

    _stem = "iir"

    def __init__(self, streams, channels, sections, max_frames, device=0, hip_stream=None, _new=None):
        d = IirDesc(device, streams, channels, sections, max_frames, hip_stream)
        self.h = (_new or lib.cmhip_iir_new)(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_iir_new", ERROR_INVAL)
        self.streams, self.channels, self.sections, self.max_frames = streams, channels, sections, max_frames

    def set_rc(self, stream, section, sec):
        """cmhip_iir_set as it is -> error number"""
        return lib.cmhip_iir_set(self.h, stream, section, C.byref(sec))

    def set(self, stream, section, sec):
        """the stream's section from its next frame on (stream -1: every stream)"""
        _check("iir_set", self.set_rc(stream, section, sec))

    def get(self, stream, section):
        """the section in force: between its ends while it ramps"""
        s = IirSection()
        _check("iir_get", lib.cmhip_iir_get(self.h, stream, section, C.byref(s)))
        return s

    def ramp_rc(self, stream, section, target, ramp_frames):
        """cmhip_iir_ramp as it is -> error number"""
        return lib.cmhip_iir_ramp(self.h, stream, section, C.byref(target), ramp_frames)

    def ramp(self, stream, section, target, ramp_frames):
        """the stream's section moves to `target` over its next ramp_frames frames, from the section in force (stream
        -1: every stream; 0 or 1 frames: set)"""
        _check("iir_ramp", self.ramp_rc(stream, section, target, ramp_frames))

    def ramp_state(self, stream, section):
        """-> (done, ramp_frames) of the section's ramp, (0, 0) at rest; from the host mirror"""
        done, frames = C.c_uint32(), C.c_uint32()
        _check("iir_ramp_state", lib.cmhip_iir_ramp_state(self.h, stream, section, C.byref(done), C.byref(frames)))
        return done.value, frames.value

    def state(self, clear=False):
        """-> (clips uint64 [S], overs uint64 [S]); a synchronous round trip"""
        c = np.zeros(self.streams, dtype=np.uint64)
        o = np.zeros(self.streams, dtype=np.uint64)
        _check("iir_state", lib.cmhip_iir_state(self.h, c.ctypes.data, o.ctypes.data, 1 if clear else 0))
        return c, o

    def rows(self):
        """Test hook: the rows' sections as the device holds them -> int32 [S * C][N][5] (u1, u2, v1, v2, e)"""
        r = np.zeros((self.streams * self.channels, self.sections, 5), dtype=np.int32)
        _check("iir_rows", lib.cmhip_test_iir_rows(self.h, r.ctypes.data))
        return r


class Mixer(_Stage):
    """cmhip_mix_t: channel mixing of S streams beside a batch, one matrix int16 [C_out][C_in] (units of 2^-14) per
    stream.  `matrix`: set for every stream at creation (default: the leading channels kept)."""

    _stem = "mix"

    def __init__(self, streams, channels_in, channels_out, max_frames, matrix=None, device=0, hip_stream=None):
        d = MixDesc(device, streams, channels_in, channels_out, max_frames, hip_stream)
        self.h = lib.cmhip_mix_new(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_mix_new", ERROR_INVAL)
        self.streams, self.channels_in, self.channels_out, self.max_frames = streams, channels_in, channels_out, max_frames
        if matrix is not None:
            self.set_matrix(-1, matrix)

    def set_matrix_rc(self, stream, W):
        """cmhip_mix_set_matrix as it is -> error number"""
        w = np.ascontiguousarray(W, dtype=np.int16)
        assert w.size == self.channels_out * self.channels_in
        return lib.cmhip_mix_set_matrix(self.h, stream, w.ctypes.data)

    def set_matrix(self, stream, W):
        """stream -1: every stream.  Ordered with the runs on the mixer's stream."""
        _check("mix_set_matrix", self.set_matrix_rc(stream, W))

    def get_matrix(self, stream):
        w = np.zeros((self.channels_out, self.channels_in), dtype=np.int16)
        _check("mix_get_matrix", lib.cmhip_mix_get_matrix(self.h, stream, w.ctypes.data))
        return w

    def ramp_matrix_rc(self, stream, W, ramp_frames):
        """cmhip_mix_ramp_matrix as it is -> error number"""
        w = np.ascontiguousarray(W, dtype=np.int16)
        assert w.size == self.channels_out * self.channels_in
        return lib.cmhip_mix_ramp_matrix(self.h, stream, w.ctypes.data, ramp_frames)

    def ramp_matrix(self, stream, W, ramp_frames):
        """a click-free move to W over ramp_frames of the stream's frames (stream -1: every stream, each from its own
        matrix in force).  Ordered with the runs on the mixer's stream."""
        _check("mix_ramp_matrix", self.ramp_matrix_rc(stream, W, ramp_frames))

    def ramp_state(self, stream):
        """-> (done, ramp_frames, the matrix in force int16 [C_out][C_in]); (0, 0, the matrix) when nothing ramps"""
        done, total = C.c_uint32(0), C.c_uint32(0)
        w = np.zeros((self.channels_out, self.channels_in), dtype=np.int16)
        _check("mix_ramp_state", lib.cmhip_mix_ramp_state(self.h, stream, C.byref(done), C.byref(total), w.ctypes.data))
        return done.value, total.value, w


class Bus(_Stage):
    """cmhip_bus_t: a mix bus beside a batch -- `streams` input slots summed into `buses` output slots by a routing
    table of sends (bus, stream, W int16 [C_out][C_in] in units of 2^-14).  Routing at creation: empty."""

    _stem = "bus"

    def __init__(self, streams, buses, channels_in, channels_out, max_frames, max_sends, device=0, hip_stream=None):
        d = BusDesc(device, streams, buses, channels_in, channels_out, max_frames, max_sends, hip_stream)
        self.h = lib.cmhip_bus_new(C.byref(d))
        if not self.h:
            raise CoolmicError("cmhip_bus_new", ERROR_INVAL)
        self.streams, self.buses, self.channels_in, self.channels_out = streams, buses, channels_in, channels_out
        self.max_frames, self.max_sends = max_frames, max_sends

    def set_routing_rc(self, bus, stream, W):
        """cmhip_bus_set_routing as it is -> error number"""
        b, s, w, n = _bus_table(bus, stream, W, self.channels_in, self.channels_out)
        return lib.cmhip_bus_set_routing(self.h, n, b.ctypes.data, s.ctypes.data, w.ctypes.data)

    def set_routing(self, bus, stream, W):
        """replaces the whole table; ordered with the runs on the object's stream"""
        _check("bus_set_routing", self.set_routing_rc(bus, stream, W))

    def sends(self):
        return lib.cmhip_bus_sends(self.h)

    def get_routing(self):
        n = self.sends()
        b, s = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        w = np.zeros((max(n, 1), self.channels_out, self.channels_in), dtype=np.int16)
        _check("bus_get_routing", lib.cmhip_bus_get_routing(self.h, n, b.ctypes.data, s.ctypes.data, w.ctypes.data))
        return b[:n], s[:n], w[:n]

    def ramp_sends_rc(self, first, W, ramp_frames):
        """cmhip_bus_ramp_sends as it is -> error number; W int16 [count][C_out][C_in]"""
        w = np.ascontiguousarray(W, dtype=np.int16).reshape(-1, self.channels_out, self.channels_in)
        return lib.cmhip_bus_ramp_sends(self.h, first, w.shape[0], w.ctypes.data, ramp_frames)

    def ramp_sends(self, first, W, ramp_frames):
        """a click-free move of sends first .. (the caller's order) to W over ramp_frames output frames of their buses;
        ramp_frames 0 or 1: a step.  Ordered with the runs on the object's stream."""
        _check("bus_ramp_sends", self.ramp_sends_rc(first, W, ramp_frames))

    def ramp_state(self, send):
        """-> (done, ramp_frames, the matrix in force int16 [C_out][C_in]); (0, 0, the matrix) when the send is at rest"""
        done, total = C.c_uint32(0), C.c_uint32(0)
        w = np.zeros((self.channels_out, self.channels_in), dtype=np.int16)
        _check("bus_ramp_state", lib.cmhip_bus_ramp_state(self.h, send, C.byref(done), C.byref(total), w.ctypes.data))
        return done.value, total.value, w

    def run_rc(self, src, in_stride, frames, dst, out_stride, frames_per_stream=None, out_frames=None):
        """cmhip_bus_run as it is -> error number; out_frames: a uint32 array of `buses` entries or None"""
        return lib.cmhip_bus_run(self.h, src, in_stride, frames, self._counts(frames_per_stream), dst, out_stride,
                                 out_frames.ctypes.data if out_frames is not None else None)

    def run(self, src, in_stride, frames, dst, out_stride, frames_per_stream=None):
        """one run over device arrays (src, dst: device pointers) -> every bus's frame count (uint32 [buses])"""
        got = np.zeros(self.buses, dtype=np.uint32)
        _check("bus_run", self.run_rc(src, in_stride, frames, dst, out_stride, frames_per_stream, got))
        return got


class Limiter(_Stage):
    """cmhip_lim_t: a look-ahead peak limiter of S streams beside a batch; per stream a threshold (sample units) and a
    drive (units of 2^-12).  The output is the input delayed by delay() frames and never above the threshold.
    detector=None creates it with cmhip_lim_new, a detector (LIM_DETECT_SAMPLE: the same limiter; LIM_DETECT_TRUE_PEAK: the
    gain follows the 4x oversampled signal) with cmhip_lim_new_detector.  release_log2=None leaves the constructor as
    that; a number (0..11: the gain rises by at most 32768 >> release_log2 per frame; 0: no release stage) creates the
    limiter with cmhip_lim_new_release, detector None then meaning the sample detector."""

    _stem = "lim"

    def __init__(self, streams, channels, lookahead_log2, hold, max_frames, threshold=None, drive=None, device=0,
                 hip_stream=None, detector=None, release_log2=None):
        d = LimDesc(device, streams, channels, lookahead_log2, hold, max_frames, hip_stream)
        if release_log2 is not None:
            what, self.h = "cmhip_lim_new_release", lib.cmhip_lim_new_release(
                C.byref(d), LIM_DETECT_SAMPLE if detector is None else detector, release_log2)
        elif detector is None:                      # the constructor without a detector: the sample detector
            what, self.h = "cmhip_lim_new", lib.cmhip_lim_new(C.byref(d))
        else:
            what, self.h = "cmhip_lim_new_detector", lib.cmhip_lim_new_detector(C.byref(d), detector)
        if not self.h:
            raise CoolmicError(what, ERROR_INVAL)
        self.streams, self.channels, self.max_frames = streams, channels, max_frames
        if threshold is not None or drive is not None:
            self.set(-1, 32767 if threshold is None else threshold, 4096 if drive is None else drive)

    def delay(self):
        return lib.cmhip_lim_delay(self.h)

    def detector(self):
        return lib.cmhip_lim_detector(self.h)

    def release(self):
        """release_log2 (0: no release stage)"""
        return lib.cmhip_lim_release(self.h)

    def set_rc(self, stream, threshold, drive):
        """cmhip_lim_set as it is -> error number"""
        return lib.cmhip_lim_set(self.h, stream, threshold, drive)

    def set(self, stream, threshold, drive):
        """stream -1: every stream.  Ordered with the runs on the limiter's stream."""
        _check("lim_set", self.set_rc(stream, threshold, drive))

    def get(self, stream):
        t, d = C.c_uint(), C.c_uint()
        _check("lim_get", lib.cmhip_lim_get(self.h, stream, C.byref(t), C.byref(d)))
        return t.value, d.value

    def min_gain(self, reset=False):
        """waits for the stream -> the streams' gain-reduction meters, uint32 [S] in Q15"""
        out = np.zeros(self.streams, dtype=np.uint32)
        _check("lim_min_gain", lib.cmhip_lim_min_gain(self.h, out.ctypes.data, 1 if reset else 0))
        return out


class Dynamics(_Stage):
    """cmhip_dyn_t: a compressor / gate of S streams beside a batch; per stream a curve of 128 uint16 gains (Q15, at most
    32768) over a level grid of 8 knots per octave (dyn_design makes one).  The output is the input delayed by delay()
    frames and never louder than it; make-up gain is the drive of the Limiter that follows.  set_key lets the level of
    another stream steer a stream's gain (a side-chain: ducking, linked stems).  detector=None creates it with
    cmhip_dyn_new, a detector (DYN_DETECT_MEAN: the same stage; DYN_DETECT_RMS: the level is the root of the mean square)
    with cmhip_dyn_new_detector."""

    _stem = "dyn"

    def __init__(self, streams, channels, detector_log2, smooth_log2, hold, max_frames, curve=None, device=0,
                 hip_stream=None, detector=None):
        d = DynDesc(device, streams, channels, detector_log2, smooth_log2, hold, max_frames, hip_stream)
        if detector is None:                        # the constructor without a detector: the mean detector
            what, self.h = "cmhip_dyn_new", lib.cmhip_dyn_new(C.byref(d))
        else:
            what, self.h = "cmhip_dyn_new_detector", lib.cmhip_dyn_new_detector(C.byref(d), detector)
        if not self.h:
            raise CoolmicError(what, ERROR_INVAL)
        self.streams, self.channels, self.max_frames = streams, channels, max_frames
        if curve is not None:
            self.set_curve(-1, curve)

    def delay(self):
        return lib.cmhip_dyn_delay(self.h)

    def detector(self):
        return lib.cmhip_dyn_detector(self.h)

    def set_curve_rc(self, stream, curve):
        """cmhip_dyn_set_curve as it is -> error number"""
        return lib.cmhip_dyn_set_curve(self.h, stream, _dyn_table(curve).ctypes.data)

    def set_curve(self, stream, curve):
        """stream -1: every stream.  Ordered with the runs on the stage's stream."""
        _check("dyn_set_curve", self.set_curve_rc(stream, curve))

    def get_curve(self, stream):
        t = np.zeros(DYN_CURVE, dtype=np.uint16)
        _check("dyn_get_curve", lib.cmhip_dyn_get_curve(self.h, stream, t.ctypes.data))
        return t

    def set_key_rc(self, stream, key):
        """cmhip_dyn_set_key as it is -> error number"""
        return lib.cmhip_dyn_set_key(self.h, stream, key)

    def set_key(self, stream, key):
        """the detector of `stream` (-1: every stream) reads stream `key` (-1, or the stream itself: its own frames).
        Ordered with the runs on the stage's stream."""
        _check("dyn_set_key", self.set_key_rc(stream, key))

    def get_key(self, stream):
        """-> the stream's key, -1 for its own detector (from the host's mirror)"""
        k = C.c_long()
        _check("dyn_get_key", lib.cmhip_dyn_get_key(self.h, stream, C.byref(k)))
        return k.value

    def min_gain(self, reset=False):
        """waits for the stream -> the streams' gain meters, uint32 [S] in Q15"""
        out = np.zeros(self.streams, dtype=np.uint32)
        _check("dyn_min_gain", lib.cmhip_dyn_min_gain(self.h, out.ctypes.data, 1 if reset else 0))
        return out


class PinnedPcm:
    """pinned host mirror of a batch's PCM slots: numpy view int16 [S][stride]"""

    def __init__(self, batch):
        self.shape = (batch.streams, batch.stride)
        self.nbytes = batch.streams * batch.stride * 2
        self.ptr = lib.cmhip_host_alloc(self.nbytes)
        if not self.ptr:
            raise CoolmicError("cmhip_host_alloc", ERROR_NOMEM)
        buf = (C.c_int16 * (self.nbytes // 2)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=np.int16).reshape(self.shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib.cmhip_host_free(self.ptr)
            self.ptr = None


class DeviceWords:
    """n int64 words of plain device memory (cmhip_device_alloc): `.dev` for the engine, read() for the host"""

    def __init__(self, n, device=0):
        self.n, self.device = n, device
        self.dev = lib.cmhip_device_alloc(device, n * 8)
        if not self.dev:
            raise CoolmicError("cmhip_device_alloc", ERROR_NOMEM)

    def read(self):
        out = np.zeros(self.n, dtype=np.int64)
        _check("device_read", lib.cmhip_device_read(self.device, out.ctypes.data, self.dev, self.n * 8))
        return out

    def free(self):
        if self.dev:
            lib.cmhip_device_free(self.device, self.dev)
            self.dev = None


class MappedPcm:
    """pinned, device-mapped host mirror of a batch's slot layout: numpy view int16 [S][stride] on the
    host, `.dev` for cmhip_batch_run_slots"""

    def __init__(self, batch):
        self.shape = (batch.streams, batch.stride)
        self.nbytes = batch.streams * batch.stride * 2
        dev = C.c_void_p()
        self.ptr = lib.cmhip_host_alloc_mapped(self.nbytes, C.byref(dev))
        if not self.ptr:
            raise CoolmicError("cmhip_host_alloc_mapped", ERROR_NOMEM)
        self.dev = dev.value
        buf = (C.c_int16 * (self.nbytes // 2)).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=np.int16).reshape(self.shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib.cmhip_host_free(self.ptr)
            self.ptr = None


def node_finish(words, channels, rate=48000):
    w = np.ascontiguousarray(words, dtype=np.int64)
    assert w.size == NODE_WORDS
    r = VuResult()
    rc = lib.cmhip_node_finish(w.ctypes.data, channels, rate, C.byref(r))
    return rc, r


NODE_ID_BYTES = 128


def node_unique_id():
    """rank 0: the 128-byte id every rank hands to Node() (ncclGetUniqueId)"""
    buf = (C.c_ubyte * NODE_ID_BYTES)()
    _check("node_unique_id", lib.cmhip_node_unique_id(buf))
    return bytes(buf)


def node_runtime():
    """'hip=<path> rccl=<path>': the HIP runtime the engine is bound to and the librccl it resolved"""
    return lib.cmhip_node_runtime().decode()


def node_merge_host(records):
    """SUM / MAX of per-rank node records on the host (the no-collective form)"""
    w = np.ascontiguousarray(records, dtype=np.int64).reshape(-1, NODE_WORDS)
    out = np.zeros(NODE_WORDS, dtype=np.int64)
    _check("node_merge_host", lib.cmhip_node_merge_host(w.ctypes.data, w.shape[0], out.ctypes.data))
    return out


class Node:
    """cmhip_node_t: the node-global VU exchange over RCCL, one per GPU / rank"""

    def __init__(self, device, nranks, rank, unique_id, max_records=8):
        assert len(unique_id) == NODE_ID_BYTES
        self._id = (C.c_ubyte * NODE_ID_BYTES).from_buffer_copy(unique_id)
        self.max_records = max_records
        self.h = lib.cmhip_node_new(device, nranks, rank, self._id, max_records)
        if not self.h:
            raise CoolmicError("cmhip_node_new: " + last_error(), ERROR_GENERIC)

    def close(self):
        if self.h:
            lib.cmhip_node_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ranks(self):
        return lib.cmhip_node_ranks(self.h)

    def partial(self, batch, set_, slot, first_global=0, global_step=1):
        _check("node_partial", lib.cmhip_node_partial(self.h, batch.h, set_, slot, first_global, global_step))

    def allreduce(self, set_, count, after=None):
        _check("node_allreduce", lib.cmhip_node_allreduce(self.h, set_, count, after.h if after else None))

    def fetch(self, set_, count):
        out = np.zeros((count, NODE_WORDS), dtype=np.int64)
        _check("node_fetch", lib.cmhip_node_fetch(self.h, set_, count, out.ctypes.data))
        return out


# ---------------------------------------------------------------------------
# the reference's per-stream operator API


_alive = {}


class IoHandle:
    """Owns one reference to a coolmic_iohandle_t."""

    def __init__(self, ptr, keep=()):
        if not ptr:
            raise CoolmicError("iohandle", ERROR_GENERIC)
        self.ptr = ptr
        self._keep = keep

    @classmethod
    def from_callbacks(cls, read, eof=None, free=None):
        """read(nbytes) -> bytes | int(<=0); eof() -> int.  The ctypes thunks stay alive
        until the C side runs the handle's free callback (i.e. until the last unref)."""
        token = object()

        def _read(_ud, buf, n):
            got = read(n)
            if isinstance(got, int):
                return got
            got = bytes(got)[:n]
            C.memmove(buf, got, len(got))
            return len(got)

        def _free(_ud):
            if free:
                free()
            _alive.pop(id(token), None)
            return 0

        rcb = READ_FN(_read)
        ecb = EOF_FN((lambda _ud: eof())) if eof else EOF_FN()
        fcb = FREE_FN(_free)
        _alive[id(token)] = (token, rcb, ecb, fcb)
        ptr = lib.coolmic_iohandle_new(None, None, None, fcb, rcb, ecb)
        if not ptr:
            _alive.pop(id(token), None)
        return cls(ptr)

    @classmethod
    def from_bytes(cls, data, chunk=0):
        """serves `data` in pieces of at most `chunk` bytes (0: as asked), then reports EOF"""
        state = {"pos": 0}
        data = bytes(data)

        def read(n):
            k = min(n, len(data) - state["pos"])
            if chunk:
                k = min(k, chunk)
            out = data[state["pos"]: state["pos"] + k]
            state["pos"] += k
            return out

        return cls.from_callbacks(read, eof=lambda: 1 if state["pos"] >= len(data) else 0)

    def read(self, nbytes):
        buf = (C.c_ubyte * max(nbytes, 1))()
        n = lib.coolmic_iohandle_read(self.ptr, buf, nbytes)
        return n, bytes(buf[: max(n, 0)])

    def eof(self):
        return lib.coolmic_iohandle_eof(self.ptr)

    def refcount(self):
        return lib.coolmic_ro_refcount(self.ptr)

    def root(self):
        """Test hook (cmhip_test_iohandle_root, needs no GPU): the address of the object this handle finally reads
        from, through the tees and transforms attached right now; None for a chain too long to walk.  Streams of
        a group whose handles have one root stay on the pumping thread."""
        return lib.cmhip_test_iohandle_root(self.ptr)

    def unref(self):
        if self.ptr:
            lib.coolmic_ro_unref(self.ptr)
            self.ptr = None


class Snddev:
    def __init__(self, driver, rate=48000, channels=1, flags=1, device=None):
        self.ptr = lib.coolmic_snddev_new(None, None, driver.encode() if driver else None,
                                          C.c_char_p(device.encode()) if device else None,
                                          rate, channels, flags, -1)
        if not self.ptr:
            raise CoolmicError("coolmic_snddev_new", ERROR_GENERIC)

    def get_iohandle(self):
        return IoHandle(lib.coolmic_snddev_get_iohandle(self.ptr))

    def attach(self, handle):
        return lib.coolmic_snddev_attach_iohandle(self.ptr, handle.ptr if handle else None)

    def iter(self):
        return lib.coolmic_snddev_iter(self.ptr)

    def unref(self):
        if self.ptr:
            lib.coolmic_ro_unref(self.ptr)
            self.ptr = None


class Transform:
    def __init__(self, rate=48000, channels=1):
        self.ptr = lib.coolmic_transform_new(None, None, rate, channels)
        if not self.ptr:
            raise CoolmicError("coolmic_transform_new", ERROR_GENERIC)
        self.channels = channels

    def attach(self, handle):
        return lib.coolmic_transform_attach_iohandle(self.ptr, handle.ptr if handle else None)

    def get_iohandle(self):
        return IoHandle(lib.coolmic_transform_get_iohandle(self.ptr))

    def set_master_gain(self, channels, scale, gains):
        arr = (C.c_uint16 * len(gains))(*gains) if gains is not None and len(gains) else None
        return lib.coolmic_transform_set_master_gain(self.ptr, channels, scale, arr)

    def set_channel_map(self, cmap):
        if cmap is None:
            return lib.coolmic_transform_set_channel_map(self.ptr, None)
        m = np.asarray(cmap, dtype=np.uint8)
        return lib.coolmic_transform_set_channel_map(self.ptr, m.ctypes.data)

    def set_device(self, device):
        return lib.coolmic_transform_set_device(self.ptr, device)

    def set_eq(self, coef):
        """coef: 5 floats per section (b0 b1 b2 a1 a2), or None / empty to switch the filter off"""
        if coef is None or len(coef) == 0:
            return lib.coolmic_transform_set_eq(self.ptr, 0, None)
        c = np.ascontiguousarray(coef, dtype=np.float32)
        return lib.coolmic_transform_set_eq(self.ptr, c.size // 5, c.ctypes.data)

    def refcount(self):
        return lib.coolmic_ro_refcount(self.ptr)

    def unref(self):
        if self.ptr:
            lib.coolmic_ro_unref(self.ptr)
            self.ptr = None


class Vumeter:
    def __init__(self, rate=48000, channels=1):
        self.ptr = lib.coolmic_vumeter_new(None, None, rate, channels)
        if not self.ptr:
            raise CoolmicError("coolmic_vumeter_new", ERROR_GENERIC)
        self.channels = channels

    def attach(self, handle):
        return lib.coolmic_vumeter_attach_iohandle(self.ptr, handle.ptr if handle else None)

    def read(self, maxlen=-1):
        return lib.coolmic_vumeter_read(self.ptr, maxlen)

    def result(self):
        r = VuResult()
        rc = lib.coolmic_vumeter_result(self.ptr, C.byref(r))
        return rc, r

    def reset(self):
        return lib.coolmic_vumeter_reset(self.ptr)

    def set_device(self, device):
        return lib.coolmic_vumeter_set_device(self.ptr, device)

    def mode(self):
        """test hook: 0 own batch, 1 shares the launch of the transform right above, 2 shares it through a tee"""
        return lib.coolmic_debug_vumeter_mode(self.ptr)

    def unref(self):
        if self.ptr:
            lib.coolmic_ro_unref(self.ptr)
            self.ptr = None


class Tee:
    def __init__(self, readers):
        self.ptr = lib.coolmic_tee_new(None, None, readers)
        if not self.ptr:
            raise CoolmicError("coolmic_tee_new", ERROR_GENERIC)

    def attach(self, handle):
        return lib.coolmic_tee_attach_iohandle(self.ptr, handle.ptr if handle else None)

    def get_iohandle(self, index=-1):
        return IoHandle(lib.coolmic_tee_get_iohandle(self.ptr, index))

    def unref(self):
        if self.ptr:
            lib.coolmic_ro_unref(self.ptr)
            self.ptr = None


class Group:
    """coolmic_group_t: many transform -> vumeter pipelines, one launch per block"""

    def __init__(self, channels, max_streams, block_frames, queue_blocks=2, rate=48000, device=None):
        if device is None:
            self.ptr = lib.coolmic_group_new(None, None, rate, channels, max_streams, block_frames,
                                             queue_blocks)
        else:
            self.ptr = lib.coolmic_group_new_on(device, None, None, rate, channels, max_streams, block_frames,
                                                queue_blocks)
        if not self.ptr:
            raise CoolmicError("coolmic_group_new", ERROR_GENERIC)
        self.channels = channels

    @property
    def device(self):
        return lib.coolmic_group_device(self.ptr)

    def engine(self):
        """the group's cmhip_batch_t (a borrowed pointer: cmhip_node_partial and friends)"""
        return lib.coolmic_group_engine(self.ptr)

    def add_stream(self, handle):
        return lib.coolmic_group_add_stream(self.ptr, handle.ptr if handle else None)

    def set_master_gain(self, slot, channels, scale, gains):
        arr = (C.c_uint16 * len(gains))(*gains) if gains is not None and len(gains) else None
        return lib.coolmic_group_set_master_gain(self.ptr, slot, channels, scale, arr)

    def set_channel_map(self, slot, cmap):
        if cmap is None:
            return lib.coolmic_group_set_channel_map(self.ptr, slot, None)
        m = np.asarray(cmap, dtype=np.uint8)
        return lib.coolmic_group_set_channel_map(self.ptr, slot, m.ctypes.data)

    def set_eq(self, slot, coef):
        if coef is None or len(coef) == 0:
            return lib.coolmic_group_set_eq(self.ptr, slot, 0, None)
        c = np.ascontiguousarray(coef, dtype=np.float32)
        return lib.coolmic_group_set_eq(self.ptr, slot, c.size // 5, c.ctypes.data)

    def get_iohandle(self, slot):
        return IoHandle(lib.coolmic_group_get_iohandle(self.ptr, slot))

    def pump(self):
        return lib.coolmic_group_pump(self.ptr)

    def set_pull_threads(self, threads):
        return lib.coolmic_group_set_pull_threads(self.ptr, threads)

    def shared_source(self, slot):
        """Test hook (cmhip_test_group_shared_source): 1 when the stream was recognised as reading from the same
        object as another stream of the group (it stays on the pumping thread), 0 when not, ERROR_INVAL: no slot"""
        return lib.cmhip_test_group_shared_source(self.ptr, slot)

    def _results(self, call, T, out):
        return _all_results("group_" + call, getattr(lib, "coolmic_group_" + call), self.ptr, self.streams(), T, out)

    def vumeter_result(self, slot):
        return _one_result(lib.coolmic_group_vumeter_result, self.ptr, slot, VuResult)

    def vumeter_results(self, out=None):
        """every slot's window in one snapshot and collect -> (VuResult array, rc list); `out`: the array to fill"""
        return self._results("vumeter_results", VuResult, out)

    def set_vu_finish(self, where):
        return lib.coolmic_group_set_vu_finish(self.ptr, where)

    def set_true_peak(self, on):
        return lib.coolmic_group_set_true_peak(self.ptr, int(bool(on)))

    def true_peak(self, slot):
        return _one_result(lib.coolmic_group_true_peak, self.ptr, slot, TruePeakResult)

    def true_peaks(self, out=None):
        """every slot's true-peak window at once -> (TruePeakResult array, rc list); `out`: the array to fill"""
        return self._results("true_peaks", TruePeakResult, out)

    def set_correlation(self, on):
        return lib.coolmic_group_set_correlation(self.ptr, int(bool(on)))

    def correlation_set_pairs(self, pairs):
        return lib.coolmic_group_correlation_set_pairs(self.ptr, len(pairs), _corr_pairs(pairs))

    def correlation(self, slot, out=None):
        return _one_result(lib.coolmic_group_correlation, self.ptr, slot, CorrResult, out)

    def correlations(self, out=None):
        """every slot's correlation window at once -> (CorrResult array, rc list); `out`: the array to fill"""
        return self._results("correlations", CorrResult, out)

    def correlation_reset(self, slot=-1):
        return lib.coolmic_group_correlation_reset(self.ptr, slot)

    def set_spectrum(self, on):
        return lib.coolmic_group_set_spectrum(self.ptr, int(bool(on)))

    def spectrum_configure(self, fft_log2=10, edges=None, channels=None):
        return lib.coolmic_group_spectrum_configure(self.ptr, fft_log2, *_spec_geometry(edges, channels))

    def spectrum(self, slot, out=None):
        return _one_result(lib.coolmic_group_spectrum, self.ptr, slot, SpecResult, out)

    def spectra(self, out=None):
        """every slot's spectrum window at once -> (SpecResult array, rc list); `out`: the array to fill"""
        return self._results("spectra", SpecResult, out)

    def spectrum_reset(self, slot=-1):
        return lib.coolmic_group_spectrum_reset(self.ptr, slot)

    def set_watch(self, on):
        return lib.coolmic_group_set_watch(self.ptr, int(bool(on)))

    def watch_configure(self, quiet=32, rail=32767, clip_run=3):
        return lib.coolmic_group_watch_configure(self.ptr, quiet, rail, clip_run)

    def watch(self, slot, out=None):
        return _one_result(lib.coolmic_group_watch, self.ptr, slot, WatchResult, out)

    def watches(self, out=None):
        """every slot's watch window at once -> (WatchResult array, rc list); `out`: the array to fill"""
        return self._results("watches", WatchResult, out)

    def watch_reset(self, slot=-1):
        return lib.coolmic_group_watch_reset(self.ptr, slot)

    def set_loudness(self, on):
        return lib.coolmic_group_set_loudness(self.ptr, int(bool(on)))

    def loudness(self, slot):
        return _one_result(lib.coolmic_group_loudness, self.ptr, slot, LoudnessResult)

    def loudnesses(self, out=None):
        """every slot's loudness at once -> (LoudnessResult array, rc list); `out`: the array to fill"""
        return self._results("loudnesses", LoudnessResult, out)

    def loudness_set_weights(self, slot, weights):
        if len(weights) != self.channels:
            raise ValueError("loudness_set_weights: %d weights for %d channels" % (len(weights), self.channels))
        w = (C.c_double * self.channels)(*weights)
        return lib.coolmic_group_loudness_set_weights(self.ptr, slot, w)

    def loudness_reset(self, slot=-1):
        return lib.coolmic_group_loudness_reset(self.ptr, slot)

    def streams(self):
        return lib.coolmic_group_streams(self.ptr)

    def unref(self):
        if self.ptr:
            lib.coolmic_ro_unref(self.ptr)
            self.ptr = None


_log_keep = []


def set_log_callback(fn):
    """fn(level:int, msg:str) or None"""
    if fn is None:
        lib.coolmic_logging_set_cb_simple(LOG_FN())
        return
    cb = LOG_FN(lambda lvl, msg: fn(lvl, msg.decode(errors="replace")) or 0)
    _log_keep.append(cb)
    lib.coolmic_logging_set_cb_simple(cb)
