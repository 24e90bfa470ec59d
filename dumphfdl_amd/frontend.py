"""ctypes mirror of include/hfdl_gpu.h (libhfdl_gpu.so).  No compute happens in Python."""
import ctypes as C
import os
import sys
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PDU_MAX_OCTETS = 960

TAP_SPECTRUM, TAP_FILTER, TAP_CHAN_OUT, TAP_RESAMPLED, TAP_MF_OUT, TAP_SYMBOLS, TAP_AGC_LEVEL, TAP_PHASE_CYCLES, TAP_NCO_PHASORS, TAP_NOTCH_OUT = range(1, 11)


SFMT_CF32, SFMT_CS16, SFMT_CU8 = 0, 1, 2
SFMT_RS16, SFMT_RF32 = 3, 4      # real samples, int16 / float32: a RealFrontend's formats (HFDL_GPU_SFMT_RS16 / _RF32)
FCS_GOOD, FCS_BAD, FCS_TOO_SHORT = 0, 1, 2
KIND_SPDU, KIND_MPDU_DOWNLINK, KIND_MPDU_UPLINK = 0, 1, 2


class GpuError(RuntimeError):
    pass


class Geometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "sample_rate", "decimation", "pre_decimation", "post_decimation", "taps_length", "overlap_length",
        "fft_size", "fft_inv_size", "input_size", "post_input_size", "scrap", "outputs_per_block",
        "channels", "fold_slices")] + [("transition_bw", C.c_float), ("resamp_rate", C.c_float), ("max_outputs_per_block", C.c_int32), ("demod_batch", C.c_int32), ("fold_batch", C.c_int32),
                                       ("prefetch_depth", C.c_int32), ("fold_rows", C.c_int32)]


class Pdu(C.Structure):
    _fields_ = [("channel", C.c_int32), ("freq", C.c_int32), ("mode", C.c_int32), ("bit_rate", C.c_int32),
                ("len", C.c_int32), ("freq_err_hz", C.c_float), ("rssi_db", C.c_float), ("noise_floor_db", C.c_float),
                ("slot", C.c_char), ("fcs_status", C.c_uint8), ("pdu_kind", C.c_uint8), ("hdr_len", C.c_uint16),
                ("sample_index", C.c_uint64),
                ("train_bits_bad", C.c_int32), ("train_bits_total", C.c_int32),
                ("lpdus_processed", C.c_uint8), ("lpdus_good", C.c_uint8), ("lpdus_bad_fcs", C.c_uint8), ("lpdus_too_short", C.c_uint8),
                ("lpdus_truncated", C.c_uint8), ("lpdu_pad", C.c_uint8 * 3),
                ("octets", C.c_uint8 * PDU_MAX_OCTETS)]


class ChannelStats(C.Structure):
    _fields_ = [("freq", C.c_int32), ("a2_found", C.c_uint32), ("m1_found", C.c_uint32), ("m1_not_found", C.c_uint32),
                ("frames", C.c_uint32), ("noise_floor_db", C.c_float), ("agc_level", C.c_float), ("costas_dphi", C.c_float),
                ("framer_state", C.c_int32), ("sample_cnt", C.c_uint64), ("symbol_cnt", C.c_uint64),
                ("a1_found", C.c_uint32), ("a1_corr_avg", C.c_float), ("a2_corr_avg", C.c_float), ("m1_corr_avg", C.c_float),
                ("train_bits_bad", C.c_uint32), ("train_bits_total", C.c_uint32)]


class FrameQuality(C.Structure):
    _fields_ = [("sample_index", C.c_uint64), ("channel", C.c_int32), ("freq", C.c_int32), ("mode", C.c_int32), ("bitmask_lsb", C.c_int32),
                ("nsym", C.c_int32), ("segments", C.c_int32), ("train_bits_bad", C.c_int32), ("train_bits_total", C.c_int32),
                ("freq_err_hz", C.c_float), ("rssi_db", C.c_float), ("noise_floor_db", C.c_float),
                ("sym_power", C.c_float), ("err_power", C.c_float), ("err_max", C.c_float), ("gain_re", C.c_float), ("gain_im", C.c_float),
                ("seg_err_power", C.c_float * 168)]


class SpectrumRow(C.Structure):
    _fields_ = [("row", C.c_uint64), ("first_block", C.c_uint64), ("blocks", C.c_uint32), ("pad", C.c_uint32)]


class BlankerStats(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("samples_blanked", C.c_uint64), ("last_power", C.c_float), ("last_threshold", C.c_float)]


class IqbalStats(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("refused", C.c_uint64), ("kappa_re", C.c_float), ("kappa_im", C.c_float), ("dc_re", C.c_float), ("dc_im", C.c_float),
                ("power", C.c_float), ("image_rejection_db", C.c_float), ("valid", C.c_uint32), ("hold", C.c_uint32)]


class NotchStats(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("resets", C.c_uint64), ("last_in_power", C.c_float), ("last_out_power", C.c_float), ("tap_energy", C.c_float)]


class FrontendCounters(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("pdus_taken", C.c_uint32), ("pdus_dropped", C.c_uint32), ("pdu_ring_capacity", C.c_uint32)]


def lib_path():
    # HFDL_GPU_LIB: load a specific build of the library (A/B measurements of two builds in one gpurun)
    return os.environ.get("HFDL_GPU_LIB") or os.path.join(_HERE, "libhfdl_gpu.so")


def lab_lib_path():
    return os.environ.get("HFDL_GPU_LAB_LIB") or os.path.join(_HERE, "libhfdl_gpu_lab.so")


_lib = None
_lab = None

# every symbol include/hfdl_gpu.h declares (tests/test_host_lib_cpu.py compares this list with the header and with `nm -D`)
EXPORTS = [
    "hfdl_gpu_plan_geometry", "hfdl_gpu_host_alloc", "hfdl_gpu_host_free",
    "hfdl_gpu_frontend_create", "hfdl_gpu_frontend_destroy", "hfdl_gpu_frontend_geometry",
    "hfdl_gpu_frontend_push_block", "hfdl_gpu_frontend_push_block_raw", "hfdl_gpu_frontend_input_done", "hfdl_gpu_frontend_input_done_upto", "hfdl_gpu_frontend_channelize_block", "hfdl_gpu_frontend_sync",
    "hfdl_gpu_frontend_poll_pdus", "hfdl_gpu_frontend_poll_pdus_ready", "hfdl_gpu_frontend_counters", "hfdl_gpu_frontend_all_channel_stats", "hfdl_gpu_frontend_stream", "hfdl_gpu_frontend_read_tap",
    "hfdl_gpu_frontend_channel_stats", "hfdl_gpu_frontend_enable_taps", "hfdl_gpu_frontend_fold_time_ms", "hfdl_gpu_frontend_demod_time_ms", "hfdl_gpu_frontend_reset_timers", "hfdl_gpu_frontend_step_period_ms", "hfdl_gpu_last_stage_ms",
    "hfdl_gpu_frontend_fold_blocks", "hfdl_gpu_frontend_fold_launch_shapes", "hfdl_gpu_frontend_stage_times", "hfdl_gpu_frontend_read_tap_block", "hfdl_gpu_frontend_push_baseband", "hfdl_gpu_frontend_input_copied",
    "hfdl_gpu_fft_forward", "hfdl_gpu_viterbi27", "hfdl_gpu_burst_decode", "hfdl_gpu_nco_decimate", "hfdl_gpu_crc16_ccitt", "hfdl_gpu_pdu_triage", "hfdl_gpu_lpdu_walk", "hfdl_gpu_frontend_prefetch_block_raw", "hfdl_gpu_frontend_prefetch_cancel", "hfdl_gpu_psk_slice",
    "hfdl_gpu_last_error", "hfdl_gpu_device_count",
    "hfdl_gpu_frontend_create_multi", "hfdl_gpu_frontend_push_blocks_raw", "hfdl_gpu_frontend_channel_receiver",
    "hfdl_gpu_frontend_spectrum_enable", "hfdl_gpu_frontend_spectrum_read",
    "hfdl_gpu_frontend_spectrum_history", "hfdl_gpu_frontend_spectrum_row_close", "hfdl_gpu_frontend_spectrum_rows",
    "hfdl_gpu_frontend_export_enable", "hfdl_gpu_frontend_export_read",
    "hfdl_gpu_frontend_retune_channel",
    "hfdl_gpu_frontend_quality_enable", "hfdl_gpu_frontend_quality_read", "hfdl_gpu_frame_quality_batch",
    "hfdl_gpu_frontend_blanker_enable", "hfdl_gpu_frontend_blanker_stats", "hfdl_gpu_blank_block",
    "hfdl_gpu_frontend_notch_enable", "hfdl_gpu_frontend_notch_stats", "hfdl_gpu_notch_rows",
    "hfdl_gpu_frontend_iqbal_enable", "hfdl_gpu_frontend_iqbal_seed", "hfdl_gpu_frontend_iqbal_stats", "hfdl_gpu_iqbal_blocks",
    "hfdl_gpu_frontend_create_real", "hfdl_gpu_frontend_real_input",
]


FOLD_BATCH_MAX = 32        # HFDL_GPU_FOLD_BATCH_MAX of include/hfdl_gpu.h
RECEIVERS_MAX = 64         # HFDL_GPU_RECEIVERS_MAX
SPECTRUM_HANN, SPECTRUM_MAXHOLD = 1, 2     # HFDL_GPU_SPECTRUM_*
SPECTRUM_ROWS_MAX = 1024   # HFDL_GPU_SPECTRUM_ROWS_MAX
EXPORT_CF32, EXPORT_CS16 = 0, 1            # HFDL_GPU_EXPORT_*
EXPORT_RING_MAX = 4096     # HFDL_GPU_EXPORT_RING_MAX
QUALITY_SYMBOLS = 1        # HFDL_GPU_QUALITY_SYMBOLS
QUALITY_SEGMENTS_MAX, QUALITY_SYMBOLS_MAX, QUALITY_RING_MAX = 168, 5040, 65536     # HFDL_GPU_QUALITY_*

# what include/hfdl_gpu_lab.h adds in the laboratory build (libhfdl_gpu_lab.so)
LAB_EXPORTS = ["hfdl_gpu_lab_fold_variant_count", "hfdl_gpu_lab_fold_variant_describe", "hfdl_gpu_lab_fold_variant_probe", "hfdl_gpu_lab_stream_read_probe",
               "hfdl_gpu_lab_read_constants", "hfdl_gpu_lab_clock_probe_read", "hfdl_gpu_lab_burst_soft"]
LAB_VIN_MAX = 15120        # HFDL_GPU_LAB_VIN_MAX of include/hfdl_gpu_lab.h


def fold_variants():
    """The compiled tilings of the matrix-pipe fold kernel in the laboratory build: [(P, Q, W, D, max blocks, tap layout)]."""
    L = load_lab()
    out = []
    for v in range(L.hfdl_gpu_lab_fold_variant_count()):
        d = (C.c_int32 * 6)()
        _check(L.hfdl_gpu_lab_fold_variant_describe(v, C.byref(d)), L)
        out.append(tuple(d))
    return out


def load():
    """Load libhfdl_gpu.so.  If torch is going to be used in this process it must own the HIP runtime:
    torch bundles its own libamdhip64 with the same SONAME, so it is imported first when available in sys.modules."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise GpuError("libhfdl_gpu.so is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(dumphfdl_amd/csrc/build.sh). There is no CPU fallback.")
    if "torch" in sys.modules:
        import torch  # noqa: F401  (already imported: make sure its HIP runtime is the one resolved)
    _lib = _bind(C.CDLL(p, mode=C.RTLD_GLOBAL))
    return _lib


def load_lab():
    """Load the laboratory build (libhfdl_gpu_lab.so: include/hfdl_gpu_lab.h on top of include/hfdl_gpu.h).  It lives beside the
    product library in one process; Frontend(..., lib=load_lab()) binds a front end to it."""
    global _lab
    if _lab is not None:
        return _lab
    p = lab_lib_path()
    if not os.path.exists(p):
        raise GpuError("libhfdl_gpu_lab.so is missing: build it with dumphfdl_amd/csrc/build.sh lab")
    if "torch" in sys.modules:
        import torch  # noqa: F401
    L = _bind(C.CDLL(p, mode=C.RTLD_LOCAL))
    L.hfdl_gpu_lab_fold_variant_describe.argtypes = [C.c_int, C.POINTER(C.c_int32 * 6)]
    L.hfdl_gpu_lab_fold_variant_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.hfdl_gpu_lab_stream_read_probe.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.hfdl_gpu_lab_read_constants.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.hfdl_gpu_lab_clock_probe_read.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.hfdl_gpu_lab_burst_soft.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    _lab = L
    return L


def _bind(L):
    L.hfdl_gpu_last_error.restype = C.c_char_p
    L.hfdl_gpu_frontend_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
    L.hfdl_gpu_frontend_destroy.argtypes = [C.c_void_p]
    L.hfdl_gpu_plan_geometry.argtypes = [C.c_int32, C.c_float, C.POINTER(Geometry)]
    L.hfdl_gpu_host_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hfdl_gpu_host_free.argtypes = [C.c_void_p]
    L.hfdl_gpu_host_free.restype = None
    L.hfdl_gpu_frontend_destroy.restype = None
    L.hfdl_gpu_frontend_geometry.argtypes = [C.c_void_p, C.POINTER(Geometry)]
    L.hfdl_gpu_frontend_push_block.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hfdl_gpu_frontend_channelize_block.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hfdl_gpu_frontend_push_block_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    L.hfdl_gpu_frontend_push_baseband.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.hfdl_gpu_frontend_sync.argtypes = [C.c_void_p]
    L.hfdl_gpu_frontend_input_done.argtypes = [C.c_void_p]
    L.hfdl_gpu_frontend_input_done_upto.argtypes = [C.c_void_p, C.c_uint64]
    L.hfdl_gpu_frontend_poll_pdus.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.hfdl_gpu_frontend_poll_pdus_ready.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    L.hfdl_gpu_frontend_counters.argtypes = [C.c_void_p, C.POINTER(FrontendCounters)]
    L.hfdl_gpu_frontend_all_channel_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.hfdl_gpu_frontend_stream.argtypes = [C.c_void_p]
    L.hfdl_gpu_frontend_stream.restype = C.c_void_p
    L.hfdl_gpu_frontend_read_tap.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.hfdl_gpu_frontend_read_tap_block.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.hfdl_gpu_frontend_enable_taps.argtypes = [C.c_void_p, C.c_int]
    L.hfdl_gpu_frontend_channel_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ChannelStats)]
    L.hfdl_gpu_frontend_fold_time_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.hfdl_gpu_frontend_demod_time_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.hfdl_gpu_frontend_fold_blocks.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.hfdl_gpu_frontend_fold_launch_shapes.argtypes = [C.c_void_p, C.POINTER(C.c_int64 * (FOLD_BATCH_MAX + 1)), C.POINTER(C.c_double * (FOLD_BATCH_MAX + 1))]
    L.hfdl_gpu_frontend_input_copied.argtypes = [C.c_void_p, C.c_uint64]
    L.hfdl_gpu_frontend_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_double * 5), C.POINTER(C.c_int64 * 5)]
    L.hfdl_gpu_frontend_reset_timers.argtypes = [C.c_void_p, C.c_int]
    L.hfdl_gpu_fft_forward.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int]
    L.hfdl_gpu_viterbi27.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.hfdl_gpu_burst_decode.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.hfdl_gpu_frontend_step_period_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.hfdl_gpu_last_stage_ms.restype = C.c_double
    L.hfdl_gpu_nco_decimate.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                        C.c_void_p, C.POINTER(C.c_int32)]
    L.hfdl_gpu_crc16_ccitt.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint16, C.POINTER(C.c_uint16)]
    L.hfdl_gpu_pdu_triage.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hfdl_gpu_lpdu_walk.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.hfdl_gpu_psk_slice.argtypes = [C.c_int, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.hfdl_gpu_frontend_prefetch_block_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hfdl_gpu_frontend_prefetch_cancel.argtypes = [C.c_void_p]
    L.hfdl_gpu_frontend_create_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hfdl_gpu_frontend_push_blocks_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    L.hfdl_gpu_frontend_channel_receiver.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.hfdl_gpu_frontend_spectrum_enable.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
    L.hfdl_gpu_frontend_spectrum_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
    L.hfdl_gpu_frontend_spectrum_history.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.hfdl_gpu_frontend_spectrum_row_close.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.hfdl_gpu_frontend_spectrum_rows.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_int]
    L.hfdl_gpu_frontend_export_enable.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_float, C.c_int32]
    L.hfdl_gpu_frontend_export_read.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_int]
    L.hfdl_gpu_frontend_retune_channel.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.hfdl_gpu_frontend_quality_enable.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
    L.hfdl_gpu_frontend_quality_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_int]
    L.hfdl_gpu_frame_quality_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.hfdl_gpu_frontend_blanker_enable.argtypes = [C.c_void_p, C.c_float]
    L.hfdl_gpu_frontend_blanker_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(BlankerStats)]
    L.hfdl_gpu_blank_block.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int, C.c_float, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    L.hfdl_gpu_frontend_iqbal_enable.argtypes = [C.c_void_p, C.c_int32, C.c_float]
    L.hfdl_gpu_frontend_iqbal_seed.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int]
    L.hfdl_gpu_frontend_iqbal_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(IqbalStats)]
    L.hfdl_gpu_iqbal_blocks.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.hfdl_gpu_frontend_notch_enable.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_float]
    L.hfdl_gpu_frontend_notch_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(NotchStats)]
    L.hfdl_gpu_notch_rows.argtypes = [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    L.hfdl_gpu_frontend_create_real.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hfdl_gpu_frontend_real_input.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return L


def _check(rc, L=None):
    if rc != 0:
        raise GpuError("hfdl_gpu error %d: %s" % (rc, (L or load()).hfdl_gpu_last_error().decode(errors="replace")))


def plan_geometry(decimation, transition_bw):
    g = Geometry()
    _check(load().hfdl_gpu_plan_geometry(decimation, transition_bw, C.byref(g)))
    return g


def host_alloc(nbytes):
    p = C.c_void_p()
    _check(load().hfdl_gpu_host_alloc(C.byref(p), nbytes))
    return p.value


def host_free(ptr):
    load().hfdl_gpu_host_free(C.c_void_p(ptr))


def device_count():
    return load().hfdl_gpu_device_count()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Frontend:
    """All HFDL channels of one wideband receiver on one GPU (hfdl_gpu_frontend_*).

    Mirrors the reference wiring fft_create + N x hfdl_channel_create (src/main.c:699-755): one block of
    `geometry.input_size` samples in, PDUs out."""

    def __init__(self, sample_rate, centerfreq, freqs, device=0, lib=None):
        L = self._L = lib or load()
        fr = np.ascontiguousarray(freqs, dtype=np.int32)
        self._h = C.c_void_p()
        _check(L.hfdl_gpu_frontend_create(C.byref(self._h), device, sample_rate, centerfreq, _p(fr), len(fr)), self._L)
        self.geometry = Geometry()
        _check(L.hfdl_gpu_frontend_geometry(self._h, C.byref(self.geometry)), self._L)
        self.freqs = [int(f) for f in fr]
        self.centerfreq = int(centerfreq)
        self._spec_bins, self._spec_peak = 0, False

    @property
    def input_size(self):
        return self.geometry.input_size

    def push_block(self, samples):
        """samples: complex64 numpy array of input_size samples (host), or an int device pointer."""
        L = self._L
        if isinstance(samples, int):
            _check(L.hfdl_gpu_frontend_push_block(self._h, C.c_void_p(samples), self.geometry.input_size, 1), self._L)
        else:
            s = np.ascontiguousarray(samples, dtype=np.complex64)
            _check(L.hfdl_gpu_frontend_push_block(self._h, _p(s), len(s), 0), self._L)
            # the copy is enqueued asynchronously from pageable memory: HIP stages it before returning

    def push_block_raw(self, raw, sample_format):
        """raw: int16 (SFMT_CS16) / uint8 (SFMT_CU8) / float32 (SFMT_CF32) numpy array of 2*input_size interleaved I,Q values."""
        dt = {SFMT_CF32: np.float32, SFMT_CS16: np.int16, SFMT_CU8: np.uint8}[sample_format]
        r = np.ascontiguousarray(raw, dtype=dt)
        _check(self._L.hfdl_gpu_frontend_push_block_raw(self._h, _p(r), len(r) // 2, sample_format, 0), self._L)

    def channelize_block(self, samples):
        L = self._L
        if isinstance(samples, int):
            _check(L.hfdl_gpu_frontend_channelize_block(self._h, C.c_void_p(samples), self.geometry.input_size, 1), self._L)
        else:
            s = np.ascontiguousarray(samples, dtype=np.complex64)
            _check(L.hfdl_gpu_frontend_channelize_block(self._h, _p(s), len(s), 0), self._L)

    def push_baseband(self, per_channel):
        """per_channel: one complex64 array of channelizer OUTPUT per channel (<= max_outputs_per_block + 1 samples each): the demodulator
        and burst decoder stage alone, fed from the host (stage parity)."""
        g = self.geometry
        row = g.max_outputs_per_block + 1
        assert len(per_channel) == g.channels
        buf = np.zeros((g.channels, row), np.complex64)
        cnt = np.zeros(g.channels, np.int32)
        for c, x in enumerate(per_channel):
            x = np.asarray(x, np.complex64)
            buf[c, :len(x)] = x
            cnt[c] = len(x)
        _check(self._L.hfdl_gpu_frontend_push_baseband(self._h, _p(buf), _p(cnt)), self._L)

    def push_host_ptr(self, ptr, sample_format=SFMT_CF32):
        """ptr: address of a (page-locked) host buffer holding one block; valid until input_done() / sync()."""
        _check(self._L.hfdl_gpu_frontend_push_block_raw(self._h, C.c_void_p(ptr), self.geometry.input_size, sample_format, 0), self._L)

    def prefetch_host_ptr(self, ptr, sample_format=SFMT_CF32):
        """Queue the copy of a block that push_host_ptr(ptr, sample_format) will push later (up to geometry.prefetch_depth wait this
        way; they are pushed in the order they were prefetched)."""
        _check(self._L.hfdl_gpu_frontend_prefetch_block_raw(self._h, C.c_void_p(ptr), self.geometry.input_size, sample_format), self._L)

    def prefetch_cancel(self):
        _check(self._L.hfdl_gpu_frontend_prefetch_cancel(self._h), self._L)

    def input_done(self):
        _check(self._L.hfdl_gpu_frontend_input_done(self._h), self._L)

    def input_copied(self, host_block):
        """True once the upload of that host block has finished (no waiting)."""
        rc = self._L.hfdl_gpu_frontend_input_copied(self._h, C.c_uint64(host_block))
        if rc < 0:
            _check(rc, self._L)
        return bool(rc)

    def input_done_upto(self, host_block):
        _check(self._L.hfdl_gpu_frontend_input_done_upto(self._h, C.c_uint64(host_block)), self._L)

    def sync(self):
        _check(self._L.hfdl_gpu_frontend_sync(self._h), self._L)

    def poll_pdus_raw(self, max_pdus=4096, max_in_flight=0):
        """The C structs as the library hands them over: (ctypes array of hfdl_gpu_pdu, count)."""
        buf = (Pdu * max_pdus)()
        n = C.c_int32(0)
        if max_in_flight:
            _check(self._L.hfdl_gpu_frontend_poll_pdus_ready(self._h, buf, max_pdus, C.byref(n), max_in_flight), self._L)
        else:
            _check(self._L.hfdl_gpu_frontend_poll_pdus(self._h, buf, max_pdus, C.byref(n)), self._L)
        return buf, n.value

    @staticmethod
    def pdus_to_dicts(buf, n):
        out = []
        for i in range(n):
            p = buf[i]
            out.append(dict(channel=p.channel, freq=p.freq, mode=p.mode, bit_rate=p.bit_rate,
                            octets=bytes(p.octets[:p.len]), freq_err_hz=p.freq_err_hz, rssi_db=p.rssi_db,
                            noise_floor_db=p.noise_floor_db, slot=p.slot.decode(), sample_index=p.sample_index,
                            fcs_status=p.fcs_status, pdu_kind=p.pdu_kind, hdr_len=p.hdr_len,
                            train_bits_bad=p.train_bits_bad, train_bits_total=p.train_bits_total,
                            lpdus=(p.lpdus_processed, p.lpdus_good, p.lpdus_bad_fcs, p.lpdus_too_short, p.lpdus_truncated)))
        return out

    def poll_pdus(self, max_pdus=4096, max_in_flight=0):
        """max_in_flight=0: everything decoded so far (drains the pipeline); 1: nothing is drained -- the half being filled keeps
        filling, the newest closed half keeps running, and what is known complete (the half before it) is returned: nothing until two
        halves of geometry.fold_batch blocks were closed, and the tail only comes with a draining poll (include/hfdl_gpu.h)."""
        return self.pdus_to_dicts(*self.poll_pdus_raw(max_pdus, max_in_flight))

    def counters(self):
        c = FrontendCounters()
        _check(self._L.hfdl_gpu_frontend_counters(self._h, C.byref(c)), self._L)
        return {n: getattr(c, n) for n, _ in FrontendCounters._fields_}

    def all_channel_stats(self):
        nch = self.geometry.channels
        buf = (ChannelStats * nch)()
        n = C.c_int32(0)
        _check(self._L.hfdl_gpu_frontend_all_channel_stats(self._h, buf, nch, C.byref(n)), self._L)
        return [{k: getattr(buf[i], k) for k, _ in ChannelStats._fields_} for i in range(n.value)]

    def read_tap(self, what, channel=0, back=0):
        """back: TAP_SPECTRUM / TAP_CHAN_OUT / TAP_NCO_PHASORS of the block `back` blocks before the newest (within the newest half)."""
        g = self.geometry
        cap = 2 * g.fft_size if what in (TAP_SPECTRUM, TAP_FILTER) else 2 * (g.post_input_size + 64) * max(1, g.demod_batch)   # demodulator taps cover a launch
        buf = np.empty(cap, np.float32)
        n = C.c_size_t(0)
        _check(self._L.hfdl_gpu_frontend_read_tap_block(self._h, what, channel, back, _p(buf), cap, C.byref(n)), self._L)
        out = buf[:n.value].copy()
        return out if what in (TAP_AGC_LEVEL, TAP_PHASE_CYCLES) else out.view(np.complex64)

    def enable_taps(self, enable=True):
        _check(self._L.hfdl_gpu_frontend_enable_taps(self._h, int(enable)), self._L)

    def channel_stats(self, channel):
        st = ChannelStats()
        _check(self._L.hfdl_gpu_frontend_channel_stats(self._h, channel, C.byref(st)), self._L)
        return {n: getattr(st, n) for n, _ in ChannelStats._fields_}

    def reset_timers(self, enable=True):
        _check(self._L.hfdl_gpu_frontend_reset_timers(self._h, int(enable)), self._L)

    def fold_time_ms(self):
        ms = C.c_double(0)
        n = C.c_int64(0)
        _check(self._L.hfdl_gpu_frontend_fold_time_ms(self._h, C.byref(ms), C.byref(n)), self._L)
        return ms.value, n.value

    def fold_blocks(self):
        """Blocks covered by the timed fold launches (a launch folds up to geometry.fold_batch blocks)."""
        n = C.c_int64(0)
        _check(self._L.hfdl_gpu_frontend_fold_blocks(self._h, C.byref(n)), self._L)
        return n.value

    def fold_launch_shapes(self):
        """{blocks per launch: timed fold launches of that size} since reset_timers(True)."""
        c = (C.c_int64 * (FOLD_BATCH_MAX + 1))()
        _check(self._L.hfdl_gpu_frontend_fold_launch_shapes(self._h, C.byref(c), None), self._L)
        return {nb: int(c[nb]) for nb in range(1, FOLD_BATCH_MAX + 1) if c[nb]}

    def fold_launch_times(self):
        """{blocks per launch: (timed fold launches of that size, their kernel time in ms)} since reset_timers(True)."""
        c, ms = (C.c_int64 * (FOLD_BATCH_MAX + 1))(), (C.c_double * (FOLD_BATCH_MAX + 1))()
        _check(self._L.hfdl_gpu_frontend_fold_launch_shapes(self._h, C.byref(c), C.byref(ms)), self._L)
        return {nb: (int(c[nb]), float(ms[nb])) for nb in range(1, FOLD_BATCH_MAX + 1) if c[nb]}

    def stage_times(self):
        """{stage: (total ms, launches)} of the timed kernels since reset_timers(True): fft (per block), fold, ifft, demod, decode."""
        ms, n = (C.c_double * 5)(), (C.c_int64 * 5)()
        _check(self._L.hfdl_gpu_frontend_stage_times(self._h, C.byref(ms), C.byref(n)), self._L)
        return {k: (ms[i], int(n[i])) for i, k in enumerate(("fft", "fold", "ifft", "demod", "decode"))}

    def fold_variant_probe(self, variant, nb, reps=3):
        """Laboratory build: (avg ms, best ms, checksum of the partial sums) of `reps` launches of one compiled fold tiling on `nb` blocks
        (variant -1: the plain-VALU FMA-chain reference kernel)."""
        avg, best, chk = C.c_double(0), C.c_double(0), C.c_uint64(0)
        _check(self._L.hfdl_gpu_lab_fold_variant_probe(self._h, variant, nb, reps, C.byref(avg), C.byref(best), C.byref(chk)), self._L)
        return avg.value, best.value, chk.value

    def demod_time_ms(self):
        ms = C.c_double(0)
        n = C.c_int64(0)
        nb = C.c_int64(0)
        _check(self._L.hfdl_gpu_frontend_demod_time_ms(self._h, C.byref(ms), C.byref(n), C.byref(nb)), self._L)
        return ms.value, n.value, nb.value

    def step_period_ms(self):
        v = C.c_double(0)
        _check(self._L.hfdl_gpu_frontend_step_period_ms(self._h, C.byref(v)), self._L)
        return v.value

    def stream_read_probe(self):
        """Laboratory build: GB/s a bare read-only kernel reaches over the resident filter taps."""
        v = C.c_double(0)
        _check(self._L.hfdl_gpu_lab_stream_read_probe(self._h, C.byref(v)), self._L)
        return v.value

    def stream(self):
        return self._L.hfdl_gpu_frontend_stream(self._h)

    def _rx_center(self, rx):
        return self.centerfreq

    def spectrum_enable(self, bins, hann=False, maxhold=False):
        """Spectrum monitor (include/hfdl_gpu.h): `bins` band powers per receiver from every block's forward FFT, from the next block on;
        bins = 0 turns it off.  Calling it again starts every receiver's average over."""
        flags = (SPECTRUM_HANN if hann else 0) | (SPECTRUM_MAXHOLD if maxhold else 0)
        _check(self._L.hfdl_gpu_frontend_spectrum_enable(self._h, bins, flags), self._L)
        self._spec_bins, self._spec_peak = int(bins), bool(maxhold)
        self._spec_rows = 0                    # the library drops the history of interval rows with the old monitor

    def spectrum_band_centres(self, rx=0):
        """Centre frequencies in Hz (float64) of the monitor's bands of receiver rx: band b spans centre +- G fs / 2N with
        centre = centerfreq + (b G - N/2 - 0.5 + G/2) fs / N, G = N / bins."""
        g = self.geometry
        n, b = g.fft_size, self._spec_bins
        G = n // b
        return self._rx_center(rx) + (np.arange(b, dtype=np.float64) * G - n / 2 - 0.5 + G / 2) * (g.sample_rate / n)

    def spectrum_read(self, rx=0, reset=False):
        """dict(mean, peak (None without maxhold), blocks, first_block, freqs): linear band powers (float32; a full-scale tone = 1.0) of
        receiver rx averaged / max-held over the `blocks` blocks since its last reset, the first of them block `first_block`; freqs =
        the band centres in Hz.  Nothing accumulated yet: blocks = 0, mean (and peak) None.  Waits for the forward FFTs only."""
        b = self._spec_bins
        if not b:
            raise GpuError("the spectrum monitor is off: spectrum_enable() first")
        mean = np.zeros(b, np.float32)
        peak = np.zeros(b, np.float32) if self._spec_peak else None
        T, first = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.hfdl_gpu_frontend_spectrum_read(self._h, rx, _p(mean), _p(peak) if peak is not None else None, b,
                                                       C.byref(T), C.byref(first), int(reset)), self._L)
        if T.value == 0:
            mean, peak = None, None
        return dict(mean=mean, peak=peak, blocks=T.value, first_block=first.value, freqs=self.spectrum_band_centres(rx))

    def spectrum_history(self, rows, interval_blocks=0):
        """Keep the newest `rows` (2 .. SPECTRUM_ROWS_MAX) finished interval rows on the device; rows = 0 turns the history off.  A row =
        mean (and max-hold) over the blocks of one interval, closed by spectrum_row_close() or by itself after interval_blocks blocks.
        Rows are numbered from 0 at every call; spectrum_enable() drops the history."""
        _check(self._L.hfdl_gpu_frontend_spectrum_history(self._h, rows, interval_blocks), self._L)
        self._spec_rows = int(rows)

    def spectrum_row_close(self):
        """End the open row (host bookkeeping: no device call, no wait); returns its index.  An open row without a block stays open."""
        row = C.c_uint64(0)
        _check(self._L.hfdl_gpu_frontend_spectrum_row_close(self._h, C.byref(row)), self._L)
        return row.value

    def spectrum_rows(self, rx=0, from_row=0, max_rows=None, wait=False):
        """Finished rows of receiver rx from max(from_row, oldest kept) on: dict(mean [n][bins] float32, peak likewise (None without
        maxhold), row, first_block, blocks: [n] each, next_row: the from_row of the next call).  wait=False never waits for a kernel
        stream: only rows whose last launch has run; wait=True waits for every row closed so far.  A row is bit-identical to what
        spectrum_read(rx, reset=True) returns for the same blocks."""
        b = self._spec_bins
        if not b:
            raise GpuError("the spectrum monitor is off: spectrum_enable() first")
        cap = getattr(self, "_spec_rows", 0) if max_rows is None else int(max_rows)
        mean = np.zeros((max(cap, 0), b), np.float32)
        peak = np.zeros((max(cap, 0), b), np.float32) if self._spec_peak else None
        info = (SpectrumRow * max(cap, 1))()
        n, nxt = C.c_int32(0), C.c_uint64(0)
        _check(self._L.hfdl_gpu_frontend_spectrum_rows(self._h, rx, C.c_uint64(from_row), cap, _p(mean), _p(peak) if peak is not None else None,
                                                       info, C.byref(n), C.byref(nxt), int(wait)), self._L)
        k = n.value
        return dict(mean=mean[:k], peak=peak[:k] if peak is not None else None, row=[info[i].row for i in range(k)],
                    first_block=[info[i].first_block for i in range(k)], blocks=[info[i].blocks for i in range(k)], next_row=nxt.value)

    def export_enable(self, channels, fmt="cf32", scale=1.0, ring_blocks=64):
        """Channel baseband export (include/hfdl_gpu.h): from the next pushed block on, the device keeps the newest `ring_blocks`
        (2 .. EXPORT_RING_MAX) blocks of the channelizer's output of `channels` (distinct global indices; their order is the order of the
        exported rows).  fmt "cf32", or "cs16" = int16 of rint(v * scale).  No channels: off.  Calling it again starts over."""
        ch = np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
        f = {"cf32": EXPORT_CF32, "cs16": EXPORT_CS16}.get(fmt, fmt)
        _check(self._L.hfdl_gpu_frontend_export_enable(self._h, _p(ch) if len(ch) else None, len(ch), f, scale, ring_blocks), self._L)
        self._export = (len(ch), f, int(ring_blocks))

    def export_read(self, from_block=0, max_blocks=None, wait=False):
        """Finished blocks of the export from max(from_block, oldest kept) on: (samples [n, nsel, P] complex64 -- or int16 [n, nsel, P, 2]
        for cs16 --, counts [n, nsel] int32 valid samples of each row, power [n, nsel] float32, clipped [n, nsel] uint32, blocks [n]
        their indices, next_block: the from_block of the next call).  wait=False never waits for a kernel stream: only blocks whose
        launch has run; wait=True waits for the newest export launch queued and closes nothing (blocks of an open half come later)."""
        nsel, f, ring = getattr(self, "_export", (0, 0, 0))
        if not nsel:
            raise GpuError("the channel export is off: export_enable() first")
        cap = ring if max_blocks is None else int(max_blocks)
        k, P = max(cap, 0), self.geometry.max_outputs_per_block
        samples = np.zeros((k, nsel, P, 2), np.int16) if f == EXPORT_CS16 else np.zeros((k, nsel, P), np.complex64)
        counts, power, clipped = np.zeros((k, nsel), np.int32), np.zeros((k, nsel), np.float32), np.zeros((k, nsel), np.uint32)
        info = np.zeros(max(k, 1), np.uint64)
        n, nxt = C.c_int32(0), C.c_uint64(0)
        _check(self._L.hfdl_gpu_frontend_export_read(self._h, C.c_uint64(from_block), cap, _p(samples), _p(counts), _p(power), _p(clipped), _p(info),
                                                     C.byref(n), C.byref(nxt), int(wait)), self._L)
        m = n.value
        return samples[:m], counts[:m], power[:m], clipped[:m], [int(b) for b in info[:m]], nxt.value

    def retune(self, channel, freq_hz):
        """Move `channel` (a global index) to freq_hz (include/hfdl_gpu.h hfdl_gpu_frontend_retune_channel): blocks pushed before the
        call run on the old frequency, blocks pushed after it on the new one, where the channel starts as a freshly created one.  Nothing
        is drained.  A refusal raises GpuError with the library's text and changes nothing."""
        _check(self._L.hfdl_gpu_frontend_retune_channel(self._h, int(channel), int(freq_hz)), self._L)
        self.freqs[channel] = int(freq_hz)

    def quality_enable(self, ring_frames=4096, symbols=False):
        """Frame quality records (include/hfdl_gpu.h): from the next demodulator launch queued on, one record per finished frame in a
        ring of ring_frames (2 .. QUALITY_RING_MAX) records; symbols=True keeps each frame's data symbols too.  ring_frames = 0: off.
        Calling it again starts over with an empty ring."""
        _check(self._L.hfdl_gpu_frontend_quality_enable(self._h, int(ring_frames), QUALITY_SYMBOLS if symbols else 0), self._L)
        self._quality = (int(ring_frames), bool(symbols))

    def quality_read_raw(self, max_frames=None, wait=False, out=None):
        """The C structs as the library hands them over: (ctypes array of hfdl_gpu_frame_quality, symbols [max_frames, 5040] complex64 or
        None, count, dropped).  out = (array, symbols) of an earlier call: filled again instead of allocating (a caller that reads after
        every push)."""
        ring, with_sym = getattr(self, "_quality", (0, False))
        cap = ring if max_frames is None else int(max_frames)
        if out is None:
            out = ((FrameQuality * max(cap, 1))(), np.zeros((max(cap, 0), QUALITY_SYMBOLS_MAX), np.complex64) if with_sym else None)
        buf, sym = out
        n, dropped = C.c_int32(0), C.c_uint32(0)
        _check(self._L.hfdl_gpu_frontend_quality_read(self._h, buf, _p(sym) if sym is not None else None, cap, C.byref(n), C.byref(dropped), int(wait)), self._L)
        return buf, sym, n.value, dropped.value

    def quality_read(self, max_frames=None, wait=False):
        """(records as dicts, symbols [n, 5040] complex64 with zeros past nsym -- None unless enabled with symbols=True --, frames
        dropped since the enable).  wait=False never waits for a kernel stream: only records known to be complete; wait=True syncs
        first.  A record belongs to the PDU with the same (channel, sample_index)."""
        buf, sym, n, dropped = self.quality_read_raw(max_frames, wait)
        return [quality_to_dict(buf[i]) for i in range(n)], (sym[:n] if sym is not None else None), dropped

    def blanker_enable(self, threshold_db):
        """Wideband impulse-noise blanker (include/hfdl_gpu.h): from the next pushed block on, a new sample whose power exceeds
        10^(threshold_db / 10) times the mean power of its receiver's block enters the transform as zero.  6 .. 60 dB; 0 turns it off."""
        _check(self._L.hfdl_gpu_frontend_blanker_enable(self._h, float(threshold_db)), self._L)

    def blanker_stats(self, rx=0):
        """dict(blocks, samples_blanked, last_power, last_threshold) of receiver rx since the first blanker_enable(); waits for the
        forward FFTs' side of the pipeline only."""
        st = BlankerStats()
        _check(self._L.hfdl_gpu_frontend_blanker_stats(self._h, rx, C.byref(st)), self._L)
        return dict(blocks=st.blocks, samples_blanked=st.samples_blanked, last_power=np.float32(st.last_power), last_threshold=np.float32(st.last_threshold))

    def iqbal_enable(self, alpha, rx=-1):
        """Wideband I/Q imbalance and DC corrector (include/hfdl_gpu.h) of receiver rx (-1: every receiver): from the next pushed block on,
        a block enters the transform as d - kappa conj(d), d = x - m, with (kappa, m) estimated from the blocks before it; alpha 2^-10 .. 1
        is the weight of a block in the running averages, 0 turns it off."""
        _check(self._L.hfdl_gpu_frontend_iqbal_enable(self._h, rx, float(alpha)), self._L)

    def iqbal_seed(self, kappa, dc=0j, hold=False, rx=-1):
        """Presets (kappa, dc) of receiver rx (-1: every receiver) from its next pushed block; hold: keep them, estimate nothing."""
        kappa, dc = complex(kappa), complex(dc)
        _check(self._L.hfdl_gpu_frontend_iqbal_seed(self._h, rx, kappa.real, kappa.imag, dc.real, dc.imag, int(bool(hold))), self._L)

    def iqbal_stats(self, rx=0):
        """dict(blocks, refused, kappa, dc, power, image_rejection_db, valid, hold) of receiver rx's newest block; waits for the forward
        FFTs' side of the pipeline only."""
        st = IqbalStats()
        _check(self._L.hfdl_gpu_frontend_iqbal_stats(self._h, rx, C.byref(st)), self._L)
        return iqbal_stats_to_dict(st)

    def notch_enable(self, mu, channels=None):
        """Adaptive carrier canceller (include/hfdl_gpu.h) in front of the demodulator of `channels` (None: every channel), each from
        zero state, for the blocks pushed from now on.  mu 1e-5 .. 0.05; 0 turns it off."""
        sel = None if channels is None else np.ascontiguousarray(channels, dtype=np.int32)
        _check(self._L.hfdl_gpu_frontend_notch_enable(self._h, _p(sel) if sel is not None and len(sel) else None, 0 if sel is None else len(sel), float(mu)), self._L)

    def notch_stats(self, channel):
        """dict(blocks, resets, last_in_power, last_out_power, tap_energy) of a selected channel since notch_enable(); waits for the
        canceller launches queued so far only."""
        st = NotchStats()
        _check(self._L.hfdl_gpu_frontend_notch_stats(self._h, channel, C.byref(st)), self._L)
        return dict(blocks=st.blocks, resets=st.resets, last_in_power=np.float32(st.last_in_power), last_out_power=np.float32(st.last_out_power),
                    tap_energy=np.float32(st.tap_energy))

    @staticmethod
    def notch_rows(x, mu, state=None, device=0):
        """The canceller alone (module-level notch_rows)."""
        return notch_rows(x, mu, state, device)

    def real_input(self):
        """(is_real, sample_rate_real) as the library reports them (hfdl_gpu_frontend_real_input; (False, 0) for a complex front end)."""
        a, b = C.c_int32(-1), C.c_int32(-1)
        _check(self._L.hfdl_gpu_frontend_real_input(self._h, C.byref(a), C.byref(b)), self._L)
        return bool(a.value), b.value

    def close(self):
        if self._h:
            self._L.hfdl_gpu_frontend_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiFrontend(Frontend):
    """Several receivers' I/Q streams at one sample rate in ONE front end (hfdl_gpu_frontend_create_multi): receivers =
    [(centerfreq, [freqs...]), ...].  Channel indices are global, receiver-major (receiver 0's channels first); every step takes a
    block of every receiver (push_blocks / push_blocks_raw).  Polls, stats, taps, timers and the lab probe are Frontend's."""

    def __init__(self, sample_rate, receivers, device=0, lib=None):
        L = self._L = lib or load()
        self.receivers = [(int(c), [int(f) for f in fs]) for c, fs in receivers]
        centres = np.ascontiguousarray([c for c, _ in self.receivers], dtype=np.int32)
        counts = np.ascontiguousarray([len(fs) for _, fs in self.receivers], dtype=np.int32)
        fr = np.ascontiguousarray([f for _, fs in self.receivers for f in fs], dtype=np.int32)
        self._h = C.c_void_p()
        _check(L.hfdl_gpu_frontend_create_multi(C.byref(self._h), device, sample_rate, len(self.receivers), _p(centres), _p(fr), _p(counts)), L)
        self.geometry = Geometry()
        _check(L.hfdl_gpu_frontend_geometry(self._h, C.byref(self.geometry)), L)
        self.freqs = [int(f) for f in fr]
        self._spec_bins, self._spec_peak = 0, False
        self._rx_of = [r for r, (_, fs) in enumerate(self.receivers) for _ in fs]

    @property
    def nrx(self):
        return len(self.receivers)

    def _rx_center(self, rx):
        return self.receivers[rx][0]

    def receiver_of(self, channel):
        """(receiver index, its centre frequency) of a global channel index."""
        rx, cf = C.c_int32(0), C.c_int32(0)
        _check(self._L.hfdl_gpu_frontend_channel_receiver(self._h, channel, C.byref(rx), C.byref(cf)), self._L)
        return rx.value, cf.value

    def push_blocks_raw(self, blocks, sample_format, on_device=False, nsamples=None):
        """blocks[r]: receiver r's block -- an int16 / uint8 / float32 numpy array of 2*input_size interleaved I,Q values, or (on_device)
        an int device pointer (nsamples: input_size unless given).  One call = one step = one host block."""
        dt = {SFMT_CF32: np.float32, SFMT_CS16: np.int16, SFMT_CU8: np.uint8}[sample_format]
        keep = []
        ptrs = (C.c_void_p * max(1, len(blocks)))()
        for r, b in enumerate(blocks):
            if isinstance(b, int):
                ptrs[r] = b
            else:
                a = np.ascontiguousarray(b, dtype=dt)
                keep.append(a)
                ptrs[r] = a.ctypes.data
        if keep:
            lens = {len(a) // 2 for a in keep}
            if len(lens) != 1:
                raise ValueError("the receivers' blocks differ in length: %s" % sorted(lens))
            nsamples = lens.pop() if nsamples is None else nsamples
        n = self.geometry.input_size if nsamples is None else nsamples
        _check(self._L.hfdl_gpu_frontend_push_blocks_raw(self._h, ptrs, n, sample_format, int(on_device)), self._L)

    def push_blocks(self, blocks):
        """blocks[r]: complex64 numpy array of input_size samples of receiver r (host), or an int device pointer to one; all of one kind."""
        dev = all(isinstance(b, int) for b in blocks) and len(blocks) > 0
        if dev:
            self.push_blocks_raw(list(blocks), SFMT_CF32, on_device=True)
        else:
            self.push_blocks_raw([np.ascontiguousarray(b, dtype=np.complex64).view(np.float32) for b in blocks], SFMT_CF32)

    def pdus_to_dicts(self, buf, n):
        out = Frontend.pdus_to_dicts(buf, n)
        for d in out:
            d["receiver"] = self._rx_of[d["channel"]]
        return out


class RealFrontend(MultiFrontend):
    """Receivers that deliver REAL samples (direct sampling) at sample_rate_real in one front end (hfdl_gpu_frontend_create_real):
    receivers = [(base_freq, [freqs...]), ...], base_freq the RF frequency at 0 Hz of the samples.  The front end is MultiFrontend's for
    the equivalent complex stream -- geometry.sample_rate = sample_rate_real / 2, receiver centres base + sample_rate_real / 4 --
    and takes blocks of 2 * input_size real samples as SFMT_RS16 / SFMT_RF32 (push_real)."""

    def __init__(self, sample_rate_real, receivers, device=0, lib=None):
        L = self._L = lib or load()
        self.sample_rate_real = int(sample_rate_real)
        self.bases = [int(b) for b, _ in receivers]
        self.receivers = [(int(b) + self.sample_rate_real // 4, [int(f) for f in fs]) for b, fs in receivers]
        bases = np.ascontiguousarray(self.bases, dtype=np.int32)
        counts = np.ascontiguousarray([len(fs) for _, fs in self.receivers], dtype=np.int32)
        fr = np.ascontiguousarray([f for _, fs in self.receivers for f in fs], dtype=np.int32)
        self._h = C.c_void_p()
        _check(L.hfdl_gpu_frontend_create_real(C.byref(self._h), device, self.sample_rate_real, len(self.receivers), _p(bases), _p(fr), _p(counts)), L)
        self.geometry = Geometry()
        _check(L.hfdl_gpu_frontend_geometry(self._h, C.byref(self.geometry)), L)
        self.freqs = [int(f) for f in fr]
        self._spec_bins, self._spec_peak = 0, False
        self._rx_of = [r for r, (_, fs) in enumerate(self.receivers) for _ in fs]

    @property
    def real_block(self):
        """real samples of one block of one receiver"""
        return 2 * self.geometry.input_size

    def push_real(self, blocks, sample_format=SFMT_RS16, on_device=False):
        """blocks[r]: receiver r's 2 * input_size real samples -- an int16 (SFMT_RS16) / float32 (SFMT_RF32) numpy array, or (on_device)
        an int device pointer.  One call = one step."""
        dt = {SFMT_RS16: np.int16, SFMT_RF32: np.float32}[sample_format]
        keep = [b if isinstance(b, int) else np.ascontiguousarray(b, dtype=dt) for b in blocks]
        ptrs = (C.c_void_p * max(1, len(keep)))(*[b if isinstance(b, int) else b.ctypes.data for b in keep])
        lens = {len(b) for b in keep if not isinstance(b, int)} or {self.real_block}
        if len(lens) != 1:
            raise ValueError("the receivers' blocks differ in length: %s" % sorted(lens))
        _check(self._L.hfdl_gpu_frontend_push_blocks_raw(self._h, ptrs, lens.pop(), sample_format, int(on_device)), self._L)


BLANK_CHUNK = 4096         # samples per workgroup of the blanker's block power (dumphfdl_amd/csrc/blanker.h)


def blank_sum_depth(n):
    """fp32 additions on the longest path of the blanker's block power over n samples (blanker.h blank_sum_depth): 8 + 1 of a thread
    and 6 + 2 of the tree per chunk of 4096 samples, then ceil(chunks / 256) of a thread and 6 + 2 of the tree over the chunk sums."""
    chunks = -(-int(n) // BLANK_CHUNK)
    return 9 + 8 + -(-chunks // 256) + 8


def blank_block(raw, sample_format, threshold_db, device=0):
    """The blanker alone (hfdl_gpu_blank_block) on one block: raw = float32 / int16 / uint8 numpy array of 2 n interleaved I, Q values
    (a complex64 array for SFMT_CF32 will do).  Returns (out: n complex64 as they would enter the transform, P: float32, blanked)."""
    dt = {SFMT_CF32: np.float32, SFMT_CS16: np.int16, SFMT_CU8: np.uint8}[sample_format]
    r = np.asarray(raw)
    if sample_format == SFMT_CF32 and r.dtype == np.complex64:
        r = np.ascontiguousarray(r).view(np.float32)
    r = np.ascontiguousarray(r, dtype=dt)
    n = len(r) // 2
    out = np.zeros(n, np.complex64)
    power, blanked = C.c_float(0), C.c_uint64(0)
    _check(load().hfdl_gpu_blank_block(device, _p(r) if n else None, n, sample_format, float(threshold_db), _p(out) if n else None, C.byref(power), C.byref(blanked)))
    return out, np.float32(power.value), blanked.value


IQBAL_BLOCKS_MAX = 64      # blocks of one iqbal_blocks() call (dumphfdl_amd/csrc/iqbal.h)


def iqbal_stats_to_dict(st):
    return dict(blocks=st.blocks, refused=st.refused, kappa=np.complex64(complex(st.kappa_re, st.kappa_im)), dc=np.complex64(complex(st.dc_re, st.dc_im)),
                power=np.float32(st.power), image_rejection_db=np.float32(st.image_rejection_db), valid=bool(st.valid), hold=bool(st.hold))


def iqbal_blocks(raw, n, sample_format, alpha, seed=None, hold=False, device=0):
    """The I/Q corrector alone (hfdl_gpu_iqbal_blocks) on consecutive blocks of n samples of one receiver, from a fresh enable: raw =
    float32 / int16 / uint8 numpy array of 2 n nblocks interleaved I, Q values (a complex64 array for SFMT_CF32 will do); seed = None or
    (kappa, dc).  Returns (out: nblocks * n complex64 as they would enter the transform, records: the IqbalStats array, one per block)."""
    dt = {SFMT_CF32: np.float32, SFMT_CS16: np.int16, SFMT_CU8: np.uint8}[sample_format]
    r = np.asarray(raw)
    if sample_format == SFMT_CF32 and r.dtype == np.complex64:
        r = np.ascontiguousarray(r).view(np.float32)
    r = np.ascontiguousarray(r, dtype=dt)
    n = int(n)
    nblocks = len(r) // (2 * n) if n > 0 else 0
    out = np.zeros(max(nblocks, 0) * max(n, 0), np.complex64)
    recs = (IqbalStats * max(nblocks, 1))()
    sd = None if seed is None else np.array([complex(seed[0]).real, complex(seed[0]).imag, complex(seed[1]).real, complex(seed[1]).imag], np.float32)
    _check(load().hfdl_gpu_iqbal_blocks(device, _p(r) if r.size else None, n, nblocks, sample_format, float(alpha), _p(sd) if sd is not None else None,
                                        int(bool(hold)), _p(out) if out.size else None, C.cast(recs, C.c_void_p)))
    return out, recs


NOTCH_STATE_FLOATS = 174   # HFDL_GPU_NOTCH_STATE_FLOATS: 32 taps (re, im), then the last 55 inputs (re, im), newest first


def notch_rows(x, mu, state=None, device=0):
    """The carrier canceller alone (hfdl_gpu_notch_rows): x = [nch][n] complex64, every row a channel's next n samples; state =
    [nch][NOTCH_STATE_FLOATS] float32 carried from an earlier call, or None for fresh channels.  Returns (y [nch][n] complex64, the
    state after the rows)."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    if x.ndim == 1:
        x = x[None, :]
    nch, n = x.shape
    st = np.zeros((nch, NOTCH_STATE_FLOATS), np.float32) if state is None else np.array(state, dtype=np.float32, order="C").reshape(nch, NOTCH_STATE_FLOATS)
    y = np.zeros((nch, n), np.complex64)
    _check(load().hfdl_gpu_notch_rows(device, _p(x) if x.size else None, nch, n, float(mu), _p(st), _p(y) if y.size else None))
    return y, st


def fft_forward(x, shifted=False, device=0):
    x = np.ascontiguousarray(x, dtype=np.complex64)
    out = np.empty_like(x)
    _check(load().hfdl_gpu_fft_forward(device, _p(x), _p(out), len(x), int(shifted)))
    return out


def viterbi27(soft, nbits, device=0):
    """soft: uint8 array [nframes, 2*nbits] -> uint8 [nframes, ceil(nbits/8)] (libfec bit order)."""
    soft = np.ascontiguousarray(soft, dtype=np.uint8).reshape(-1, 2 * nbits)
    out = np.zeros((soft.shape[0], (nbits + 7) // 8), np.uint8)
    _check(load().hfdl_gpu_viterbi27(device, _p(soft), nbits, soft.shape[0], _p(out)))
    return out


def burst_decode(symbol_list, modes, bitmask_lsb=None, device=0):
    """decode_user_data for a batch of frames; symbol_list[i] = the segments*30 equalised data symbols of frame i."""
    n = len(symbol_list)
    modes = np.ascontiguousarray(modes, dtype=np.int32)
    bm = np.zeros(n, np.int32) if bitmask_lsb is None else np.ascontiguousarray(bitmask_lsb, dtype=np.int32)
    sym = np.ascontiguousarray(np.concatenate([np.asarray(s, np.complex64) for s in symbol_list]), dtype=np.complex64)
    octets = np.zeros((n, PDU_MAX_OCTETS), np.uint8)
    lens = np.zeros(n, np.int32)
    _check(load().hfdl_gpu_burst_decode(device, _p(sym), _p(modes), _p(bm), n, _p(octets), _p(lens)))
    return [bytes(octets[i, :lens[i]]) for i in range(n)]


def quality_to_dict(q):
    """A hfdl_gpu_frame_quality as a dict; seg_err_power as a float32 array of `segments` entries, `raw` = the struct's 744 bytes."""
    d = {k: getattr(q, k) for k, _ in FrameQuality._fields_ if k != "seg_err_power"}
    d["seg_err_power"] = np.frombuffer(bytes(q), np.float32, QUALITY_SEGMENTS_MAX, FrameQuality.seg_err_power.offset).copy()
    d["raw"] = bytes(q)
    return d


def frame_quality(symbol_list, modes, device=0):
    """The frame quality figures of a batch of frames by the device function of the front end's records (hfdl_gpu_frame_quality_batch);
    symbol_list[i] = the segments*30 equalised data symbols of frame i.  One dict per frame."""
    n = len(symbol_list)
    modes = np.ascontiguousarray(modes, dtype=np.int32)
    sym = np.ascontiguousarray(np.concatenate([np.asarray(s, np.complex64) for s in symbol_list]), dtype=np.complex64)
    out = (FrameQuality * n)()
    _check(load().hfdl_gpu_frame_quality_batch(device, _p(sym), _p(modes), n, out))
    return [quality_to_dict(out[i]) for i in range(n)]


def lab_burst_soft(symbol_list, modes, bitmask_lsb=None, device=0):
    """burst_decode's frames stopped in front of the Viterbi decoder (laboratory build): the soft bytes it is fed, one uint8 array per frame."""
    L = load_lab()
    n = len(symbol_list)
    modes = np.ascontiguousarray(modes, dtype=np.int32)
    bm = np.zeros(n, np.int32) if bitmask_lsb is None else np.ascontiguousarray(bitmask_lsb, dtype=np.int32)
    sym = np.ascontiguousarray(np.concatenate([np.asarray(s, np.complex64) for s in symbol_list]), dtype=np.complex64)
    vin = np.zeros((n, LAB_VIN_MAX), np.uint8)
    lens = np.zeros(n, np.int32)
    _check(L.hfdl_gpu_lab_burst_soft(device, _p(sym), _p(modes), _p(bm), n, _p(vin), _p(lens)), L)
    return [vin[i, :lens[i]].copy() for i in range(n)]


def last_stage_ms():
    return load().hfdl_gpu_last_stage_ms()


def nco_decimate(x, rate, decimation, decimation_remain=0, starting_phase=0.0, device=0):
    """decimating_shift_addition_cc on the device; returns (out, decimation_remain, starting_phase) -- feed the state back in."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    out = np.zeros((len(x) + decimation - 1) // decimation, np.complex64)
    rem, ph, n = C.c_int32(decimation_remain), C.c_float(starting_phase), C.c_int32(0)
    _check(load().hfdl_gpu_nco_decimate(device, _p(x), len(x), rate, decimation, C.byref(rem), C.byref(ph), _p(out), C.byref(n)))
    return out[:n.value].copy(), rem.value, ph.value


def crc16_ccitt(data, crc_init=0xFFFF, device=0):
    a = np.frombuffer(bytes(data), np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    crc = C.c_uint16(0)
    _check(load().hfdl_gpu_crc16_ccitt(device, _p(a), len(data), crc_init, C.byref(crc)))
    return crc.value


def pdu_triage(pdus, device=0):
    """pdus: list of bytes -> list of (fcs_status, pdu_kind, hdr_len) computed on the device."""
    n = len(pdus)
    stride = max(len(p) for p in pdus)
    octets = np.zeros((n, stride), np.uint8)
    for i, p in enumerate(pdus):
        octets[i, :len(p)] = np.frombuffer(bytes(p), np.uint8)
    lens = np.array([len(p) for p in pdus], np.int32)
    fcs, kind, hl = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint16)
    _check(load().hfdl_gpu_pdu_triage(device, _p(octets), _p(lens), n, stride, _p(fcs), _p(kind), _p(hl)))
    return [(int(fcs[i]), int(kind[i]), int(hl[i])) for i in range(n)]


def lpdu_walk(pdus, device=0):
    """pdus: list of bytes -> list of (processed, good, bad_fcs, too_short, truncated) computed on the device."""
    n = len(pdus)
    stride = max(len(p) for p in pdus)
    octets = np.zeros((n, stride), np.uint8)
    for i, p in enumerate(pdus):
        octets[i, :len(p)] = np.frombuffer(bytes(p), np.uint8)
    lens = np.array([len(p) for p in pdus], np.int32)
    counts = np.zeros((n, 5), np.uint8)
    _check(load().hfdl_gpu_lpdu_walk(device, _p(octets), _p(lens), n, stride, _p(counts)))
    return [tuple(int(v) for v in counts[i]) for i in range(n)]


def psk_slice(arity, symbols, device=0):
    """symbols: complex64 array -> (Gray-coded decisions uint32, phase errors float32) from the carrier loop's slicer."""
    x = np.ascontiguousarray(symbols, dtype=np.complex64)
    sym = np.zeros(len(x), np.uint32)
    err = np.zeros(len(x), np.float32)
    _check(load().hfdl_gpu_psk_slice(device, arity, _p(x), len(x), _p(sym), _p(err)))
    return sym, err
