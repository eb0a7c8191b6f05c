"""ctypes binding of include/habdec_amd.h and include/habdec_amd_host.h (1:1, no logic)."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "libhabdec_amd.so"
_lib = None


class HabdecError(RuntimeError):
    pass


class hd_engine_config(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_streams", C.c_uint32), ("max_chunk", C.c_uint32), ("sampling_rate", C.c_double),
                ("decimation", C.c_uint32), ("baud", C.c_double), ("rtty_bits", C.c_uint32), ("rtty_stops", C.c_float),
                ("lowpass_bw_hz", C.c_float), ("lowpass_trans", C.c_float), ("dc_remove", C.c_int32), ("lookup_mode", C.c_int32),
                ("enable_spectrum", C.c_int32), ("ungated", C.c_int32), ("keep_filtered", C.c_int32), ("pipeline", C.c_int32), ("arith", C.c_int32)]


class hd_afc_info(C.Structure):
    _fields_ = [("frequency_correction", C.c_double), ("shift_hz", C.c_double), ("noise_floor", C.c_double),
                ("noise_variance", C.c_double), ("peak_left", C.c_int32), ("peak_right", C.c_int32), ("spectra", C.c_uint64)]


class hd_timing(C.Structure):
    _fields_ = [("ms_total", C.c_double), ("ms_front", C.c_double), ("front_bytes", C.c_uint64), ("samples", C.c_uint64),
                ("host_enqueue_us", C.c_double), ("host_wait_us", C.c_double), ("host_text_us", C.c_double), ("timed_calls", C.c_uint64),
                ("path", C.c_uint32), ("step_variant", C.c_uint32), ("host_calls_in_place", C.c_uint64), ("lowpass_fft_calls", C.c_uint64)]


class hd_tune_info(C.Structure):
    _fields_ = [("offset_hz", C.c_double), ("step", C.c_uint32), ("phase", C.c_uint32), ("retunes", C.c_uint64), ("from_call", C.c_uint64),
                ("auto_afc", C.c_int32)]


class hd_front_tune_info(C.Structure):
    _fields_ = [("offset_hz", C.c_double), ("step", C.c_uint32), ("phase", C.c_uint32), ("from_call", C.c_uint64)]


class hd_survey_params(C.Structure):
    _fields_ = [("threshold_db", C.c_double), ("merge_hz", C.c_double), ("dc_guard_hz", C.c_double), ("max_width_hz", C.c_double)]


class hd_survey_candidate(C.Structure):
    _fields_ = [("offset_hz", C.c_double), ("snr_db", C.c_double), ("width_hz", C.c_double), ("bin_lo", C.c_uint32), ("bin_hi", C.c_uint32)]


WATERFALL_WORDS, WF_SHORT, WF_BAD, WF_NO_FLOOR = 128, 1, 2, 4


class hd_waterfall_params(C.Structure):
    _fields_ = [("slot_segments", C.c_uint32), ("rows_cap", C.c_uint32), ("threshold_db", C.c_double), ("dc_guard_hz", C.c_double)]


class hd_waterfall_row(C.Structure):
    _fields_ = [("first_sample", C.c_uint64), ("segments", C.c_uint32), ("flags", C.c_uint32), ("floor", C.c_float), ("level", C.c_float),
                ("n_marked", C.c_uint32), ("_pad", C.c_uint32)]


# one hd_waterfall_row
WATERFALL_ROW_DTYPE = np.dtype([("first_sample", "<u8"), ("segments", "<u4"), ("flags", "<u4"), ("floor", "<f4"), ("level", "<f4"), ("n_marked", "<u4"),
                                ("_pad", "<u4")])


class hd_waterfall_track_params(C.Structure):
    _fields_ = [("merge_hz", C.c_double), ("max_width_hz", C.c_double), ("gap_rows", C.c_uint32), ("min_rows", C.c_uint32)]


class hd_waterfall_track(C.Structure):
    _fields_ = [("first_sample", C.c_uint64), ("end_sample", C.c_uint64), ("first_row", C.c_uint64), ("last_row", C.c_uint64), ("marks", C.c_uint64),
                ("offset_hz", C.c_double), ("width_hz", C.c_double), ("rows_hit", C.c_uint32), ("bin_lo", C.c_uint32), ("bin_hi", C.c_uint32),
                ("open", C.c_int32)]


PROBE_CANDIDATES, PROBE_SCALES, TRIAL_FORMATS = 1024, 9, 4
PROBE_WINDOWS = (1, 3, 7, 15, 31, 63, 127, 255, 511)


class hd_baud_probe_params(C.Structure):
    _fields_ = [("baud_lo", C.c_double), ("baud_hi", C.c_double), ("min_coherence", C.c_double)]


class hd_baud_estimate(C.Structure):
    _fields_ = [("baud", C.c_double), ("nominal", C.c_double), ("rho", C.c_double), ("rho_max", C.c_double), ("samples", C.c_uint64),
                ("edges", C.c_uint64), ("k", C.c_uint32), ("settled", C.c_int32), ("valid", C.c_int32), ("_pad", C.c_uint32)]


class hd_baud_probe_stream_state(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("edges", C.c_uint64 * PROBE_SCALES), ("history", C.c_uint64 * 8), ("majority", C.c_uint32 * PROBE_SCALES),
                ("n_candidates", C.c_uint32)]


# one hd_baud_probe_candidate
PROBE_CANDIDATE_DTYPE = np.dtype([("P", "<u8"), ("Q", "<u8"), ("NB", "<u4"), ("re", "<i4"), ("im", "<i4"), ("n", "<u4"), ("cur_block", "<u4"), ("_pad", "<u4")])


class hd_format_trial_result(C.Structure):
    _fields_ = [("best", C.c_int32), ("best_bits", C.c_uint32), ("best_stops", C.c_float), ("bits", C.c_uint32 * TRIAL_FORMATS),
                ("stops", C.c_float * TRIAL_FORMATS), ("_pad", C.c_uint32), ("sentences_ok", C.c_uint64 * TRIAL_FORMATS),
                ("matches", C.c_uint64 * TRIAL_FORMATS), ("printable", C.c_uint64 * TRIAL_FORMATS)]


class hd_clocked_params(C.Structure):
    _fields_ = [("record_cap", C.c_uint32), ("repair_bits", C.c_uint32), ("repair_flips", C.c_uint32), ("_pad", C.c_uint32)]


class hd_clocked_counters(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("samples", "cursor", "characters", "rejects", "dropped", "matches_failed", "sentences_plain", "sentences_repaired")]


# one hd_clocked_record, one hd_clocked_sentence
CLOCKED_RECORD_DTYPE = np.dtype([("pos", "<u8"), ("data", "<i4", (8,)), ("start", "<i4"), ("stop", "<i4"), ("stop2", "<i4"), ("ch", "<u4")])
CLOCKED_SENTENCE_DTYPE = np.dtype([("pos", "<u8"), ("flips", "<u4"), ("len", "<u4"), ("text", "S496")])
CLOCKED_MAX_SPB, CLOCKED_RING, CLOCKED_CHUNK = 2048, 32768, 4096


class hd_tones_params(C.Structure):
    _fields_ = [("max_push", C.c_uint32), ("window_q8", C.c_uint32)]


class hd_tones_info(C.Structure):
    _fields_ = [("samples", C.c_uint64)] + [(k, C.c_uint32) for k in ("F", "full", "W", "L", "step_hi", "step_lo")]


TONES_MAX_SPB, TONES_CHUNK = 2048, 4096


class hd_tone_search_params(C.Structure):
    _fields_ = [("max_push", C.c_uint32), ("_pad", C.c_uint32)]


class hd_tone_search_info(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("segments", C.c_uint64), ("carry", C.c_uint32), ("_pad", C.c_uint32)]


class hd_tone_search_detect_params(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("baud", "shift_lo_hz", "shift_hi_hz", "min_quality")]


class hd_tone_search_result(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("f_hi_hz", "f_lo_hz", "quality", "floor")] + [("segments", C.c_uint64)] + \
        [(k, C.c_uint32) for k in ("bin_lo", "shift_bins", "w", "valid")]


TONE_SEARCH_BINS, TONE_SEARCH_HOP, TONE_SEARCH_CHUNK = 4096, 2048, 65536


class hd_combine_params(C.Structure):
    _fields_ = [("max_push", C.c_uint32), ("_pad", C.c_uint32)]


class hd_combine_lag_params(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("window", "max_lag", "guard", "min_peak_q8", "min_margin_q8")]


class hd_combine_info(C.Structure):
    _fields_ = [("samples", C.c_uint64)] + [(k, C.c_uint32) for k in ("group", "delay", "weight", "members")]


# one hd_combine_lag
COMBINE_LAG_DTYPE = np.dtype([("stream", "<u4"), ("lag", "<i4"), ("peak", "<i4"), ("second", "<i4"), ("valid", "<u4")])
COMBINE_MAX_MEMBERS, COMBINE_MAX_DELAY, COMBINE_RING, COMBINE_CHUNK, COMBINE_MAX_LAG, COMBINE_NO_GROUP = 8, 8192, 32768, 4096, 4096, 0xFFFFFFFF


class hd_ssdv_params(C.Structure):
    _fields_ = [("max_fill", C.c_uint32), ("_pad", C.c_uint32)]


class hd_ssdv_counters(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("bytes", "decided", "fillers", "crc_bad", "overlaps")] + [("packets", C.c_uint64 * 5)]


# one hd_ssdv_packet
SSDV_PACKET_DTYPE = np.dtype([("pos", "<u8")] + [(k, "<u4") for k in ("trial", "errors", "erasures", "erasures_changed", "type", "image_id", "packet_id", "width",
                                                                      "height", "flags", "mcu_offset", "mcu_index")] + [("callsign", "S8"), ("data", "u1", (256,))])
SSDV_NOFEC, SSDV_TYPE_NOFEC, SSDV_RING, SSDV_LAUNCH = 255, 0x67, 4096, 16384


class hd_fsk4_frame(C.Structure):
    _fields_ = [("payload_bytes", C.c_uint32), ("uw", C.c_uint8 * 2), ("_pad", C.c_uint16), ("interleave_mul", C.c_uint32), ("scrambler_seed", C.c_uint32),
                ("golay_poly", C.c_uint32)]


class hd_fsk4_params(C.Structure):
    _fields_ = [("max_push", C.c_uint32), ("window_q8", C.c_uint32), ("uw_max_errors", C.c_uint32), ("chase_bits", C.c_uint32), ("max_corrected", C.c_int32),
                ("_pad", C.c_uint32)]


class hd_fsk4_counters(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("samples", "slots", "candidates", "gate_passes", "crc_failures", "refused", "overlaps", "frames")] + \
        [("F", C.c_uint32), ("W", C.c_uint32), ("step", C.c_uint32 * 4), ("symbols", C.c_uint32), ("codewords", C.c_uint32)]


# one hd_fsk4_rx, one hd_fsk4_candidate
FSK4_RX_DTYPE = np.dtype([("slot", "<u8"), ("start_sample", "<u8"), ("metric", "<u8"), ("payload_bytes", "<u4"), ("corrected", "<u4"), ("phase", "<u4"),
                          ("uw_errors", "<u4"), ("payload", "u1", (32,))])
FSK4_CANDIDATE_DTYPE = np.dtype([("slot", "<u8"), ("metric", "<u8"), ("crc_ok", "<u4"), ("corrected", "<u4"), ("uw_errors", "<u4"), ("_pad", "<u4"),
                                 ("payload", "u1", (32,))])
FSK4_MAX_SPB, FSK4_CHUNK, FSK4_LAUNCH, FSK4_HORUS_V1, FSK4_HORUS_V2 = 2048, 4096, 16384, 1, 2


class hd_fsk4_retune_info(C.Structure):
    _fields_ = [("retunes", C.c_uint64), ("late", C.c_uint64), ("waiting", C.c_uint64), ("psi", C.c_uint32 * 4)]


class hd_fsk4_track_params(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("max_push", "epoch_segments", "decay_q8", "min_quality_q8", "min_segments", "deadband")]


class hd_fsk4_comb_params(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("baud", "spacing_lo_hz", "spacing_hi_hz", "f_lo_hz", "f_hi_hz")] + [("min_quality_q8", C.c_uint32), ("segments_ok", C.c_uint32)]


class hd_fsk4_track_info(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("samples", "segments", "epochs", "valid_epochs", "retunes")]


# one hd_fsk4_comb_record, one hd_fsk4_track_est
FSK4_COMB_RECORD_DTYPE = np.dtype([("f0_q8", "<i4"), ("spacing_q8", "<i4"), ("c0", "<u4"), ("d", "<u4"), ("w", "<u4"), ("floor", "<u4"), ("score", "<u4"),
                                   ("quality_q8", "<u4"), ("valid", "<u4"), ("centroid_q8", "<i4", (4,)), ("_pad", "<u4", (3,))])
FSK4_TRACK_EST_DTYPE = np.dtype([("rec", FSK4_COMB_RECORD_DTYPE), ("f0_hz", "<f8"), ("spacing_hz", "<f8"), ("end_sample", "<u8"), ("epoch", "<u8")])
assert FSK4_COMB_RECORD_DTYPE.itemsize == 64 and FSK4_TRACK_EST_DTYPE.itemsize == 96


class hd_afsk_params(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("max_push", "max_frame_bytes", "repair_bits", "repair_flips", "require_addr", "_pad")]


class hd_afsk_counters(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("samples", "slots", "flags", "unshaped", "fcs_failures", "frames_plain", "frames_repaired", "refused", "overlaps")] + \
        [("F", C.c_uint32), ("W", C.c_uint32), ("step", C.c_uint32 * 2)]


# one hd_afsk_rx, one hd_afsk_candidate
AFSK_MAX_SPB, AFSK_CHUNK, AFSK_LAUNCH, AFSK_RING, AFSK_MAX_FRAME, AFSK_MIN_FRAME = 2048, 4096, 4096, 65536, 332, 17
AFSK_OPEN, AFSK_ABORT, AFSK_UNSHAPED, AFSK_FCS_FAILED, AFSK_REFUSED, AFSK_PLAIN, AFSK_REPAIRED = range(7)
AFSK_RX_DTYPE = np.dtype([("slot", "<u8"), ("start_sample", "<u8"), ("close_slot", "<u8"), ("metric", "<u8"), ("len", "<u4"), ("flips", "<u4"), ("phase", "<u4"),
                          ("addr_ok", "<u4"), ("fcs", "<u4"), ("_pad", "<u4"), ("data", "u1", (AFSK_MAX_FRAME,)), ("_pad2", "<u4")])
AFSK_CANDIDATE_DTYPE = np.dtype([("slot", "<u8"), ("close_slot", "<u8"), ("metric", "<u8"), ("result", "<u4"), ("bits", "<u4"), ("len", "<u4"), ("flips", "<u4"),
                                 ("addr_ok", "<u4"), ("fcs", "<u4"), ("data", "u1", (AFSK_MAX_FRAME,)), ("_pad", "<u4")])
assert AFSK_RX_DTYPE.itemsize == 392 and AFSK_CANDIDATE_DTYPE.itemsize == 384


# IQ sample formats (HD_IQ_*): what the *_fmt calls take; numpy dtype of one component, bytes per complex sample
IQ_CF32, IQ_CS16, IQ_CS8, IQ_CU8 = 0, 1, 2, 3
IQ_DTYPES = {IQ_CF32: np.dtype(np.float32), IQ_CS16: np.dtype("<i2"), IQ_CS8: np.dtype(np.int8), IQ_CU8: np.dtype(np.uint8)}
IQ_NAMES = {"cf32": IQ_CF32, "cs16": IQ_CS16, "cs8": IQ_CS8, "cu8": IQ_CU8}


def iq_fmt(fmt) -> int:
    """'cs16' / 'cs8' / 'cu8' / 'cf32' or an HD_IQ_* number -> the number (unknown numbers pass through: the library refuses them)."""
    return IQ_NAMES[fmt] if isinstance(fmt, str) else int(fmt)


SENTENCE_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p)
MATCH_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int)
CHARS_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.POINTER(C.c_char), C.c_size_t)

_vp, _u32, _sz, _dbl, _int, _f = C.c_void_p, C.c_uint32, C.c_size_t, C.c_double, C.c_int, C.c_float
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")

# name -> (restype, argtypes): every symbol declared in include/habdec_amd.h
ENGINE_API = {
    "hd_engine_config_default": (None, [C.POINTER(hd_engine_config)]),
    "hd_engine_create": (_int, [C.POINTER(hd_engine_config), C.POINTER(_vp)]),
    "hd_engine_destroy": (None, [_vp]),
    "hd_pinned_alloc": (_vp, [_sz]),
    "hd_pinned_free": (None, [_vp]),
    "hd_last_error": (C.c_char_p, []),
    "hd_engine_streams": (_u32, [_vp]),
    "hd_engine_decimation": (_u32, [_vp]),
    "hd_engine_decimated_rate": (_dbl, [_vp]),
    "hd_engine_lowpass_taps_max": (_u32, [_vp]),
    "hd_stream_set_baud": (_int, [_vp, _u32, _dbl]),
    "hd_stream_set_rtty": (_int, [_vp, _u32, _u32, _f]),
    "hd_stream_set_lowpass_bw": (_int, [_vp, _u32, _f]),
    "hd_stream_set_lowpass_trans": (_int, [_vp, _u32, _f]),
    "hd_stream_set_dc_remove": (_int, [_vp, _u32, _int]),
    "hd_stream_reset_frequency_correction": (_int, [_vp, _u32, _dbl]),
    "hd_stream_set_tune": (_int, [_vp, _u32, _dbl]),
    "hd_stream_set_front_tune": (_int, [_vp, _u32, _dbl]),
    "hd_stream_front_tune": (_int, [_vp, _u32, C.POINTER(hd_front_tune_info)]),
    "hd_stream_set_auto_afc": (_int, [_vp, _u32, _int, _dbl, _dbl]),
    "hd_stream_tune": (_int, [_vp, _u32, C.POINTER(hd_tune_info)]),
    "hd_set_sentence_callback": (None, [_vp, SENTENCE_CB, _vp]),
    "hd_set_match_callback": (None, [_vp, MATCH_CB, _vp]),
    "hd_set_chars_callback": (None, [_vp, CHARS_CB, _vp]),
    "hd_process_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_process_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_process_host_fmt": (_int, [_vp, _int, _vp, _sz, _vp, _u32]),
    "hd_process_device_fmt": (_int, [_vp, _int, _vp, _sz, _vp, _u32]),
    "hd_flush": (_int, [_vp]),
    "hd_ingest_run": (_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "hd_stream_rtty": (_sz, [_vp, _u32, C.c_char_p, _sz]),
    "hd_stream_last_sentence": (_sz, [_vp, _u32, C.c_char_p, _sz]),
    "hd_stream_take_sentences": (_sz, [_vp, _u32, C.c_char_p, _sz]),
    "hd_stream_take_matches": (_sz, [_vp, _u32, C.c_char_p, _sz]),
    "hd_stream_take_chars": (_sz, [_vp, _u32, C.c_char_p, _sz]),
    "hd_engine_sentences_ok": (C.c_uint64, [_vp]),
    "hd_stream_afc": (_int, [_vp, _u32, C.POINTER(hd_afc_info)]),
    "hd_stream_spectrum": (_sz, [_vp, _u32, _f32p, _sz]),
    "hd_stream_power": (_sz, [_vp, _u32, _f32p, _sz]),
    "hd_stream_demodulated": (_sz, [_vp, _u32, _f32p, _sz]),
    "hd_stream_decimated": (_sz, [_vp, _u32, _f32p, _sz]),
    "hd_stream_filtered": (_sz, [_vp, _u32, _f32p, _sz]),
    "hd_stream_bits": (_sz, [_vp, _u32, _u8p, _sz]),
    "hd_stream_flips": (_sz, [_vp, _u32, _u32p, _sz]),
    "hd_stream_fir_taps": (_sz, [_vp, _u32, _f32p, _sz]),
    "hd_stream_symbol_backlog": (_u32, [_vp, _u32]),
    "hd_stream_bits_total": (C.c_uint64, [_vp, _u32]),
    "hd_stream_flip_list_full": (C.c_uint64, [_vp, _u32]),
    "hd_stream_demod_checksum": (C.c_int, [_vp, _u32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "hd_stream_demod_checksum_total": (C.c_int, [_vp, _u32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hd_min_chunk": (_u32, [_u32]),
    "hd_engine_timing": (_int, [_vp, C.POINTER(hd_timing)]),
    "hd_engine_set_timing": (None, [_vp, _int]),
    "hd_survey_create": (_int, [_vp, C.POINTER(_vp)]),
    "hd_survey_destroy": (None, [_vp]),
    "hd_survey_reset": (_int, [_vp]),
    "hd_survey_push_device": (_int, [_vp, _vp, C.c_uint64]),
    "hd_survey_push_host": (_int, [_vp, _vp, C.c_uint64]),
    "hd_survey_push_host_fmt": (_int, [_vp, _int, _vp, C.c_uint64]),
    "hd_survey_push_device_fmt": (_int, [_vp, _int, _vp, C.c_uint64]),
    "hd_survey_power": (_int, [_vp, _vp, _sz, C.POINTER(C.c_uint64)]),
    "hd_survey_params_default": (None, [C.POINTER(hd_survey_params)]),
    "hd_survey_detect": (_int, [_vp, C.POINTER(hd_survey_params), C.POINTER(hd_survey_candidate), _u32, C.POINTER(_u32)]),
    "hd_waterfall_params_default": (None, [C.POINTER(hd_waterfall_params)]),
    "hd_waterfall_track_params_default": (None, [C.POINTER(hd_waterfall_track_params)]),
    "hd_waterfall_create": (_int, [_vp, C.POINTER(hd_waterfall_params), C.POINTER(_vp)]),
    "hd_waterfall_destroy": (None, [_vp]),
    "hd_waterfall_reset": (_int, [_vp]),
    "hd_waterfall_push_device": (_int, [_vp, _vp, C.c_uint64]),
    "hd_waterfall_push_host": (_int, [_vp, _vp, C.c_uint64]),
    "hd_waterfall_push_device_fmt": (_int, [_vp, _int, _vp, C.c_uint64]),
    "hd_waterfall_push_host_fmt": (_int, [_vp, _int, _vp, C.c_uint64]),
    "hd_waterfall_push_rows": (_int, [_vp, _vp, _vp, _u32, _int]),
    "hd_waterfall_rows_total": (C.c_uint64, [_vp]),
    "hd_waterfall_headers": (_int, [_vp, C.c_uint64, _u32, _vp]),
    "hd_waterfall_marks": (_int, [_vp, C.c_uint64, _u32, _vp]),
    "hd_waterfall_rows": (_int, [_vp, C.c_uint64, _u32, _vp]),
    "hd_waterfall_hits": (_int, [_vp, _vp, C.POINTER(C.c_uint64)]),
    "hd_waterfall_tracks": (_int, [_vp, C.POINTER(hd_waterfall_track_params), C.POINTER(hd_waterfall_track), _u32, C.POINTER(_u32)]),
    "hd_baud_probe_params_default": (None, [C.POINTER(hd_baud_probe_params)]),
    "hd_baud_probe_create": (_int, [_vp, C.POINTER(hd_baud_probe_params), C.POINTER(_vp)]),
    "hd_baud_probe_destroy": (None, [_vp]),
    "hd_baud_probe_reset": (_int, [_vp, _u32]),
    "hd_baud_probe_push_engine": (_int, [_vp]),
    "hd_baud_probe_push_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_baud_probe_push_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_baud_probe_estimate": (_int, [_vp, _u32, C.POINTER(hd_baud_estimate)]),
    "hd_baud_probe_state": (_int, [_vp, _u32, C.POINTER(hd_baud_probe_stream_state), _vp, _sz]),
    "hd_clocked_params_default": (None, [C.POINTER(hd_clocked_params)]),
    "hd_clocked_create": (_int, [_vp, C.POINTER(hd_clocked_params), C.POINTER(_vp)]),
    "hd_clocked_destroy": (None, [_vp]),
    "hd_clocked_reset": (_int, [_vp, _u32]),
    "hd_clocked_set_modem": (_int, [_vp, _u32, _dbl, _u32, _u32, _int]),
    "hd_clocked_push_engine": (_int, [_vp]),
    "hd_clocked_push_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_clocked_push_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_clocked_records": (_int, [_vp, _u32, _vp, _sz]),
    "hd_clocked_take_sentences": (_int, [_vp, _u32, _vp, _sz]),
    "hd_clocked_stats": (_int, [_vp, _u32, C.POINTER(hd_clocked_counters)]),
    "hd_tones_params_default": (None, [C.POINTER(hd_tones_params)]),
    "hd_tones_create": (_int, [_vp, C.POINTER(hd_tones_params), C.POINTER(_vp)]),
    "hd_tones_destroy": (None, [_vp]),
    "hd_tones_reset": (_int, [_vp, _u32]),
    "hd_tones_set_modem": (_int, [_vp, _u32, _dbl, _dbl, _dbl]),
    "hd_tones_set_modem_from_afc": (_int, [_vp, _u32, _dbl]),
    "hd_tones_push_engine": (_int, [_vp]),
    "hd_tones_push_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_tones_push_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_tones_rows": (_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), _vp]),
    "hd_tones_output": (_int, [_vp, _u32, _vp, _sz]),
    "hd_tones_stats": (_int, [_vp, _u32, C.POINTER(hd_tones_info)]),
    "hd_tone_search_params_default": (None, [C.POINTER(hd_tone_search_params)]),
    "hd_tone_search_detect_params_default": (None, [C.POINTER(hd_tone_search_detect_params)]),
    "hd_tone_search_create": (_int, [_vp, C.POINTER(hd_tone_search_params), C.POINTER(_vp)]),
    "hd_tone_search_destroy": (None, [_vp]),
    "hd_tone_search_reset": (_int, [_vp, _u32]),
    "hd_tone_search_push_engine": (_int, [_vp]),
    "hd_tone_search_push_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_tone_search_push_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_tone_search_power": (_int, [_vp, _u32, _vp, _sz, C.POINTER(C.c_uint64)]),
    "hd_tone_search_stats": (_int, [_vp, _u32, C.POINTER(hd_tone_search_info)]),
    "hd_tone_search_detect": (_int, [_vp, _u32, C.POINTER(hd_tone_search_detect_params), C.POINTER(hd_tone_search_result)]),
    "hd_combine_params_default": (None, [C.POINTER(hd_combine_params)]),
    "hd_combine_lag_params_default": (None, [C.POINTER(hd_combine_lag_params)]),
    "hd_combine_create": (_int, [_vp, C.POINTER(hd_combine_params), C.POINTER(_vp)]),
    "hd_combine_destroy": (None, [_vp]),
    "hd_combine_reset": (_int, [_vp, _u32]),
    "hd_combine_set_group": (_int, [_vp, _vp, _u32]),
    "hd_combine_set_delay": (_int, [_vp, _u32, _u32]),
    "hd_combine_set_weight": (_int, [_vp, _u32, _u32]),
    "hd_combine_push_engine": (_int, [_vp]),
    "hd_combine_push_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_combine_push_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_combine_rows": (_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), _vp]),
    "hd_combine_output": (_int, [_vp, _u32, _vp, _sz]),
    "hd_combine_stats": (_int, [_vp, _u32, C.POINTER(hd_combine_info)]),
    "hd_combine_lags": (_int, [_vp, _u32, C.POINTER(hd_combine_lag_params), _vp, _sz]),
    "hd_combine_align": (_int, [_vp, _u32, C.POINTER(hd_combine_lag_params), _vp, _sz]),
    "hd_ssdv_params_default": (None, [C.POINTER(hd_ssdv_params)]),
    "hd_ssdv_create": (_int, [_vp, C.POINTER(hd_ssdv_params), C.POINTER(_vp)]),
    "hd_ssdv_destroy": (None, [_vp]),
    "hd_ssdv_reset": (_int, [_vp, _u32]),
    "hd_ssdv_push_bytes": (_int, [_vp, _u32, _vp, _vp, _sz]),
    "hd_ssdv_push_records": (_int, [_vp, _u32, _vp, _sz, _u32]),
    "hd_ssdv_push_clocked": (_int, [_vp, _vp]),
    "hd_ssdv_scan": (_int, [_vp]),
    "hd_ssdv_take_packets": (_int, [_vp, _u32, _vp, _sz]),
    "hd_ssdv_stats": (_int, [_vp, _u32, C.POINTER(hd_ssdv_counters)]),
    "hd_fsk4_params_default": (None, [C.POINTER(hd_fsk4_params)]),
    "hd_fsk4_frame_preset": (_int, [_int, C.POINTER(hd_fsk4_frame)]),
    "hd_fsk4_create": (_int, [_vp, C.POINTER(hd_fsk4_params), C.POINTER(_vp)]),
    "hd_fsk4_destroy": (None, [_vp]),
    "hd_fsk4_reset": (_int, [_vp, _u32]),
    "hd_fsk4_set_modem": (_int, [_vp, _u32, _dbl, _dbl, _dbl, C.POINTER(hd_fsk4_frame)]),
    "hd_fsk4_push_engine": (_int, [_vp]),
    "hd_fsk4_push_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_fsk4_push_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_fsk4_scan": (_int, [_vp]),
    "hd_fsk4_take_frames": (_int, [_vp, _u32, _vp, _sz]),
    "hd_fsk4_stats": (_int, [_vp, _u32, C.POINTER(hd_fsk4_counters)]),
    "hd_fsk4_retune": (_int, [_vp, _u32, _dbl, _dbl, C.c_uint64]),
    "hd_fsk4_retune_stats": (_int, [_vp, _u32, C.POINTER(hd_fsk4_retune_info)]),
    "hd_fsk4_track_params_default": (None, [C.POINTER(hd_fsk4_track_params)]),
    "hd_fsk4_track_create": (_int, [_vp, C.POINTER(hd_fsk4_track_params), C.POINTER(_vp)]),
    "hd_fsk4_track_destroy": (None, [_vp]),
    "hd_fsk4_track_reset": (_int, [_vp, _u32]),
    "hd_fsk4_track_set_stream": (_int, [_vp, _u32, _dbl, _dbl, _dbl, _dbl, _dbl]),
    "hd_fsk4_track_attach": (_int, [_vp, _vp]),
    "hd_fsk4_track_push_engine": (_int, [_vp]),
    "hd_fsk4_track_push_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_fsk4_track_push_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_fsk4_track_estimate": (_int, [_vp, _u32, _vp]),
    "hd_fsk4_track_stats": (_int, [_vp, _u32, C.POINTER(hd_fsk4_track_info)]),
    "hd_afsk_params_default": (None, [C.POINTER(hd_afsk_params)]),
    "hd_afsk_create": (_int, [_vp, C.POINTER(hd_afsk_params), C.POINTER(_vp)]),
    "hd_afsk_destroy": (None, [_vp]),
    "hd_afsk_reset": (_int, [_vp, _u32]),
    "hd_afsk_set_modem": (_int, [_vp, _u32, _dbl, _dbl, _dbl]),
    "hd_afsk_set_bell202": (_int, [_vp, _u32]),
    "hd_afsk_push_engine": (_int, [_vp]),
    "hd_afsk_push_device": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_afsk_push_host": (_int, [_vp, _vp, _sz, _vp, _u32]),
    "hd_afsk_take_frames": (_int, [_vp, _u32, _vp, _sz]),
    "hd_afsk_stats": (_int, [_vp, _u32, C.POINTER(hd_afsk_counters)]),
    "hd_stream_set_format_trial": (_int, [_vp, _u32, _int]),
    "hd_stream_format_trial": (_int, [_vp, _u32, C.POINTER(hd_format_trial_result)]),
}
# every symbol declared in include/habdec_amd_host.h
HOST_API = {
    "hd_host_decim_plan": (_int, [C.c_uint, C.POINTER(_int), C.POINTER(C.c_uint)]),
    "hd_host_decim_taps": (_sz, [C.c_uint, _int, _f32p, _sz]),
    "hd_host_lowpass_design": (_sz, [_f, _f, _sz, _sz, _int, _f32p, _sz]),
    "hd_host_fir_demod_lds_bytes": (_sz, [_u32, C.POINTER(C.c_size_t)]),
    "hd_host_fir_demod_max_taps": (_u32, [_sz]),
    "hd_host_rtty_new": (_vp, [_sz, _f]),
    "hd_host_rtty_free": (None, [_vp]),
    "hd_host_rtty_pending": (_sz, [_vp]),
    "hd_host_rtty_push_run": (_sz, [_vp, _u8p, _sz, C.c_char_p, _sz]),
    "hd_host_crc16": (None, [C.c_char_p, _sz, C.c_char_p]),
    "hd_host_extract_sentence": (_int, [C.c_char_p, _sz, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, _sz]),
    "hd_host_text_new": (_vp, [_sz, _f]),
    "hd_host_text_free": (None, [_vp]),
    "hd_host_text_push_bits": (None, [_vp, _u8p, _sz]),
    "hd_host_text_get": (_sz, [_vp, _int, C.c_char_p, _sz]),
    "hd_host_afc_new": (_vp, []),
    "hd_host_afc_free": (None, [_vp]),
    "hd_host_afc_step": (None, [_vp, _int, _int, _int, _int, _f, _f, _dbl, _dbl, _sz, _dbl]),
    "hd_host_afc_reset": (None, [_vp, _dbl, _sz, _dbl]),
    "hd_host_afc_get": (None, [_vp] + [C.POINTER(_dbl)] * 4 + [C.POINTER(_int)] * 2),
    "hd_host_atan2f": (None, [_f32p, _f32p, _f32p, _sz]),
    "hd_host_discriminate": (None, [_f32p, _sz, _f, _f, _f32p]),
    "hd_host_spectrum_payload": (_sz, [_f32p, _sz, _dbl, _dbl, _dbl, _dbl, _int, _int, _f, _int, _int, _u8p, _sz, C.POINTER(_sz)]),
    "hd_host_demod_payload": (_sz, [_f32p, _sz, _int, _int, _u8p, _sz, C.POINTER(_sz)]),
    "hd_host_parse_time": (_int, [C.c_char_p, C.POINTER(_int), C.POINTER(_int), C.POINTER(_f)]),
    "hd_host_parse_gps_pos": (_int, [C.c_char_p, C.POINTER(_f)]),
    "hd_host_parse_sentence": (_int, [C.c_char_p, _vp]),
    "hd_host_timestamp_from_hms": (_sz, [C.c_int64, _int, _int, _f, C.c_char_p, _sz]),
    "hd_host_gps_distance": (None, [_dbl] * 6 + [C.POINTER(_dbl)]),
    "hd_host_sondehub_new": (_vp, [C.c_char_p, C.c_char_p]),
    "hd_host_sondehub_free": (None, [_vp]),
    "hd_host_sondehub_push_sentence": (_int, [_vp, _u32, C.c_char_p, C.c_char_p, C.c_int64]),
    "hd_host_sondehub_push": (_int, [_vp, C.c_char_p, C.c_char_p, C.c_char_p, _int, _f, _f, _f]),
    "hd_host_sondehub_size": (_sz, [_vp]),
    "hd_host_sondehub_take": (_sz, [_vp, C.c_int64, C.c_char_p, _sz, C.POINTER(_sz)]),
    "hd_host_utc_iso": (_sz, [C.c_int64, C.c_char_p, _sz]),
    "hd_host_json_number": (_sz, [_dbl, C.c_char_p, _sz]),
    "hd_host_iqfiles_open": (_vp, [C.POINTER(C.c_char_p), C.c_uint32, _int, C.c_uint32, C.c_uint32, _dbl]),
    "hd_host_iqfiles_close": (None, [_vp]),
    "hd_host_iqfiles_streams": (C.c_uint32, [_vp]),
    "hd_host_iqfiles_count": (C.c_uint64, [_vp, C.c_uint32]),
    "hd_host_iqfiles_rewinds": (C.c_uint64, [_vp, C.c_uint32]),
    "hd_host_iqfiles_next": (C.c_uint32, [_vp, _f32p, _sz, C.POINTER(C.c_uint32)]),
    "hd_host_iqfiles_open_fmt": (_vp, [C.POINTER(C.c_char_p), C.c_uint32, _int, C.c_uint32, C.c_uint32, _dbl, _int]),
    "hd_host_iqfiles_next_raw": (C.c_uint32, [_vp, _vp, _sz, C.POINTER(C.c_uint32)]),
    "hd_host_iq_bytes": (_sz, [_int]),
    "hd_host_iq_convert": (None, [_int, _vp, _sz, _f32p]),
    "hd_host_tune_step": (_int, [_dbl, _dbl, C.POINTER(C.c_uint32)]),
    "hd_host_tune_tables": (None, [_f32p, _f32p]),
    "hd_host_tune_rotate": (None, [_f32p, _sz, C.c_uint32, C.c_uint32, _f32p]),
    "hd_host_survey_window": (None, [_f32p]),
    "hd_host_survey_detect": (_int, [_f64p, C.c_uint64, _dbl, C.POINTER(hd_survey_params), C.POINTER(hd_survey_candidate), _u32, C.POINTER(_u32)]),
    "hd_host_waterfall_params_default": (None, [C.POINTER(hd_waterfall_params)]),
    "hd_host_waterfall_detect_row": (_int, [_vp, _u32, _dbl, C.POINTER(hd_waterfall_params), _vp, _vp]),
    "hd_host_waterfall_tracks": (_int, [_vp, _vp, C.c_uint64, _dbl, C.POINTER(hd_waterfall_track_params), C.POINTER(hd_waterfall_track), _u32, C.POINTER(_u32)]),
    "hd_host_baud_probe_new": (_vp, [_dbl, C.POINTER(hd_baud_probe_params)]),
    "hd_host_baud_probe_free": (None, [_vp]),
    "hd_host_baud_probe_reset": (None, [_vp]),
    "hd_host_baud_probe_push": (None, [_vp, _f32p, _sz]),
    "hd_host_baud_probe_state": (_int, [_vp, C.POINTER(hd_baud_probe_stream_state), _vp, _sz]),
    "hd_host_baud_probe_estimate": (_int, [_vp, C.POINTER(hd_baud_estimate)]),
    "hd_host_clocked_new": (_vp, [_dbl, C.POINTER(hd_clocked_params)]),
    "hd_host_clocked_free": (None, [_vp]),
    "hd_host_clocked_reset": (None, [_vp]),
    "hd_host_clocked_set_modem": (_int, [_vp, _dbl, _u32, _u32, _int]),
    "hd_host_clocked_push": (None, [_vp, _f32p, _sz]),
    "hd_host_clocked_records": (_int, [_vp, _vp, _sz]),
    "hd_host_clocked_take_sentences": (_int, [_vp, _vp, _sz]),
    "hd_host_clocked_stats": (_int, [_vp, C.POINTER(hd_clocked_counters)]),
    "hd_host_chase_repair": (_int, [C.c_char_p, _sz, _vp, _u32, _u32, _u32, _vp, C.POINTER(_u32)]),
    "hd_host_tones_new": (_vp, [_dbl, C.POINTER(hd_tones_params)]),
    "hd_host_tones_free": (None, [_vp]),
    "hd_host_tones_reset": (None, [_vp]),
    "hd_host_tones_set_modem": (_int, [_vp, _dbl, _dbl, _dbl]),
    "hd_host_tones_push": (_sz, [_vp, _vp, _sz, _vp]),
    "hd_host_tones_stats": (_int, [_vp, C.POINTER(hd_tones_info)]),
    "hd_host_tone_search_detect": (_int, [_vp, C.c_uint64, _dbl, C.POINTER(hd_tone_search_detect_params), C.POINTER(hd_tone_search_result)]),
    "hd_host_tone_search_create": (_vp, []),
    "hd_host_tone_search_destroy": (None, [_vp]),
    "hd_host_tone_search_reset": (None, [_vp]),
    "hd_host_tone_search_push": (None, [_vp, _vp, _sz]),
    "hd_host_tone_search_power": (_int, [_vp, _vp, _sz, C.POINTER(C.c_uint64)]),
    "hd_host_combine_create": (_vp, [_vp, _u32]),
    "hd_host_combine_destroy": (None, [_vp]),
    "hd_host_combine_reset": (None, [_vp]),
    "hd_host_combine_set_delay": (_int, [_vp, _u32, _u32]),
    "hd_host_combine_set_weight": (_int, [_vp, _u32, _u32]),
    "hd_host_combine_push": (_int, [_vp, _vp, _sz, _vp, _u32, _vp]),
    "hd_host_combine_lags": (_int, [_vp, C.POINTER(hd_combine_lag_params), _vp, _sz]),
    "hd_host_combine_align": (_int, [_vp, C.POINTER(hd_combine_lag_params), _vp, _sz]),
    "hd_host_combine_scores": (_int, [_vp, _u32, _vp, _sz]),
    "hd_host_combine_stats": (_int, [_vp, _u32, C.POINTER(hd_combine_info)]),
    "hd_host_ssdv_create": (_vp, [C.POINTER(hd_ssdv_params)]),
    "hd_host_ssdv_destroy": (None, [_vp]),
    "hd_host_ssdv_reset": (None, [_vp]),
    "hd_host_ssdv_push_bytes": (_int, [_vp, _vp, _vp, _sz]),
    "hd_host_ssdv_push_records": (_int, [_vp, _vp, _sz, _u32]),
    "hd_host_ssdv_take_packets": (_int, [_vp, _vp, _sz]),
    "hd_host_ssdv_stats": (_int, [_vp, C.POINTER(hd_ssdv_counters)]),
    "hd_host_ssdv_encode": (None, [_vp, _vp]),
    "hd_host_ssdv_make_packet": (None, [C.c_uint8, C.c_char_p, C.c_uint8, C.c_uint16, C.c_uint16, C.c_uint16, C.c_uint8, C.c_uint8, C.c_uint16, _vp, _vp]),
    "hd_host_fsk4_new": (_vp, [_dbl, C.POINTER(hd_fsk4_params)]),
    "hd_host_fsk4_free": (None, [_vp]),
    "hd_host_fsk4_reset": (None, [_vp]),
    "hd_host_fsk4_set_modem": (_int, [_vp, _dbl, _dbl, _dbl, C.POINTER(hd_fsk4_frame)]),
    "hd_host_fsk4_push": (_sz, [_vp, _vp, _sz]),
    "hd_host_fsk4_take_frames": (_int, [_vp, _vp, _sz]),
    "hd_host_fsk4_stats": (_int, [_vp, C.POINTER(hd_fsk4_counters)]),
    "hd_host_fsk4_slots": (_sz, [_vp, C.c_uint64, _vp, _sz]),
    "hd_host_fsk4_candidates": (_int, [_vp, _vp, _sz]),
    "hd_host_fsk4_encode": (_sz, [C.POINTER(hd_fsk4_frame), _vp, _vp]),
    "hd_host_fsk4_crc16": (_u32, [_vp, _sz]),
    "hd_host_fsk4_retune": (_int, [_vp, _dbl, _dbl, C.c_uint64]),
    "hd_host_fsk4_retune_stats": (_int, [_vp, C.POINTER(hd_fsk4_retune_info)]),
    "hd_host_fsk4_comb_detect": (_int, [_vp, _dbl, C.POINTER(hd_fsk4_comb_params), _vp]),
    "hd_host_fsk4_track_new": (_vp, [_dbl, C.POINTER(hd_fsk4_track_params)]),
    "hd_host_fsk4_track_free": (None, [_vp]),
    "hd_host_fsk4_track_reset": (None, [_vp]),
    "hd_host_fsk4_track_set_stream": (_int, [_vp, _dbl, _dbl, _dbl, _dbl, _dbl]),
    "hd_host_fsk4_track_attach": (None, [_vp, _vp]),
    "hd_host_fsk4_track_push": (None, [_vp, _vp, _sz]),
    "hd_host_fsk4_track_records": (_int, [_vp, _vp, _sz]),
    "hd_host_fsk4_track_stats": (_int, [_vp, C.POINTER(hd_fsk4_track_info)]),
    "hd_host_fsk4_track_acc": (_int, [_vp, _vp]),
    "hd_host_afsk_new": (_vp, [_dbl, C.POINTER(hd_afsk_params)]),
    "hd_host_afsk_free": (None, [_vp]),
    "hd_host_afsk_reset": (None, [_vp]),
    "hd_host_afsk_set_modem": (_int, [_vp, _dbl, _dbl, _dbl]),
    "hd_host_afsk_push": (_sz, [_vp, _vp, _sz]),
    "hd_host_afsk_take_frames": (_int, [_vp, _vp, _sz]),
    "hd_host_afsk_stats": (_int, [_vp, C.POINTER(hd_afsk_counters)]),
    "hd_host_afsk_slots": (_sz, [_vp, C.c_uint64, _vp, _sz]),
    "hd_host_afsk_candidates": (_int, [_vp, _vp, _sz]),
    "hd_host_afsk_crc16": (_u32, [_vp, _sz]),
    "hd_host_ax25_frame": (_sz, [C.c_char_p, _vp, _sz, _vp, _sz]),
    "hd_host_ax25_levels": (_sz, [_vp, _sz, _u32, _u32, _vp, _sz]),
    "hd_host_ax25_encode": (_sz, [C.c_char_p, _vp, _sz, _u32, _u32, _vp, _sz]),
    "hd_host_ax25_format": (_int, [_vp, _sz, _vp, _sz]),
    "hd_host_format_trial_new": (_vp, []),
    "hd_host_format_trial_free": (None, [_vp]),
    "hd_host_format_trial_push_bits": (None, [_vp, _u8p, _sz]),
    "hd_host_format_trial_get": (None, [_vp, C.POINTER(hd_format_trial_result)]),
}


def lib() -> C.CDLL:
    """Load libhabdec_amd.so (built in-tree by `python -m habdec_amd.build`).  Fails loudly: no fallback exists."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise HabdecError(f"{LIB_PATH} is missing: build it with `python -m habdec_amd.build` (hipcc, gfx950). "
                              "habdec_amd has no CPU or PyTorch fallback for the data path.")
        L = C.CDLL(str(LIB_PATH))
        for table in (ENGINE_API, HOST_API):
            for name, (res, args) in table.items():
                f = getattr(L, name)   # AttributeError = header and library out of sync
                f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise HabdecError(f"habdec_amd error {rc}: {lib().hd_last_error().decode()}")
