"""4FSK tone tracker (hd_fsk4_track_*, include/habdec_amd.h): finds a stream's four tones in a long-averaged spectrum, epoch by epoch, and retunes an
attached Fsk4 without a reset.

    from habdec_amd.fsk4_track import Fsk4Track, HostFsk4Track, comb_detect

Fsk4Track is a side object of an Engine like Fsk4; HostFsk4Track is one stream of it in plain C++ on the host, no GPU; comb_detect is the detector alone
on a spectrum of the caller's.  Per call: push the tracker first, then the Fsk4 it is attached to."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import HabdecError, check, lib
from .engine import Engine, _Handle, _IqRowObject, _params


def _record(r) -> dict:
    """One record (capi.FSK4_COMB_RECORD_DTYPE) as a dict."""
    d = {k: int(r[k]) for k in r.dtype.names if k not in ("centroid_q8", "_pad")}
    d["centroid_q8"] = [int(v) for v in r["centroid_q8"]]
    return d


def _estimate(e) -> dict:
    d = _record(e["rec"])
    d.update(f0_hz=float(e["f0_hz"]), spacing_hz=float(e["spacing_hz"]), end_sample=int(e["end_sample"]), epoch=int(e["epoch"]))
    return d


def _info(i) -> dict:
    return {k: int(getattr(i, k)) for k, _ in capi.hd_fsk4_track_info._fields_}


def comb_detect(acc, fsd, baud, spacing_lo, spacing_hi, f_lo, f_hi, min_quality_q8=192, segments_ok=True) -> np.ndarray:
    """hd_host_fsk4_comb_detect on 4096 fftshifted sums (no GPU): the record, one element of capi.FSK4_COMB_RECORD_DTYPE."""
    acc = np.ascontiguousarray(acc, np.float64)
    assert acc.shape == (4096,)
    p = capi.hd_fsk4_comb_params(float(baud), float(spacing_lo), float(spacing_hi), float(f_lo), float(f_hi), int(min_quality_q8), int(bool(segments_ok)))
    out = np.zeros(1, capi.FSK4_COMB_RECORD_DTYPE)
    rc = lib().hd_host_fsk4_comb_detect(acc.ctypes.data, float(fsd), C.byref(p), out.ctypes.data)
    if rc:
        raise HabdecError(f"habdec_amd error {rc}: hd_host_fsk4_comb_detect (a spacing of at least 2 baud, a band that holds the narrowest comb)")
    return out[0]


class Fsk4Track(_IqRowObject):
    """Tone tracker of an engine's streams: give a stream its search, push decimated IQ, read estimates; attach an Fsk4 to close the loop.  Closed with
    its engine, in front of it -- and in front of the Fsk4 it is attached to."""
    _prefix = "hd_fsk4_track"

    def __init__(self, eng: Engine, **params):
        super().__init__(eng, **params)
        eng._own(self)

    def set_stream(self, s, baud, spacing_lo, spacing_hi, f_lo, f_hi):
        """Give stream s its search (resets the stream): the tone spacing between spacing_lo and spacing_hi Hz (equal: known), all tones in f_lo .. f_hi."""
        check(self.L.hd_fsk4_track_set_stream(self.h, s, float(baud), float(spacing_lo), float(spacing_hi), float(f_lo), float(f_hi)))

    def attach(self, fsk4=None):
        check(self.L.hd_fsk4_track_attach(self.h, fsk4.h if fsk4 is not None else None))

    def estimate(self, s=0) -> dict:
        e = np.zeros(1, capi.FSK4_TRACK_EST_DTYPE)
        check(self.L.hd_fsk4_track_estimate(self.h, s, e.ctypes.data))
        return _estimate(e[0])

    def stats(self, s=0) -> dict:
        i = capi.hd_fsk4_track_info()
        check(self.L.hd_fsk4_track_stats(self.h, s, C.byref(i)))
        return _info(i)

    # ---- the library's test and measurement hooks (not part of the ABI)

    def debug_records(self, s=0) -> np.ndarray:
        """All records of stream s since its last reset (capi.FSK4_TRACK_EST_DTYPE)."""
        f = self.L.hd_debug_fsk4_track_records
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        out = np.zeros(max(f(self.h, s, None, 0), 0), capi.FSK4_TRACK_EST_DTYPE)
        n = f(self.h, s, out.ctypes.data, out.size) if out.size else 0
        return out[:n]

    def debug_acc(self, s=0) -> np.ndarray:
        f = self.L.hd_debug_fsk4_track_acc
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]
        out = np.zeros(4096, np.float64)
        check(min(f(self.h, s, out.ctypes.data), 0))
        return out

    def debug_comb(self, spectra, due, segments_ok) -> np.ndarray:
        """One launch of the comb kernel over spectra [S, 4096] of the caller's: the records of all streams.  Reset the streams afterwards."""
        f = self.L.hd_debug_fsk4_track_comb
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        spectra = np.ascontiguousarray(spectra, np.float64)
        due, ok = np.ascontiguousarray(due, np.uint32), np.ascontiguousarray(segments_ok, np.uint32)
        assert spectra.shape == (self.S, 4096) and due.shape == (self.S,) and ok.shape == (self.S,)
        out = np.zeros(self.S, capi.FSK4_COMB_RECORD_DTYPE)
        check(f(self.h, spectra.ctypes.data, due.ctypes.data, ok.ctypes.data, out.ctypes.data))
        return out

    def debug_guards(self, s) -> int:
        f = self.L.hd_debug_fsk4_track_guards
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32]
        return f(self.h, s)

    def debug_push_timed(self) -> tuple:
        """push_engine timed: (the whole push between two events in ms, its comb launches in ms, host microseconds of the whole call)."""
        f = self.L.hd_debug_fsk4_track_push_timed
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double)]
        a, b, us = C.c_float(0), C.c_float(0), C.c_double(0)
        check(f(self.h, C.byref(a), C.byref(b), C.byref(us)))
        return a.value, b.value, us.value


class HostFsk4Track(_Handle):
    """One stream of the tracker in plain C++ on the host (hd_host_fsk4_track_*): the tone search's double-precision spectrum, the detector's integers."""
    _destroy = "hd_host_fsk4_track_free"

    def __init__(self, decimated_rate: float, baud=None, spacing_lo=None, spacing_hi=None, f_lo=None, f_hi=None, **params):
        self.L = lib()
        p = _params(self.L, capi.hd_fsk4_track_params, "hd_fsk4_track_params_default", params, True)
        self.h = self.L.hd_host_fsk4_track_new(float(decimated_rate), C.byref(p))
        if not self.h:
            raise HabdecError("hd_host_fsk4_track_new: decimated_rate > 0, 1 <= epoch_segments <= 4096, decay_q8 <= 256")
        self._modem = None
        if baud is not None:
            self.set_stream(baud, spacing_lo, spacing_hi, f_lo, f_hi)

    def set_stream(self, baud, spacing_lo, spacing_hi, f_lo, f_hi):
        rc = self.L.hd_host_fsk4_track_set_stream(self.h, float(baud), float(spacing_lo), float(spacing_hi), float(f_lo), float(f_hi))
        if rc:
            raise HabdecError("habdec_amd error %d: hd_host_fsk4_track_set_stream (a spacing of at least 2 baud, a band that holds the narrowest comb)" % rc)

    def attach(self, host_fsk4=None):
        self._modem = host_fsk4                                          # (kept alive as long as it is attached)
        self.L.hd_host_fsk4_track_attach(self.h, host_fsk4.h if host_fsk4 is not None else None)

    def reset(self):
        self.L.hd_host_fsk4_track_reset(self.h)

    def push(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        if iq.size:
            self.L.hd_host_fsk4_track_push(self.h, iq.ctypes.data, iq.size)

    def records(self) -> np.ndarray:
        out = np.zeros(max(self.L.hd_host_fsk4_track_records(self.h, None, 0), 0), capi.FSK4_TRACK_EST_DTYPE)
        n = self.L.hd_host_fsk4_track_records(self.h, out.ctypes.data, out.size) if out.size else 0
        return out[:n]

    def acc(self) -> np.ndarray:
        out = np.zeros(4096, np.float64)
        check(min(self.L.hd_host_fsk4_track_acc(self.h, out.ctypes.data), 0))
        return out

    def stats(self) -> dict:
        i = capi.hd_fsk4_track_info()
        check(self.L.hd_host_fsk4_track_stats(self.h, C.byref(i)))
        return _info(i)
