"""APRS: Bell 202 AFSK carrying AX.25 UI frames (hd_afsk_*, include/habdec_amd.h): discriminator rows in, FCS-checked frames out.

    from habdec_amd.afsk import Afsk, HostAfsk, ax25_frame, ax25_encode, ax25_format, afsk_audio, fm_iq

Afsk is a side object of an Engine like Clocked; HostAfsk is one stream of it in plain C++ on the host, no GPU.  ax25_frame, ax25_encode, afsk_audio
and fm_iq make the signals the tests and tools decode; ax25_format writes a delivered frame as a TNC2 monitor line."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import HabdecError, check, lib
from .engine import Engine, _Handle, _RowObject, _params

OPEN, ABORT, UNSHAPED, FCS_FAILED, REFUSED, PLAIN, REPAIRED = range(7)


def crc16(data) -> int:
    """CRC-16/X-25, the FCS of the bytes."""
    d = np.frombuffer(bytes(data), np.uint8)
    return int(lib().hd_host_afsk_crc16(d.ctypes.data if d.size else None, d.size))


def ax25_frame(path: str, info=b"") -> bytes:
    """A UI frame with its FCS.  path: the TNC2 header "SRC-SSID>DST,DIGI1,DIGI2*"."""
    i = np.frombuffer(bytes(info), np.uint8)
    out = np.zeros(80 + i.size, np.uint8)
    n = lib().hd_host_ax25_frame(path.encode(), i.ctypes.data if i.size else None, i.size, out.ctypes.data, out.size)
    if not n:
        raise HabdecError(f"hd_host_ax25_frame: not a path: {path!r}")
    return out[:n].tobytes()


def ax25_levels(frame, flags_before=8, flags_after=2) -> np.ndarray:
    """Frame bytes (FCS included) -> flags, stuffed bits, flags as NRZI levels (uint8, 0 / 1), the level in front of the first bit 0."""
    f = np.frombuffer(bytes(frame), np.uint8)
    n = lib().hd_host_ax25_levels(f.ctypes.data if f.size else None, f.size, flags_before, flags_after, None, 0)
    out = np.zeros(n, np.uint8)
    lib().hd_host_ax25_levels(f.ctypes.data if f.size else None, f.size, flags_before, flags_after, out.ctypes.data, out.size)
    return out


def ax25_encode(path: str, info=b"", flags_before=8, flags_after=2) -> np.ndarray:
    """Path and information -> the frame's NRZI levels (hd_host_ax25_encode)."""
    i = np.frombuffer(bytes(info), np.uint8)
    args = (path.encode(), i.ctypes.data if i.size else None, i.size, flags_before, flags_after)
    n = lib().hd_host_ax25_encode(*args, None, 0)
    if not n:
        raise HabdecError(f"hd_host_ax25_encode: not a path: {path!r}")
    out = np.zeros(n, np.uint8)
    lib().hd_host_ax25_encode(*args, out.ctypes.data, out.size)
    return out


def ax25_format(data) -> str:
    """A delivered frame (without FCS) as "SRC-SSID>DST,DIGI*:info"."""
    d = np.frombuffer(bytes(data), np.uint8)
    out = C.create_string_buffer(6 * d.size + 128)         # (a byte outside 32 .. 126 is written as <0xNN>, six characters)
    n = lib().hd_host_ax25_format(d.ctypes.data if d.size else None, d.size, out, len(out))
    if n < 0:
        raise HabdecError("habdec_amd error %d: hd_host_ax25_format (%s)" % (n, {-3: "not a UI frame", -4: "the line does not fit"}.get(n, "no address field")))      # (HD_ERR_UNSUPPORTED, HD_ERR_CAPACITY)
    return out.value.decode("latin-1")


def afsk_audio(levels, fs, baud=1200.0, mark=1200.0, space=2200.0, peak=0.5, start=0.0, n_samples=None, idle=None, bit_peak=None) -> np.ndarray:
    """Continuous-phase AFSK audio (float64): level k -- 1 the mark tone, 0 the space tone -- from sample start + k * fs / baud on.  Around the levels
    there is silence, or the tone of level `idle` where that is 0 or 1."""
    levels = np.asarray(levels, dtype=np.int64)
    spb = fs / baud
    n = int(np.ceil(start + levels.size * spb)) if n_samples is None else int(n_samples)
    i = np.arange(n, dtype=np.float64)
    k = np.floor((i - start) / spb).astype(np.int64)
    on = (k >= 0) & (k < levels.size)
    lv = levels[np.clip(k, 0, max(levels.size - 1, 0))] if levels.size else np.zeros(n, np.int64)
    if idle is not None:
        lv = np.where(on, lv, int(idle))
        on = np.ones(n, bool)
    f = np.where(lv == 1, mark, space)
    phase = 2 * np.pi * np.cumsum(np.where(on, f, 0.0)) / fs
    if bit_peak is not None:                      # a peak per bit: a weak bit is one the modem is not sure of
        peak = np.where((k >= 0) & (k < levels.size), np.asarray(bit_peak, np.float64)[np.clip(k, 0, max(levels.size - 1, 0))], peak)
    return np.where(on, peak * np.sin(phase), 0.0)


def fm_iq(audio, fs, deviation=3000.0, audio_peak=0.5, offset=0.0, amplitude=1.0, sigma=0.0, seed=0) -> np.ndarray:
    """The audio frequency-modulated onto cf32 IQ at rate fs: audio_peak gives `deviation` Hz, the carrier stands at `offset` Hz; sigma: standard
    deviation of the noise in each of re and im."""
    a = np.asarray(audio, dtype=np.float64)
    f = offset + deviation * a / audio_peak
    iq = amplitude * np.exp(2j * np.pi * np.cumsum(f) / fs)
    if sigma:
        rng = np.random.default_rng(seed)
        iq = iq + sigma * (rng.standard_normal(a.size) + 1j * rng.standard_normal(a.size))
    return iq.astype(np.complex64)


def _frames(a) -> list:
    """One dict per record: the fields of hd_afsk_rx or hd_afsk_candidate, data as bytes of its length."""
    out = []
    for r in a:
        d = {k: int(r[k]) for k in a.dtype.names if k not in ("data", "_pad", "_pad2")}
        d["data"] = r["data"].tobytes()[:int(r["len"])]
        out.append(d)
    return out


def _counters(c) -> dict:
    d = {k: int(getattr(c, k)) for k, _ in capi.hd_afsk_counters._fields_ if k != "step"}
    d["step"] = [int(v) for v in c.step]
    return d


class Afsk(_RowObject):
    """AFSK / AX.25 modem of an engine's streams: give a stream its modem, push discriminator rows (every push scans), take frames.  Closed with its
    engine, in front of it."""
    _prefix, _ints = "hd_afsk", True

    def __init__(self, eng: Engine, **params):
        super().__init__(eng, **params)
        eng._own(self)

    def set_modem(self, s, baud=1200.0, mark=1200.0, space=2200.0):
        """Give stream s its modem (resets the stream); the defaults are Bell 202."""
        check(self.L.hd_afsk_set_modem(self.h, s, float(baud), float(mark), float(space)))

    def set_bell202(self, s):
        check(self.L.hd_afsk_set_bell202(self.h, s))

    def waiting(self, s=0) -> int:
        n = self.L.hd_afsk_take_frames(self.h, s, None, 0)
        check(min(n, 0))
        return n

    def take_frames(self, s=0, cap=None) -> list:
        out = np.zeros(self.waiting(s) if cap is None else cap, capi.AFSK_RX_DTYPE)
        n = self.L.hd_afsk_take_frames(self.h, s, out.ctypes.data, out.size) if out.size else 0
        check(min(n, 0))
        return _frames(out[:n])

    def stats(self, s=0) -> dict:
        c = capi.hd_afsk_counters()
        check(self.L.hd_afsk_stats(self.h, s, C.byref(c)))
        return _counters(c)

    # ---- the library's test and measurement hooks (not part of the ABI)

    def debug_slots(self, s, first, n) -> np.ndarray:
        """int32 [n]: the records of the slots first .. first + n - 1 as the stream's ring on the GPU holds them."""
        f = self.L.hd_debug_afsk_slots
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t]
        out = np.zeros(int(n), np.int32)
        if n:
            check(min(f(self.h, s, int(first), out.ctypes.data, int(n)), 0))
        return out

    def debug_candidates(self, s=0) -> np.ndarray:
        """Takes the log of stream s's candidates (capi.AFSK_CANDIDATE_DTYPE)."""
        f = self.L.hd_debug_afsk_candidates
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        out = np.zeros(max(f(self.h, s, None, 0), 0), capi.AFSK_CANDIDATE_DTYPE)
        n = f(self.h, s, out.ctypes.data, out.size) if out.size else 0
        return out[:n]

    def debug_guards(self, s) -> int:
        f = self.L.hd_debug_afsk_guards
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32]
        return f(self.h, s)

    def debug_push_timed(self) -> tuple:
        """push_engine with its kernels timed: (slot launches ms, gate and frame launches ms, host microseconds of the whole call)."""
        f = self.L.hd_debug_afsk_push_timed
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double)]
        a, b, us = C.c_float(0), C.c_float(0), C.c_double(0)
        check(f(self.h, C.byref(a), C.byref(b), C.byref(us)))
        return a.value, b.value, us.value


class HostAfsk(_Handle):
    """One stream of the AFSK modem in plain C++ on the host (hd_host_afsk_*): the restatement the kernels are held to, no GPU.  Every push scans."""
    _destroy = "hd_host_afsk_free"

    def __init__(self, decimated_rate: float, baud=None, mark=1200.0, space=2200.0, **params):
        self.L = lib()
        p = _params(self.L, capi.hd_afsk_params, "hd_afsk_params_default", params, True)
        self.h = self.L.hd_host_afsk_new(float(decimated_rate), C.byref(p))
        if not self.h:
            raise HabdecError("hd_host_afsk_new: decimated_rate > 0, 17 <= max_frame_bytes <= 332, repair_flips <= 4, at most 64 flip patterns, a ring that holds 8 L + 72 + max_push")
        if baud is not None:
            self.set_modem(baud, mark, space)

    def set_modem(self, baud=1200.0, mark=1200.0, space=2200.0):
        rc = self.L.hd_host_afsk_set_modem(self.h, float(baud), float(mark), float(space))
        if rc:
            raise HabdecError("habdec_amd error %d: hd_host_afsk_set_modem (8 <= samples per bit <= 2048; 0 < mark, space < rate / 2, two different tones)" % rc)

    def reset(self):
        self.L.hd_host_afsk_reset(self.h)

    def push(self, row) -> int:
        row = np.ascontiguousarray(row, dtype=np.float32).reshape(-1)
        return self.L.hd_host_afsk_push(self.h, row.ctypes.data, row.size) if row.size else 0

    def take_frames(self, cap=None) -> list:
        out = np.zeros(self.L.hd_host_afsk_take_frames(self.h, None, 0) if cap is None else cap, capi.AFSK_RX_DTYPE)
        n = self.L.hd_host_afsk_take_frames(self.h, out.ctypes.data, out.size) if out.size else 0
        return _frames(out[:n])

    def slots(self, first, n) -> np.ndarray:
        out = np.zeros(int(n), np.int32)
        got = self.L.hd_host_afsk_slots(self.h, int(first), out.ctypes.data, int(n)) if n else 0
        if got != n:
            raise HabdecError(f"hd_host_afsk_slots: the ring does not hold slots {first} .. {first + n - 1}")
        return out

    def candidates(self) -> np.ndarray:
        out = np.zeros(self.L.hd_host_afsk_candidates(self.h, None, 0), capi.AFSK_CANDIDATE_DTYPE)
        n = self.L.hd_host_afsk_candidates(self.h, out.ctypes.data, out.size) if out.size else 0
        return out[:n]

    def stats(self) -> dict:
        c = capi.hd_afsk_counters()
        check(self.L.hd_host_afsk_stats(self.h, C.byref(c)))
        return _counters(c)
