"""Horus Binary 4FSK (hd_fsk4_*, include/habdec_amd.h): tuned decimated IQ in, CRC-checked Golay-corrected payloads out.

    from habdec_amd.fsk4 import Fsk4, HostFsk4, frame, horus_encode, fsk4_iq

Fsk4 is a side object of an Engine like Tones and Ssdv; HostFsk4 is one stream of it in plain C++ on the host, no GPU.  horus_encode and fsk4_iq make
the signals the tests and tools decode."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import HabdecError, check, lib
from .engine import Engine, _Handle, _IqRowObject, _params

HORUS_V1, HORUS_V2 = capi.FSK4_HORUS_V1, capi.FSK4_HORUS_V2


def frame(preset=HORUS_V1, **fields) -> capi.hd_fsk4_frame:
    """A frame descriptor: one of the presets (or a descriptor to copy), then every keyword over it (uw: two bytes)."""
    f = capi.hd_fsk4_frame()
    if isinstance(preset, capi.hd_fsk4_frame):
        C.memmove(C.byref(f), C.byref(preset), C.sizeof(f))
    elif lib().hd_fsk4_frame_preset(int(preset), C.byref(f)):
        raise HabdecError(f"hd_fsk4_frame_preset: no preset {preset}")
    for k, v in fields.items():
        if k == "uw":
            f.uw[0], f.uw[1] = int(v[0]), int(v[1])
        else:
            setattr(f, k, int(v))
    return f


def _frame(f) -> capi.hd_fsk4_frame:
    return f if isinstance(f, capi.hd_fsk4_frame) else frame(f)


def body_bytes(payload_bytes: int) -> int:
    """B of the definition: the payload and its parity stream."""
    return payload_bytes + (11 * ((8 * payload_bytes + 11) // 12) + 7) // 8


def crc16(data) -> int:
    d = np.frombuffer(bytes(data), np.uint8)
    return int(lib().hd_host_fsk4_crc16(d.ctypes.data if d.size else None, d.size))


def horus_encode(payload, frm=HORUS_V1) -> bytes:
    """The frame's bytes, unique word first.  payload: payload_bytes bytes as they are, or two fewer, and the CRC16 is appended."""
    f = _frame(frm)
    p = bytes(payload)
    if len(p) == f.payload_bytes - 2:
        c = crc16(p)
        p += bytes([c & 0xFF, c >> 8])
    assert len(p) == f.payload_bytes, (len(p), f.payload_bytes)
    d = np.frombuffer(p, np.uint8)
    out = np.zeros(2 + body_bytes(f.payload_bytes), np.uint8)
    n = lib().hd_host_fsk4_encode(C.byref(f), d.ctypes.data, out.ctypes.data)
    if n != out.size:
        raise HabdecError("hd_host_fsk4_encode: a frame the decoder cannot take")
    return out.tobytes()


def symbols(frame_bytes) -> np.ndarray:
    """Bytes -> 4FSK symbols: most significant bit first, two bits a symbol, first bit high."""
    b = np.unpackbits(np.frombuffer(bytes(frame_bytes), np.uint8))
    return (2 * b[0::2] + b[1::2]).astype(np.uint8)


def fsk4_iq(syms, fs, baud, f0, spacing, sigma=0.0, seed=0, amplitude=1.0, start=0.0, n_samples=None) -> np.ndarray:
    """Continuous-phase 4FSK: symbol k is the tone f0 + syms[k] * spacing from sample start + k * fs / baud on; silence (noise only) around it.
    sigma: standard deviation of the noise in each of re and im."""
    syms = np.asarray(syms, dtype=np.int64)
    spb = fs / baud
    n_sig = int(np.ceil(start + syms.size * spb))
    n = n_sig if n_samples is None else int(n_samples)
    i = np.arange(n, dtype=np.float64)
    k = np.floor((i - start) / spb).astype(np.int64)
    on = (k >= 0) & (k < syms.size)
    tone = syms[np.clip(k, 0, syms.size - 1)] if syms.size else np.zeros(n, np.int64)
    f = np.where(on, f0 + spacing * tone, 0.0)
    phase = 2 * np.pi * np.cumsum(f) / fs
    iq = np.where(on, amplitude * np.exp(1j * phase), 0.0)
    if sigma:
        rng = np.random.default_rng(seed)
        iq = iq + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return iq.astype(np.complex64)


def _frames(a) -> list:
    """One dict per frame: the fields of hd_fsk4_rx, payload as bytes of its length."""
    out = []
    for r in a:
        d = {k: int(r[k]) for k in a.dtype.names if k not in ("payload", "_pad")}
        d["payload"] = r["payload"].tobytes()[:int(r["payload_bytes"])] if "payload_bytes" in a.dtype.names else r["payload"].tobytes()
        out.append(d)
    return out


def _counters(c) -> dict:
    d = {k: int(getattr(c, k)) for k, _ in capi.hd_fsk4_counters._fields_ if k != "step"}
    d["step"] = [int(v) for v in c.step]
    return d


def _retune_info(i) -> dict:
    return {"retunes": int(i.retunes), "late": int(i.late), "waiting": int(i.waiting), "psi": [int(v) for v in i.psi]}


class Fsk4(_IqRowObject):
    """4FSK modem of an engine's streams: give a stream its modem, push decimated IQ (every push scans), take frames.  Closed with its engine, in front
    of it."""
    _prefix = "hd_fsk4"

    def __init__(self, eng: Engine, **params):
        super().__init__(eng, **params)
        eng._own(self)

    def set_modem(self, s, baud, f0, spacing, frm=HORUS_V1):
        """Give stream s its modem (resets the stream): tone t is f0 + t * spacing at the decimated rate."""
        f = _frame(frm)
        check(self.L.hd_fsk4_set_modem(self.h, s, float(baud), float(f0), float(spacing), C.byref(f)))

    def push_engine(self):
        """Demodulate every stream's decimated IQ of the call delivered last (drains the pipeline first, like the data getters), then scan."""
        super().push_engine()

    def scan(self):
        check(self.L.hd_fsk4_scan(self.h))

    def waiting(self, s=0) -> int:
        n = self.L.hd_fsk4_take_frames(self.h, s, None, 0)
        check(min(n, 0))
        return n

    def take_frames(self, s=0, cap=None) -> list:
        out = np.zeros(self.waiting(s) if cap is None else cap, capi.FSK4_RX_DTYPE)
        n = self.L.hd_fsk4_take_frames(self.h, s, out.ctypes.data, out.size) if out.size else 0
        check(min(n, 0))
        return _frames(out[:n])

    def stats(self, s=0) -> dict:
        c = capi.hd_fsk4_counters()
        check(self.L.hd_fsk4_stats(self.h, s, C.byref(c)))
        return _counters(c)

    def retune(self, s, f0, spacing, at_sample=0):
        """Move stream s's four tones at sample at_sample (counted from the stream's last reset) without a reset: the frame in flight is kept."""
        check(self.L.hd_fsk4_retune(self.h, s, float(f0), float(spacing), int(at_sample)))

    def retune_stats(self, s=0) -> dict:
        i = capi.hd_fsk4_retune_info()
        check(self.L.hd_fsk4_retune_stats(self.h, s, C.byref(i)))
        return _retune_info(i)

    # ---- the library's test and measurement hooks (not part of the ABI)

    def debug_slots(self, s, first, n) -> np.ndarray:
        """uint32 [n, 4]: the records of the slots first .. first + n - 1 as the stream's ring on the GPU holds them."""
        f = self.L.hd_debug_fsk4_slots
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t]
        out = np.zeros((int(n), 4), np.uint32)
        if n:
            check(min(f(self.h, s, int(first), out.ctypes.data, int(n)), 0))
        return out

    def debug_candidates(self, s=0) -> np.ndarray:
        """Takes the log of stream s's candidates behind the unique-word gate (capi.FSK4_CANDIDATE_DTYPE)."""
        f = self.L.hd_debug_fsk4_candidates
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        out = np.zeros(max(f(self.h, s, None, 0), 0), capi.FSK4_CANDIDATE_DTYPE)
        n = f(self.h, s, out.ctypes.data, out.size) if out.size else 0
        return out[:n]

    def debug_guards(self, s) -> int:
        f = self.L.hd_debug_fsk4_guards
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32]
        return f(self.h, s)

    def debug_push_timed(self) -> tuple:
        """push_engine with its kernels timed: (slot launches ms, frame launches ms, host microseconds of the whole call)."""
        f = self.L.hd_debug_fsk4_push_timed
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double)]
        a, b, us = C.c_float(0), C.c_float(0), C.c_double(0)
        check(f(self.h, C.byref(a), C.byref(b), C.byref(us)))
        return a.value, b.value, us.value


class HostFsk4(_Handle):
    """One stream of the 4FSK modem in plain C++ on the host (hd_host_fsk4_*): the restatement the kernels are held to, no GPU.  Every push scans."""
    _destroy = "hd_host_fsk4_free"

    def __init__(self, decimated_rate: float, baud=None, f0=None, spacing=None, frm=HORUS_V1, **params):
        self.L = lib()
        p = _params(self.L, capi.hd_fsk4_params, "hd_fsk4_params_default", params, True)
        self.h = self.L.hd_host_fsk4_new(float(decimated_rate), C.byref(p))
        if not self.h:
            raise HabdecError("hd_host_fsk4_new: decimated_rate > 0, 32 <= window_q8 <= 256, uw_max_errors <= 4, chase_bits <= 6, max_push <= 2^22")
        if baud is not None:
            self.set_modem(baud, f0, spacing, frm)

    def set_modem(self, baud, f0, spacing, frm=HORUS_V1):
        f = _frame(frm)
        rc = self.L.hd_host_fsk4_set_modem(self.h, float(baud), float(f0), float(spacing), C.byref(f))
        if rc:
            raise HabdecError("habdec_amd error %d: hd_host_fsk4_set_modem (8 <= samples per symbol <= 2048, a frame the decoder can take; every tone inside +- rate / 2)" % rc)

    def reset(self):
        self.L.hd_host_fsk4_reset(self.h)

    def retune(self, f0, spacing, at_sample=0):
        rc = self.L.hd_host_fsk4_retune(self.h, float(f0), float(spacing), int(at_sample))
        if rc:
            raise HabdecError("habdec_amd error %d: hd_host_fsk4_retune (a modem, and every tone inside +- rate / 2)" % rc)

    def retune_stats(self) -> dict:
        i = capi.hd_fsk4_retune_info()
        check(self.L.hd_host_fsk4_retune_stats(self.h, C.byref(i)))
        return _retune_info(i)

    def push(self, iq) -> int:
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        return self.L.hd_host_fsk4_push(self.h, iq.ctypes.data, iq.size) if iq.size else 0

    def take_frames(self, cap=None) -> list:
        out = np.zeros(self.L.hd_host_fsk4_take_frames(self.h, None, 0) if cap is None else cap, capi.FSK4_RX_DTYPE)
        n = self.L.hd_host_fsk4_take_frames(self.h, out.ctypes.data, out.size) if out.size else 0
        return _frames(out[:n])

    def slots(self, first, n) -> np.ndarray:
        out = np.zeros((int(n), 4), np.uint32)
        got = self.L.hd_host_fsk4_slots(self.h, int(first), out.ctypes.data, int(n)) if n else 0
        if got != n:
            raise HabdecError(f"hd_host_fsk4_slots: the ring does not hold slots {first} .. {first + n - 1}")
        return out

    def candidates(self) -> np.ndarray:
        out = np.zeros(self.L.hd_host_fsk4_candidates(self.h, None, 0), capi.FSK4_CANDIDATE_DTYPE)
        n = self.L.hd_host_fsk4_candidates(self.h, out.ctypes.data, out.size) if out.size else 0
        return out[:n]

    def stats(self) -> dict:
        c = capi.hd_fsk4_counters()
        check(self.L.hd_host_fsk4_stats(self.h, C.byref(c)))
        return _counters(c)
