"""Thin Python mirror of the C ABI: one `Engine` = one GPU, S independent IQ streams (tests and bench plumbing)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi
from .capi import HabdecError, check, lib


@dataclass
class EngineConfig:
    n_streams: int = 1
    max_chunk: int = 65536
    sampling_rate: float = 2.048e6
    decimation: int = 64
    baud: float = 300.0
    rtty_bits: int = 8
    rtty_stops: float = 2.0
    lowpass_bw_hz: float = 1500.0
    lowpass_trans: float = 0.025
    dc_remove: bool = False
    lookup_mode: int = 1
    enable_spectrum: bool = True
    ungated: bool = False
    keep_filtered: bool = False
    pipeline: int = 0        # 0 synchronous, 1 batch mode (results one call later), 2 batch mode with one more call in flight
    arith: int = 0           # 0 exact (separately rounded multiply and add: bit-identical floats), 1 fast (fused multiply-add, tolerance 1e-5)
    device: int = 0


class _Handle:
    """An object of the library behind a handle: L the library, h the handle, _destroy the name of the symbol that frees it."""
    L = h = _destroy = None

    def close(self):
        if self.h:
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _create(self, eng: "Engine", symbol: str, *args):
        """A side object of an engine: symbol(engine, *args, &handle)."""
        self.L, self.eng = eng.L, eng
        h = C.c_void_p()
        check(getattr(self.L, symbol)(eng.h, *args, C.byref(h)))
        self.h = h


def _params(L, struct, default: str, kw: dict, ints=()):
    """A parameter struct: the library's defaults (the symbol `default`), then every keyword -- as an int where `ints` names it (True: all), else a float."""
    p = struct()
    getattr(L, default)(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, int(v) if ints is True or k in ints else float(v))
    return p


def _with_cap(call, cap: int, struct, convert):
    """call(out, cap, byref(found)) fills at most cap of `struct` and reports how many there are: again with that capacity where it was more."""
    while True:
        out, found = (struct * max(cap, 1))(), C.c_uint32(0)
        call(out, cap, C.byref(found))
        if found.value <= cap:
            return convert(out, found.value)
        cap = found.value


def _power(fn, *h, host: str | None = None):
    """(float64[4096], segments) from one of the power getters; any other answer than 4096 bins raises (host: the name of a function that sets no message)."""
    p, seg = np.zeros(4096, np.float64), C.c_uint64(0)
    n = fn(*h, p.ctypes.data, p.size, C.byref(seg))
    if n != 4096 and host:
        raise HabdecError(f"habdec_amd error {n}: {host}")
    if n != 4096:
        check(n if n < 0 else -1)
    return p, int(seg.value)


class Engine(_Handle):
    _destroy = "hd_engine_destroy"

    def __init__(self, cfg: EngineConfig | None = None, **kw):
        self._cbs, self._owned, self._pinned = [], [], []
        cfg = cfg or EngineConfig(**kw)
        self.cfg = cfg
        L = lib()
        c = capi.hd_engine_config()
        L.hd_engine_config_default(C.byref(c))
        for k in ("device", "n_streams", "max_chunk", "sampling_rate", "decimation", "baud", "rtty_bits", "rtty_stops",
                  "lowpass_bw_hz", "lowpass_trans", "lookup_mode"):
            setattr(c, k, getattr(cfg, k))
        c.dc_remove, c.enable_spectrum, c.ungated, c.keep_filtered = int(cfg.dc_remove), int(cfg.enable_spectrum), int(cfg.ungated), int(cfg.keep_filtered)
        c.pipeline = int(cfg.pipeline)
        c.arith = int(cfg.arith)
        h = C.c_void_p()
        check(L.hd_engine_create(C.byref(c), C.byref(h)))
        self.h, self.L = h, L
        self.S = cfg.n_streams

    def close(self):
        for o in self._owned:       # (a side object uses its engine's device and mutex: it goes first)
            o.close()
        self._owned = []
        super().close()
        for p in self._pinned:
            self.L.hd_pinned_free(p)
        self._pinned = []

    def _own(self, obj):
        """A side object made by one of the factories below: closed with the engine, in front of it."""
        self._owned.append(obj)
        return obj

    # ---- data path
    def process_host(self, iq: np.ndarray, n: int | None = None, fmt=None):
        """iq: complex64 [S, stride]; stream s hands over its first n samples.
        Packed IQ (hd_process_host_fmt): an integer array [S, stride, 2] of dtype int16 / int8 / uint8 (cs16 / cs8 / cu8), or `fmt=` naming the format."""
        iq = np.asarray(iq)
        if fmt is None and iq.dtype in (np.int16, np.int8, np.uint8):
            fmt = {np.dtype(np.int16): capi.IQ_CS16, np.dtype(np.int8): capi.IQ_CS8, np.dtype(np.uint8): capi.IQ_CU8}[iq.dtype]
        if fmt is not None and capi.iq_fmt(fmt) != capi.IQ_CF32:
            fmt = capi.iq_fmt(fmt)
            if fmt in capi.IQ_DTYPES and iq.dtype != capi.IQ_DTYPES[fmt]:
                raise HabdecError(f"IQ format {fmt} wants dtype {capi.IQ_DTYPES[fmt]}, not {iq.dtype}")
            iq = np.ascontiguousarray(iq)
            if iq.ndim == 2:
                iq = iq[None, :, :]
            assert iq.ndim == 3 and iq.shape[0] == self.S and iq.shape[2] == 2, iq.shape
            n = iq.shape[1] if n is None else n
            check(self.L.hd_process_host_fmt(self.h, fmt, iq.ctypes.data, iq.shape[1], None, n))
            return
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        if iq.ndim == 1:
            iq = iq[None, :]
        assert iq.shape[0] == self.S
        n = iq.shape[1] if n is None else n
        check(self.L.hd_process_host(self.h, iq.ctypes.data, iq.shape[1], None, n))

    def pinned_array(self, shape, dtype=np.complex64) -> np.ndarray:
        """A numpy array in page-locked, GPU-mapped memory (hd_pinned_alloc): process_host() of a synchronous engine reads it in place over PCIe."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.L.hd_pinned_alloc(n)
        if not p:
            raise HabdecError("hd_pinned_alloc failed")
        buf = (C.c_char * n).from_address(p)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned.append(p)
        return arr

    def process_device(self, dev_ptr: int, stride: int, n: int, fmt=None):
        """fmt: the samples at dev_ptr are packed (hd_process_device_fmt); stride and n count complex samples either way."""
        if fmt is not None:
            check(self.L.hd_process_device_fmt(self.h, capi.iq_fmt(fmt), dev_ptr, stride, None, n))
            return
        check(self.L.hd_process_device(self.h, dev_ptr, stride, None, n))

    def ingest(self, files: "IqFiles", max_rounds: int = 1 << 62) -> int:
        """Pump a batch of IQ files (one per stream; cf32, or packed when opened with fmt=) through the engine (hd_ingest_run); returns the samples consumed."""
        done = C.c_uint64(0)
        check(self.L.hd_ingest_run(self.h, files.h, max_rounds, C.byref(done)))
        return int(done.value)

    def flush(self):
        check(self.L.hd_flush(self.h))

    # ---- control
    def set_baud(self, s, baud): check(self.L.hd_stream_set_baud(self.h, s, baud))
    def set_rtty(self, s, bits, stops): check(self.L.hd_stream_set_rtty(self.h, s, bits, stops))
    def set_lowpass_bw(self, s, hz): check(self.L.hd_stream_set_lowpass_bw(self.h, s, hz))
    def set_lowpass_trans(self, s, t): check(self.L.hd_stream_set_lowpass_trans(self.h, s, t))
    def set_dc_remove(self, s, on): check(self.L.hd_stream_set_dc_remove(self.h, s, int(on)))
    def reset_frequency_correction(self, s, c): check(self.L.hd_stream_reset_frequency_correction(self.h, s, c))
    def set_tune(self, s, offset_hz): check(self.L.hd_stream_set_tune(self.h, s, float(offset_hz)))

    def set_front_tune(self, s, offset_hz):
        """Tune stream s at the INPUT rate, in front of the first decimation stage (hd_stream_set_front_tune): |offset_hz| < sampling_rate / 2."""
        check(self.L.hd_stream_set_front_tune(self.h, s, float(offset_hz)))

    def front_tune(self, s=0) -> dict:
        t = capi.hd_front_tune_info()
        check(self.L.hd_stream_front_tune(self.h, s, C.byref(t)))
        return {"offset_hz": t.offset_hz, "step": t.step, "phase": t.phase, "from_call": t.from_call}

    def set_auto_afc(self, s, on=True, hold_s=6.0, min_hz=100.0):
        """The server's AFC block per stream, in sample time: retune the stream (not a radio) by the AFC's correction (hd_stream_set_auto_afc)."""
        check(self.L.hd_stream_set_auto_afc(self.h, s, int(on), float(hold_s), float(min_hz)))

    def tune(self, s=0) -> dict:
        t = capi.hd_tune_info()
        check(self.L.hd_stream_tune(self.h, s, C.byref(t)))
        return {"offset_hz": t.offset_hz, "step": t.step, "phase": t.phase, "retunes": t.retunes, "from_call": t.from_call, "auto_afc": bool(t.auto_afc)}

    def on_sentence(self, fn):
        cb = capi.SENTENCE_CB(lambda user, s, call, data, crc: fn(s, call.decode("latin-1"), data.decode("latin-1"), crc.decode("latin-1")))
        self._cbs.append(cb)
        self.L.hd_set_sentence_callback(self.h, cb, None)

    # ---- results
    def _text(self, fn, s, cap=1 << 16) -> str:
        buf = C.create_string_buffer(cap)
        n = fn(self.h, s, buf, cap)
        if n >= cap:
            return self._text(fn, s, n + 1)
        return buf.raw[:n].decode("latin-1")

    def rtty(self, s=0): return self._text(self.L.hd_stream_rtty, s)
    def last_sentence(self, s=0): return self._text(self.L.hd_stream_last_sentence, s)
    def take_sentences(self, s=0): return [x for x in self._text(self.L.hd_stream_take_sentences, s).split("\n") if x]
    def take_matches(self, s=0): return [x for x in self._text(self.L.hd_stream_take_matches, s).split("\n") if x]
    def take_chars(self, s=0): return self._text(self.L.hd_stream_take_chars, s)
    def sentences_ok(self) -> int: return self.L.hd_engine_sentences_ok(self.h)

    def afc(self, s=0) -> dict:
        a = capi.hd_afc_info()
        check(self.L.hd_stream_afc(self.h, s, C.byref(a)))
        return {"correction": a.frequency_correction, "shift_hz": a.shift_hz, "noise_floor": a.noise_floor,
                "noise_var": a.noise_variance, "peak_l": a.peak_left, "peak_r": a.peak_right, "spectra": a.spectra}

    def _arr(self, fn, s, cplx, cap):
        buf = np.zeros(cap * (2 if cplx else 1), np.float32)
        n = fn(self.h, s, buf, cap)
        if n > cap:
            return self._arr(fn, s, cplx, n)
        out = buf[: n * (2 if cplx else 1)]
        return out.view(np.complex64) if cplx else out

    def spectrum(self, s=0): return self._arr(self.L.hd_stream_spectrum, s, True, 4096)
    def power(self, s=0): return self._arr(self.L.hd_stream_power, s, False, 4096)
    def demodulated(self, s=0): return self._arr(self.L.hd_stream_demodulated, s, False, 1 << 15)
    def decimated(self, s=0): return self._arr(self.L.hd_stream_decimated, s, True, 1 << 16)
    def filtered(self, s=0): return self._arr(self.L.hd_stream_filtered, s, True, 1 << 15)
    def fir_taps(self, s=0): return self._arr(self.L.hd_stream_fir_taps, s, False, 8192)

    def bits(self, s=0) -> np.ndarray:
        cap = 1 << 16
        buf = np.zeros(cap, np.uint8)
        n = self.L.hd_stream_bits(self.h, s, buf, cap)
        return buf[:n].copy()

    def flips(self, s=0) -> np.ndarray:
        buf = np.zeros(4096, np.uint32)
        n = self.L.hd_stream_flips(self.h, s, buf, 4096)
        return buf[:n].copy()

    def symbol_backlog(self, s=0) -> int: return self.L.hd_stream_symbol_backlog(self.h, s)

    def lowpass_taps_max(self) -> int:
        """The longest low-pass design a call may run (hd_engine_lowpass_taps_max); a call whose design is longer is refused with HD_ERR_CAPACITY."""
        return int(self.L.hd_engine_lowpass_taps_max(self.h))

    def bits_total(self, s=0) -> int: return int(self.L.hd_stream_bits_total(self.h, s))
    def flip_list_full(self, s=0) -> int: return int(self.L.hd_stream_flip_list_full(self.h, s))

    def demod_checksum(self, s=0):
        """(call index, n, ck0, ck1) of the call delivered last for stream s -- no flush; n is None where the launch path does not compute it."""
        ci, n, ck = C.c_uint64(0), C.c_uint32(0), (C.c_uint32 * 2)()
        check(self.L.hd_stream_demod_checksum(self.h, s, C.byref(ci), C.byref(n), ck))
        return int(ci.value), (None if n.value == 0xFFFFFFFF else int(n.value)), int(ck[0]), int(ck[1])

    def demod_checksum_total(self, s=0):
        """(calls folded in, delivered calls without a checksum, hash): every delivered call's discriminator checksum folded into one word -- no flush."""
        n, u, h = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(self.L.hd_stream_demod_checksum_total(self.h, s, C.byref(n), C.byref(u), C.byref(h)))
        return int(n.value), int(u.value), int(h.value)

    def timing(self) -> dict:
        t = capi.hd_timing()
        check(self.L.hd_engine_timing(self.h, C.byref(t)))
        return {"ms_total": t.ms_total, "ms_front": t.ms_front, "front_bytes": t.front_bytes, "samples": t.samples,
                "host_enqueue_us": t.host_enqueue_us, "host_wait_us": t.host_wait_us, "host_text_us": t.host_text_us,
                "timed_calls": t.timed_calls, "path": t.path, "step_variant": t.step_variant, "host_calls_in_place": t.host_calls_in_place, "lowpass_fft_calls": t.lowpass_fft_calls}

    def set_timing(self, every: int):
        """HIP-event timing on every `every`-th call (0 = off); see hd_engine_set_timing."""
        self.L.hd_engine_set_timing(self.h, every)

    def survey(self) -> "Survey":
        """A wideband survey on this engine's GPU and sampling rate (hd_survey_*): close it before the engine."""
        return self._own(Survey(self))

    def waterfall(self, **params) -> "Waterfall":
        """A waterfall on this engine's GPU and sampling rate (hd_waterfall_*; params as hd_waterfall_params): close it before the engine."""
        return self._own(Waterfall(self, **params))

    def baud_probe(self, **params) -> "BaudProbe":
        """A baud-rate probe on this engine's streams (hd_baud_probe_*; params as hd_baud_probe_params): close it before the engine."""
        return self._own(BaudProbe(self, **params))

    def clocked(self, **params) -> "Clocked":
        """A clocked decoder on this engine's streams (hd_clocked_*; params as hd_clocked_params): close it before the engine."""
        return self._own(Clocked(self, **params))

    def tones(self, **params) -> "Tones":
        """A tone-filter demodulator on this engine's streams (hd_tones_*; params as hd_tones_params): close it before the engine."""
        return self._own(Tones(self, **params))

    def tone_search(self, **params) -> "ToneSearch":
        """A tone search on this engine's streams (hd_tone_search_*; params as hd_tone_search_params): close it before the engine."""
        return self._own(ToneSearch(self, **params))

    def set_format_trial(self, s, on=True):
        """Tee the bits delivered for stream s into a framing trial (hd_stream_set_format_trial); turning it on resets it."""
        check(self.L.hd_stream_set_format_trial(self.h, s, int(on)))

    def format_trial(self, s=0) -> dict:
        r = capi.hd_format_trial_result()
        check(self.L.hd_stream_format_trial(self.h, s, C.byref(r)))
        return _trial_result(r)


def _trial_result(r) -> dict:
    return {"best": r.best, "best_bits": r.best_bits, "best_stops": r.best_stops, "bits": list(r.bits), "stops": list(r.stops),
            "sentences_ok": list(r.sentences_ok), "matches": list(r.matches), "printable": list(r.printable)}


def _estimate(e) -> dict:
    return {"baud": e.baud, "nominal": e.nominal, "rho": e.rho, "rho_max": e.rho_max, "samples": e.samples, "edges": e.edges, "k": e.k,
            "settled": bool(e.settled), "valid": bool(e.valid)}


def _probe_state(h, cand) -> dict:
    """A stream's raw accumulators as numpy arrays: what the parity tests compare integer for integer."""
    out = {k: cand[k].copy() for k in ("P", "Q", "NB", "re", "im", "n", "cur_block")}
    out.update(samples=int(h.samples), edges=np.array(list(h.edges), np.uint64), history=np.array(list(h.history), np.uint64),
               majority=np.array(list(h.majority), np.uint32))
    return out


def _rows(rows, S, n_per_stream, dtype):
    """rows: dtype [S, stride] (or [n] for one stream); n_per_stream: None = every row whole."""
    rows = np.ascontiguousarray(rows, dtype=dtype)
    if rows.ndim == 1:
        rows = rows[None, :]
    assert rows.shape[0] == S, rows.shape
    n = np.full(S, rows.shape[1], np.uint32) if n_per_stream is None else np.ascontiguousarray(n_per_stream, dtype=np.uint32)
    assert n.shape == (S,) and (S == 1 or int(n.max(initial=0)) <= rows.shape[1])
    return rows, n


class _RowObject(_Handle):
    """What BaudProbe, Clocked, Tones and ToneSearch share: made from an engine and a parameter struct, one row per stream through three doors, reset.
    _prefix names the symbols (hd_clocked -> hd_clocked_create, hd_clocked_params, ...); _ints: the parameters that are integers (_params).  The rows
    are float32 discriminator output here and complex64 decimated IQ in _IqRowObject."""
    _prefix, _ints, _dtype = None, (), np.float32
    _destroy = property(lambda self: self._prefix + "_destroy")

    def __init__(self, eng: Engine, **params):
        self.S = eng.S
        p = _params(eng.L, getattr(capi, self._prefix + "_params"), self._prefix + "_params_default", params, self._ints)
        self._create(eng, self._prefix + "_create", C.byref(p))

    def _fn(self, name):
        return getattr(self.L, self._prefix + "_" + name)

    def reset(self, s=None):
        check(self._fn("reset")(self.h, 0xFFFFFFFF if s is None else s))

    def push_engine(self):
        """Add every stream's discriminator output of the call delivered last (drains the pipeline first, like the data getters)."""
        check(self._fn("push_engine")(self.h))

    def push_host(self, rows, n_per_stream=None):
        rows, n = _rows(rows, self.S, n_per_stream, self._dtype)
        check(self._fn("push_host")(self.h, rows.ctypes.data, rows.shape[1], n.ctypes.data, 0))

    def push_device(self, dev_ptr: int, stride: int, n_per_stream):
        """float32 rows at a device address, row s at dev_ptr + 4 * s * stride."""
        n = np.ascontiguousarray(n_per_stream, dtype=np.uint32)
        assert n.shape == (self.S,)
        check(self._fn("push_device")(self.h, dev_ptr, stride, n.ctypes.data, 0))


class _IqRowObject(_RowObject):
    """The cf32 objects: the same doors under the names and docstrings their public surface has (Tones and ToneSearch add their own push_engine text)."""
    _ints, _dtype = True, np.complex64

    def push_host(self, iq, n_per_stream=None):
        super().push_host(iq, n_per_stream)

    def push_device(self, dev_ptr: int, stride: int, n_per_stream):
        """cf32 rows at a device address, row s at dev_ptr + 8 * s * stride."""
        super().push_device(dev_ptr, stride, n_per_stream)


class BaudProbe(_RowObject):
    """Baud-rate probe of an engine's streams (hd_baud_probe_*, include/habdec_amd.h): push discriminator output, read an estimate."""
    _prefix = "hd_baud_probe"

    def estimate(self, s=0) -> dict:
        e = capi.hd_baud_estimate()
        check(self.L.hd_baud_probe_estimate(self.h, s, C.byref(e)))
        return _estimate(e)

    def state(self, s=0) -> dict:
        h, cand = capi.hd_baud_probe_stream_state(), np.zeros(capi.PROBE_CANDIDATES, capi.PROBE_CANDIDATE_DTYPE)
        n = self.L.hd_baud_probe_state(self.h, s, C.byref(h), cand.ctypes.data, cand.size)
        if n != capi.PROBE_CANDIDATES:
            check(n if n < 0 else -1)
        return _probe_state(h, cand)


class HostBaudProbe(_Handle):
    """One stream of the probe in plain C++ on the host (hd_host_baud_probe_*): the restatement the kernel is held to, no GPU."""
    _destroy = "hd_host_baud_probe_free"

    def __init__(self, decimated_rate: float, **params):
        self.L = lib()
        p = _params(self.L, capi.hd_baud_probe_params, "hd_baud_probe_params_default", params)
        self.h = self.L.hd_host_baud_probe_new(float(decimated_rate), C.byref(p))
        if not self.h:
            raise HabdecError("hd_host_baud_probe_new: 0 < baud_lo < baud_hi <= decimated_rate / 3.5 and min_coherence >= 0")

    def push(self, d):
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1)
        self.L.hd_host_baud_probe_push(self.h, d, d.size)

    def reset(self):
        self.L.hd_host_baud_probe_reset(self.h)

    def estimate(self) -> dict:
        e = capi.hd_baud_estimate()
        check(self.L.hd_host_baud_probe_estimate(self.h, C.byref(e)))
        return _estimate(e)

    def state(self) -> dict:
        h, cand = capi.hd_baud_probe_stream_state(), np.zeros(capi.PROBE_CANDIDATES, capi.PROBE_CANDIDATE_DTYPE)
        n = self.L.hd_host_baud_probe_state(self.h, C.byref(h), cand.ctypes.data, cand.size)
        assert n == capi.PROBE_CANDIDATES, n
        return _probe_state(h, cand)


def _clocked_counters(c) -> dict:
    return {k: int(getattr(c, k)) for k, _ in capi.hd_clocked_counters._fields_}


def _clocked_sentences(a) -> list:
    """[(pos, flips, 'callsign,data*CRC')]"""
    return [(int(r["pos"]), int(r["flips"]), r["text"].decode("latin-1")) for r in a]


class Clocked(_RowObject):
    """Clocked soft-decision decoder of an engine's streams (hd_clocked_*, include/habdec_amd.h): push discriminator output, take records and sentences."""
    _prefix, _ints = "hd_clocked", True

    def set_modem(self, s, baud, bits, stops, invert=False):
        """Give stream s its modem (resets the stream)."""
        check(self.L.hd_clocked_set_modem(self.h, s, float(baud), int(bits), int(stops), int(invert)))

    def push_tones(self, tones: "Tones"):
        """Add the rows of the tone-filter demodulator's last push (hd_tones_rows), read in place in device memory."""
        self.push_device(*tones.rows())

    def waiting(self, s=0) -> int:
        n = self.L.hd_clocked_records(self.h, s, None, 0)
        check(min(n, 0))
        return n

    def records(self, s=0, cap=None) -> np.ndarray:
        """Take the stream's waiting records (at most cap), oldest first: an array of capi.CLOCKED_RECORD_DTYPE."""
        out = np.zeros(self.waiting(s) if cap is None else cap, capi.CLOCKED_RECORD_DTYPE)
        n = self.L.hd_clocked_records(self.h, s, out.ctypes.data, out.size) if out.size else 0
        check(min(n, 0))
        return out[:n]

    def take_sentences(self, s=0, cap=64) -> list:
        out = np.zeros(cap, capi.CLOCKED_SENTENCE_DTYPE)
        n = self.L.hd_clocked_take_sentences(self.h, s, out.ctypes.data, out.size)
        check(min(n, 0))
        return _clocked_sentences(out[:n])

    def stats(self, s=0) -> dict:
        c = capi.hd_clocked_counters()
        check(self.L.hd_clocked_stats(self.h, s, C.byref(c)))
        return _clocked_counters(c)


class HostClocked(_Handle):
    """One stream of the clocked decoder in plain C++ on the host (hd_host_clocked_*): the restatement the kernel is held to, no GPU."""
    _destroy = "hd_host_clocked_free"

    def __init__(self, decimated_rate: float, baud=None, bits=8, stops=2, invert=False, **params):
        self.L = lib()
        p = _params(self.L, capi.hd_clocked_params, "hd_clocked_params_default", params, True)
        self.h = self.L.hd_host_clocked_new(float(decimated_rate), C.byref(p))
        if not self.h:
            raise HabdecError("hd_host_clocked_new: 16 <= record_cap <= 2^20, repair_bits <= 16, repair_flips <= 4, decimated_rate > 0")
        if baud is not None:
            self.set_modem(baud, bits, stops, invert)

    def set_modem(self, baud, bits, stops, invert=False):
        rc = self.L.hd_host_clocked_set_modem(self.h, float(baud), int(bits), int(stops), int(invert))
        if rc:
            raise HabdecError("hd_host_clocked_set_modem: %d (3.5 <= samples per bit <= 2048, 7 or 8 data bits, 1 or 2 stop bits)" % rc)

    def reset(self):
        self.L.hd_host_clocked_reset(self.h)

    def push(self, d):
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1)
        self.L.hd_host_clocked_push(self.h, d, d.size)

    def waiting(self) -> int:
        return self.L.hd_host_clocked_records(self.h, None, 0)

    def records(self, cap=None) -> np.ndarray:
        out = np.zeros(self.waiting() if cap is None else cap, capi.CLOCKED_RECORD_DTYPE)
        n = self.L.hd_host_clocked_records(self.h, out.ctypes.data, out.size) if out.size else 0
        return out[:n]

    def take_sentences(self, cap=64) -> list:
        out = np.zeros(cap, capi.CLOCKED_SENTENCE_DTYPE)
        n = self.L.hd_host_clocked_take_sentences(self.h, out.ctypes.data, out.size)
        return _clocked_sentences(out[:n])

    def stats(self) -> dict:
        c = capi.hd_clocked_counters()
        check(self.L.hd_host_clocked_stats(self.h, C.byref(c)))
        return _clocked_counters(c)


def _tones_info(i) -> dict:
    return {k: int(getattr(i, k)) for k, _ in capi.hd_tones_info._fields_}


class Tones(_IqRowObject):
    """Tone-filter demodulator of an engine's streams (hd_tones_*, include/habdec_amd.h): push decimated IQ, get one float row per stream in device memory
    for Clocked.push_tones or BaudProbe.push_device."""
    _prefix = "hd_tones"

    def set_modem(self, s, baud, f_hi, f_lo):
        """Give stream s its modem (resets the stream); baud 0: the engine stream's."""
        check(self.L.hd_tones_set_modem(self.h, s, float(baud), float(f_hi), float(f_lo)))

    def set_modem_from_afc(self, s, baud=0.0):
        check(self.L.hd_tones_set_modem_from_afc(self.h, s, float(baud)))

    def push_engine(self):
        """Demodulate every stream's decimated IQ of the call delivered last (drains the pipeline first, like the data getters)."""
        super().push_engine()

    def rows(self):
        """(device address of row 0, stride in floats, the rows' lengths) of the last push: valid until the next push or reset."""
        ptr, stride, n = C.c_void_p(), C.c_size_t(), np.zeros(self.S, np.uint32)
        check(self.L.hd_tones_rows(self.h, C.byref(ptr), C.byref(stride), n.ctypes.data))
        return ptr.value, stride.value, n

    def output(self, s=0) -> np.ndarray:
        """A host copy of stream s's row of the last push."""
        n = self.L.hd_tones_output(self.h, s, None, 0)
        check(min(n, 0))
        out = np.zeros(n, np.float32)
        if n:
            check(min(self.L.hd_tones_output(self.h, s, out.ctypes.data, out.size), 0))
        return out

    def stats(self, s=0) -> dict:
        i = capi.hd_tones_info()
        check(self.L.hd_tones_stats(self.h, s, C.byref(i)))
        return _tones_info(i)


class HostTones(_Handle):
    """One stream of the tone-filter demodulator in plain C++ on the host (hd_host_tones_*): the restatement the kernel is held to, no GPU."""
    _destroy = "hd_host_tones_free"

    def __init__(self, decimated_rate: float, baud=None, f_hi=None, f_lo=None, **params):
        self.L = lib()
        p = _params(self.L, capi.hd_tones_params, "hd_tones_params_default", params, True)
        self.h = self.L.hd_host_tones_new(float(decimated_rate), C.byref(p))
        if not self.h:
            raise HabdecError("hd_host_tones_new: decimated_rate > 0")
        if baud is not None:
            self.set_modem(baud, f_hi, f_lo)

    def set_modem(self, baud, f_hi, f_lo):
        rc = self.L.hd_host_tones_set_modem(self.h, float(baud), float(f_hi), float(f_lo))
        if rc:
            raise HabdecError("hd_host_tones_set_modem: %d (3.5 <= samples per bit <= 2048, 32 <= window_q8 <= 256; |tone| < rate / 2, f_hi above f_lo)" % rc)

    def reset(self):
        self.L.hd_host_tones_reset(self.h)

    def push(self, iq) -> np.ndarray:
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        out = np.zeros(iq.size, np.float32)
        n = self.L.hd_host_tones_push(self.h, iq.ctypes.data, iq.size, out.ctypes.data) if iq.size else 0
        return out[:n]

    def stats(self) -> dict:
        i = capi.hd_tones_info()
        check(self.L.hd_host_tones_stats(self.h, C.byref(i)))
        return _tones_info(i)


def fir_demod_lds_bytes(taps: int) -> tuple:
    """(dynamic, static) LDS bytes of a low-pass launch whose longest filter has `taps` taps (hd_host_fir_demod_lds_bytes; no GPU)."""
    st = C.c_size_t(0)
    return int(lib().hd_host_fir_demod_lds_bytes(int(taps), C.byref(st))), int(st.value)


def fir_demod_max_taps(lds_bytes: int) -> int:
    """The largest odd tap count whose low-pass launch fits `lds_bytes` of LDS, 0 if none does (hd_host_fir_demod_max_taps; no GPU)."""
    return int(lib().hd_host_fir_demod_max_taps(int(lds_bytes)))


def _tone_search_detect_params(L, params):
    return _params(L, capi.hd_tone_search_detect_params, "hd_tone_search_detect_params_default", params)


def _tone_search_result(r) -> dict:
    return {k: getattr(r, k) for k, _ in capi.hd_tone_search_result._fields_}


def tone_search_detect(power: np.ndarray, segments: int, fsd: float, **params) -> dict:
    """hd_host_tone_search_detect on a 4096-bin averaged power spectrum (no GPU): the result as a dict (f_hi_hz and f_lo_hz are what Tones.set_modem
    takes); params as hd_tone_search_detect_params, baud required."""
    L = lib()
    power = np.ascontiguousarray(power, np.float64)
    assert power.shape == (4096,), power.shape
    p, r = _tone_search_detect_params(L, params), capi.hd_tone_search_result()
    rc = L.hd_host_tone_search_detect(power.ctypes.data, int(segments), float(fsd), C.byref(p), C.byref(r))
    if rc:
        raise HabdecError(f"habdec_amd error {rc}: hd_host_tone_search_detect")
    return _tone_search_result(r)


class ToneSearch(_IqRowObject):
    """Long-averaged power spectrum of every stream's decimated IQ and the two-tone detector on top of it (hd_tone_search_*, include/habdec_amd.h)."""
    _prefix = "hd_tone_search"

    def push_engine(self):
        """Take every stream's decimated IQ of the call delivered last (drains the pipeline first, like the data getters)."""
        super().push_engine()

    def power(self, s=0):
        """(float64[4096], segments) of stream s: p[k] belongs to (k - 2048) * decimated rate / 4096."""
        return _power(self.L.hd_tone_search_power, self.h, s)

    def stats(self, s=0) -> dict:
        i = capi.hd_tone_search_info()
        check(self.L.hd_tone_search_stats(self.h, s, C.byref(i)))
        return {"samples": int(i.samples), "segments": int(i.segments), "carry": int(i.carry)}

    def detect(self, s=0, **params) -> dict:
        """The stream's two tones as a dict; params as hd_tone_search_detect_params, baud required."""
        p, r = _tone_search_detect_params(self.L, params), capi.hd_tone_search_result()
        check(self.L.hd_tone_search_detect(self.h, s, C.byref(p), C.byref(r)))
        return _tone_search_result(r)


class HostToneSearch(_Handle):
    """One stream of the tone search's spectrum in plain C++ on the host (hd_host_tone_search_*): double-precision transform, no GPU."""
    _destroy = "hd_host_tone_search_destroy"

    def __init__(self):
        self.L = lib()
        self.h = self.L.hd_host_tone_search_create()

    def reset(self):
        self.L.hd_host_tone_search_reset(self.h)

    def push(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        if iq.size:
            self.L.hd_host_tone_search_push(self.h, iq.ctypes.data, iq.size)

    def power(self):
        return _power(self.L.hd_host_tone_search_power, self.h, host="hd_host_tone_search_power")

    def detect(self, fsd, **params) -> dict:
        p, seg = self.power()
        return tone_search_detect(p, seg, fsd, **params)


def chase_repair(span: str, data, nbits=8, repair_bits=8, repair_flips=3):
    """hd_host_chase_repair: (repaired span, flips) or None.  data: int32 [len(span), 8], the data_k of every character."""
    L = lib()
    b = span.encode("latin-1")
    data = np.ascontiguousarray(data, dtype=np.int32)
    assert data.shape == (len(b), 8), data.shape
    out, flips = C.create_string_buffer(len(b) + 1), C.c_uint32(0)
    rc = L.hd_host_chase_repair(b, len(b), data.ctypes.data, nbits, repair_bits, repair_flips, out, C.byref(flips))
    check(min(rc, 0))
    return (out.raw[:len(b)].decode("latin-1"), flips.value) if rc == 1 else None


class HostFormatTrial(_Handle):
    """Four text stages (7N1, 7N2, 8N1, 8N2) over the same bits on the host (hd_host_format_trial_*)."""
    _destroy = "hd_host_format_trial_free"

    def __init__(self):
        self.L = lib()
        self.h = self.L.hd_host_format_trial_new()

    def push_bits(self, bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
        self.L.hd_host_format_trial_push_bits(self.h, bits, bits.size)

    def get(self) -> dict:
        r = capi.hd_format_trial_result()
        self.L.hd_host_format_trial_get(self.h, C.byref(r))
        return _trial_result(r)


def _candidates(out, n) -> list:
    return [{"offset_hz": c.offset_hz, "snr_db": c.snr_db, "width_hz": c.width_hz, "bin_lo": c.bin_lo, "bin_hi": c.bin_hi} for c in out[:n]]


def survey_detect(power: np.ndarray, segments: int, sampling_rate: float, cap: int = 64, **params) -> list:
    """hd_host_survey_detect on a 4096-bin averaged power spectrum (no GPU): candidates as dicts, strongest first; params as hd_survey_params."""
    L = lib()
    p, power = _params(L, capi.hd_survey_params, "hd_survey_params_default", params), np.ascontiguousarray(power, np.float64)

    def call(out, cap, found):
        rc = L.hd_host_survey_detect(power, int(segments), float(sampling_rate), C.byref(p), out, cap, found)
        if rc:
            raise HabdecError(f"habdec_amd error {rc}: hd_host_survey_detect")
    return _with_cap(call, cap, capi.hd_survey_candidate, _candidates)


class _WidebandObject(_Handle):
    """What Survey and Waterfall share: full-rate IQ through two doors (hd_<_prefix>_push_device / _push_host and their _fmt forms), reset."""
    _prefix = None
    _destroy = property(lambda self: self._prefix + "_destroy")

    def _push_device(self, dev_ptr, n, fmt):
        if fmt is not None:
            check(getattr(self.L, self._prefix + "_push_device_fmt")(self.h, capi.iq_fmt(fmt), dev_ptr, n))
            return
        check(getattr(self.L, self._prefix + "_push_device")(self.h, dev_ptr, n))

    def _push_host(self, iq, fmt):
        if fmt is not None and capi.iq_fmt(fmt) != capi.IQ_CF32:
            fmt = capi.iq_fmt(fmt)
            iq = np.ascontiguousarray(iq).reshape(-1)
            if fmt in capi.IQ_DTYPES and iq.dtype != capi.IQ_DTYPES[fmt]:
                raise HabdecError(f"IQ format {fmt} wants dtype {capi.IQ_DTYPES[fmt]}, not {iq.dtype}")
            check(getattr(self.L, self._prefix + "_push_host_fmt")(self.h, fmt, iq.ctypes.data, iq.size // 2))
            return
        iq = np.ascontiguousarray(iq, dtype=np.complex64).reshape(-1)
        check(getattr(self.L, self._prefix + "_push_host")(self.h, iq.ctypes.data, iq.size))

    def reset(self):
        check(getattr(self.L, self._prefix + "_reset")(self.h))


class Survey(_WidebandObject):
    """Welch-averaged power spectrum of full-rate IQ and the payload detector on top of it (hd_survey_*, include/habdec_amd.h)."""
    _prefix = "hd_survey"

    def __init__(self, eng: Engine):
        self._create(eng, "hd_survey_create")

    def push_device(self, dev_ptr: int, n: int, fmt=None):
        """n cf32 samples at a device address; the buffer must stay valid until power() / detect() / reset() has returned.
        fmt: n packed samples (hd_survey_push_device_fmt); the buffer is the caller's again on return."""
        self._push_device(dev_ptr, n, fmt)

    def push_host(self, iq: np.ndarray, fmt=None):
        """fmt: iq is packed, an integer array [n, 2] (or flat, I then Q) of the format's dtype (hd_survey_push_host_fmt)."""
        self._push_host(iq, fmt)

    def power(self):
        """(float64[4096], segments): p[i] belongs to (i - 2048) * sampling_rate / 4096."""
        return _power(self.L.hd_survey_power, self.h)

    def detect(self, cap: int = 64, **params) -> list:
        """Candidates as dicts (offset_hz is what Engine.set_front_tune takes), strongest first; params as hd_survey_params."""
        p = _params(self.L, capi.hd_survey_params, "hd_survey_params_default", params)
        return _with_cap(lambda out, cap, found: check(self.L.hd_survey_detect(self.h, C.byref(p), out, cap, found)), cap, capi.hd_survey_candidate, _candidates)


def _tracks(out, n) -> list:
    keys = ("first_sample", "end_sample", "first_row", "last_row", "marks", "offset_hz", "width_hz", "rows_hit", "bin_lo", "bin_hi", "open")
    return [{k: getattr(t, k) for k in keys} for t in out[:n]]


def _track_params(L, params):
    return _params(L, capi.hd_waterfall_track_params, "hd_waterfall_track_params_default", params, ("gap_rows", "min_rows"))


def waterfall_tracks(headers: np.ndarray, marks: np.ndarray, sampling_rate: float, cap: int = 64, **params) -> list:
    """hd_host_waterfall_tracks over headers (capi.WATERFALL_ROW_DTYPE [n]) and marks (uint32 [n, 128]) (no GPU): tracks as dicts, ordered by
    first_sample, then offset_hz; params as hd_waterfall_track_params."""
    L = lib()
    p = _track_params(L, params)
    headers = np.ascontiguousarray(headers, capi.WATERFALL_ROW_DTYPE)
    marks = np.ascontiguousarray(marks, np.uint32).reshape(len(headers), capi.WATERFALL_WORDS)

    def call(out, cap, found):
        rc = L.hd_host_waterfall_tracks(headers.ctypes.data, marks.ctypes.data, len(headers), float(sampling_rate), C.byref(p), out, cap, found)
        if rc:
            raise HabdecError(f"habdec_amd error {rc}: hd_host_waterfall_tracks")
    return _with_cap(call, cap, capi.hd_waterfall_track, _tracks)


class Waterfall(_WidebandObject):
    """The survey's rows over time, the per-row detector on the GPU and the tracks on top of its marks (hd_waterfall_*, include/habdec_amd.h)."""
    _prefix = "hd_waterfall"

    def __init__(self, eng: Engine, **params):
        self.params = _params(eng.L, capi.hd_waterfall_params, "hd_waterfall_params_default", params, ("slot_segments", "rows_cap"))
        self._create(eng, "hd_waterfall_create", C.byref(self.params))

    def push_device(self, dev_ptr: int, n: int, fmt=None):
        """n cf32 samples at a device address, or with fmt n packed ones; returns when the new rows' headers and marks are on the host."""
        self._push_device(dev_ptr, n, fmt)

    def push_host(self, iq: np.ndarray, fmt=None):
        """fmt: iq is packed, an integer array [n, 2] (or flat, I then Q) of the format's dtype (hd_waterfall_push_host_fmt)."""
        self._push_host(iq, fmt)

    def push_rows(self, rows, segments, n_rows: int | None = None):
        """Rows of float sums made elsewhere: a float32 array [n, 4096] with segments [n], or a device address with n_rows (hd_waterfall_push_rows)."""
        seg = np.ascontiguousarray(segments, np.uint32).reshape(-1)
        if isinstance(rows, int):
            check(self.L.hd_waterfall_push_rows(self.h, rows, seg.ctypes.data, len(seg) if n_rows is None else n_rows, 1))
            return
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 4096)
        assert len(rows) == len(seg), (rows.shape, seg.shape)
        check(self.L.hd_waterfall_push_rows(self.h, rows.ctypes.data, seg.ctypes.data, len(rows), 0))

    def rows_total(self) -> int:
        return int(self.L.hd_waterfall_rows_total(self.h))

    def _range(self, first, n):
        return (first, self.rows_total() - first) if n is None else (first, n)

    def headers(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """A structured array (capi.WATERFALL_ROW_DTYPE) of rows [first, first + n); n = None: all from `first` on."""
        first, n = self._range(first, n)
        out = np.zeros(max(n, 0), capi.WATERFALL_ROW_DTYPE)
        check(self.L.hd_waterfall_headers(self.h, first, n, out.ctypes.data))
        return out

    def marks(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """uint32 [n, 128]: bit i & 31 of word i >> 5 is bin i."""
        first, n = self._range(first, n)
        out = np.zeros((max(n, 0), capi.WATERFALL_WORDS), np.uint32)
        check(self.L.hd_waterfall_marks(self.h, first, n, out.ctypes.data))
        return out

    def marks_bool(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """bool [n, 4096]"""
        m = self.marks(first, n)
        return ((m[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(len(m), 4096)

    def rows(self, first: int, n: int, normalised: bool = False) -> np.ndarray:
        """float32 [n, 4096] raw sums of rows still in the ring; normalised: float64, divided by segments * sum w^2 (the survey's scale)."""
        out = np.zeros((n, 4096), np.float32)
        check(self.L.hd_waterfall_rows(self.h, first, n, out.ctypes.data))
        if not normalised:
            return out
        w = np.zeros(4096, np.float32)
        self.L.hd_host_survey_window(w)
        return out.astype(np.float64) / (self.headers(first, n)["segments"].astype(np.float64)[:, None] * float(np.sum(w.astype(np.float64) ** 2)))

    def hits(self):
        """(uint32[4096], rows_counted)"""
        h, k = np.zeros(4096, np.uint32), C.c_uint64(0)
        check(self.L.hd_waterfall_hits(self.h, h.ctypes.data, C.byref(k)))
        return h, int(k.value)

    def tracks(self, cap: int = 64, **params) -> list:
        """Tracks as dicts (offset_hz is what Engine.set_front_tune takes); params as hd_waterfall_track_params."""
        p = _track_params(self.L, params)
        return _with_cap(lambda out, cap, found: check(self.L.hd_waterfall_tracks(self.h, C.byref(p), out, cap, found)), cap, capi.hd_waterfall_track, _tracks)


class IqFiles(_Handle):
    """Batched IQ file source (hd_host_iqfiles_*): one IQSource_File-like reader per stream, read in lock step; cf32 files, or packed ones with fmt=."""
    _destroy = "hd_host_iqfiles_close"

    def __init__(self, paths, chunk: int, granule: int, loop: bool = False, realtime_rate: float = 0.0, fmt=None):
        self.L = lib()
        arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
        self.fmt = capi.IQ_CF32 if fmt is None else capi.iq_fmt(fmt)
        self.h = self.L.hd_host_iqfiles_open_fmt(arr, len(paths), int(loop), chunk, granule, realtime_rate, self.fmt)
        if not self.h:
            raise HabdecError("hd_host_iqfiles_open failed (missing file, chunk < granule, unknown format, ...)")
        self.S, self.chunk = len(paths), chunk

    def count(self, s: int) -> int: return int(self.L.hd_host_iqfiles_count(self.h, s))
    def rewinds(self, s: int) -> int: return int(self.L.hd_host_iqfiles_rewinds(self.h, s))

    def next(self, stride: int | None = None):
        """One round: returns (slab complex64 [S, stride], n_per_stream uint32 [S], streams that read anything)."""
        stride = stride or self.chunk
        slab = np.zeros((self.S, stride), np.complex64)
        n = np.zeros(self.S, np.uint32)
        alive = self.L.hd_host_iqfiles_next(self.h, slab.view(np.float32), stride, n.ctypes.data_as(C.POINTER(C.c_uint32)))
        return slab, n, int(alive)

    def next_raw(self, stride: int | None = None):
        """One round in the files' own bytes: (slab [S, stride, 2] of the format's dtype, n_per_stream, streams that read anything)."""
        stride = stride or self.chunk
        slab = np.zeros((self.S, stride, 2), capi.IQ_DTYPES[self.fmt])
        n = np.zeros(self.S, np.uint32)
        alive = self.L.hd_host_iqfiles_next_raw(self.h, slab.ctypes.data, stride, n.ctypes.data_as(C.POINTER(C.c_uint32)))
        return slab, n, int(alive)
