"""SSDV packets (hd_ssdv_*, include/habdec_amd.h): bytes with a confidence each in, whole Reed-Solomon-corrected 256-byte packets out.

    from habdec_amd.ssdv import Ssdv, HostSsdv, make_packet, encode

Ssdv is a side object of an Engine like Clocked and Combiner; HostSsdv is one stream of it in plain C++ on the host, no GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import HabdecError, check, lib
from .engine import Engine, _Handle, _params


def _packets(a) -> list:
    """One dict per packet: the fields of hd_ssdv_packet, callsign as str, data as bytes."""
    out = []
    for r in a:
        d = {k: int(r[k]) for k in capi.SSDV_PACKET_DTYPE.names if k not in ("callsign", "data")}
        d["callsign"], d["data"] = r["callsign"].decode("latin-1"), r["data"].tobytes()
        out.append(d)
    return out


def _counters(c) -> dict:
    d = {k: int(getattr(c, k)) for k, _ in capi.hd_ssdv_counters._fields_ if k != "packets"}
    d["packets"] = [int(v) for v in c.packets]
    return d


def _bytes_conf(b, conf):
    b = np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
    b = np.ascontiguousarray(b)
    if conf is not None:
        conf = np.ascontiguousarray(conf, dtype=np.uint32).reshape(-1)
        assert conf.size == b.size, (conf.size, b.size)
    return b, conf


def _records(r):
    r = np.ascontiguousarray(r, dtype=capi.CLOCKED_RECORD_DTYPE).reshape(-1)
    return r


def encode(data223) -> bytes:
    """The 32 parity bytes of 223 data bytes (bytes 224 .. 255 of a packet)."""
    d = np.frombuffer(bytes(data223), np.uint8)
    assert d.size == 223, d.size
    out = np.zeros(32, np.uint8)
    lib().hd_host_ssdv_encode(d.ctypes.data, out.ctypes.data)
    return out.tobytes()


def make_packet(payload, type=0x66, callsign="", image_id=0, packet_id=0, width=0, height=0, flags=0, mcu_offset=0, mcu_index=0) -> bytes:
    """A whole 256-byte packet around 205 payload bytes: sync, header, CRC-32, parity (type 0x67, no-FEC: zeros in place of the parity)."""
    d = np.frombuffer(bytes(payload), np.uint8)
    assert d.size == 205, d.size
    out = np.zeros(256, np.uint8)
    lib().hd_host_ssdv_make_packet(int(type), callsign.encode("ascii"), int(image_id), int(packet_id), int(width), int(height), int(flags), int(mcu_offset),
                                   int(mcu_index), d.ctypes.data, out.ctypes.data)
    return out.tobytes()


class Ssdv(_Handle):
    """SSDV packet receiver of an engine's streams: push bytes or the clocked decoder's records, scan on the GPU, take packets.  Closed with its engine, in
    front of it."""
    _destroy = "hd_ssdv_destroy"

    def __init__(self, eng: Engine, **params):
        self.S = eng.S
        p = _params(eng.L, capi.hd_ssdv_params, "hd_ssdv_params_default", params, True)
        self._create(eng, "hd_ssdv_create", C.byref(p))
        eng._own(self)

    def reset(self, s=None):
        check(self.L.hd_ssdv_reset(self.h, 0xFFFFFFFF if s is None else s))

    def push_bytes(self, s, b, conf=None):
        """Append bytes (and their confidences, 0 .. 0xFFFFFF; None: all 0xFFFFFF) to stream s.  Nothing is decoded before scan()."""
        b, conf = _bytes_conf(b, conf)
        check(self.L.hd_ssdv_push_bytes(self.h, s, b.ctypes.data, None if conf is None else conf.ctypes.data, b.size))

    def push_records(self, s, records, char_len):
        """Append the clocked decoder's records (capi.CLOCKED_RECORD_DTYPE) with the gap rule at char_len samples per character (0: off)."""
        r = _records(records)
        check(self.L.hd_ssdv_push_records(self.h, s, r.ctypes.data, r.size, int(char_len)))

    def push_clocked(self, clocked):
        """Take every 8-bit stream's waiting records off the clocked decoder, push them and scan."""
        check(self.L.hd_ssdv_push_clocked(self.h, clocked.h))

    def scan(self):
        check(self.L.hd_ssdv_scan(self.h))

    def waiting(self, s=0) -> int:
        n = self.L.hd_ssdv_take_packets(self.h, s, None, 0)
        check(min(n, 0))
        return n

    def take_packets(self, s=0, cap=None) -> list:
        out = np.zeros(self.waiting(s) if cap is None else cap, capi.SSDV_PACKET_DTYPE)
        n = self.L.hd_ssdv_take_packets(self.h, s, out.ctypes.data, out.size) if out.size else 0
        check(min(n, 0))
        return _packets(out[:n])

    def stats(self, s=0) -> dict:
        c = capi.hd_ssdv_counters()
        check(self.L.hd_ssdv_stats(self.h, s, C.byref(c)))
        return _counters(c)

    # ---- the library's test hooks (not part of the ABI)

    def debug_guards(self, s) -> int:
        """How many guard words around stream s's ring, the counters and the results are damaged."""
        f = self.L.hd_debug_ssdv_guards
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32]
        return f(self.h, s)


class HostSsdv(_Handle):
    """One stream of the SSDV receiver in plain C++ on the host (hd_host_ssdv_*): the restatement the kernel is held to, no GPU.  Every push scans."""
    _destroy = "hd_host_ssdv_destroy"

    def __init__(self, **params):
        self.L = lib()
        p = _params(self.L, capi.hd_ssdv_params, "hd_ssdv_params_default", params, True)
        self.h = self.L.hd_host_ssdv_create(C.byref(p))
        if not self.h:
            raise HabdecError("hd_host_ssdv_create: max_fill <= 64")

    def reset(self):
        self.L.hd_host_ssdv_reset(self.h)

    def push_bytes(self, b, conf=None):
        b, conf = _bytes_conf(b, conf)
        check(self.L.hd_host_ssdv_push_bytes(self.h, b.ctypes.data, None if conf is None else conf.ctypes.data, b.size))

    def push_records(self, records, char_len):
        r = _records(records)
        check(self.L.hd_host_ssdv_push_records(self.h, r.ctypes.data, r.size, int(char_len)))

    def take_packets(self, cap=None) -> list:
        out = np.zeros(self.L.hd_host_ssdv_take_packets(self.h, None, 0) if cap is None else cap, capi.SSDV_PACKET_DTYPE)
        n = self.L.hd_host_ssdv_take_packets(self.h, out.ctypes.data, out.size) if out.size else 0
        return _packets(out[:n])

    def stats(self) -> dict:
        c = capi.hd_ssdv_counters()
        check(self.L.hd_host_ssdv_stats(self.h, C.byref(c)))
        return _counters(c)
