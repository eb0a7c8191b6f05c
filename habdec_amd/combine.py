"""Diversity combiner (hd_combine_*, include/habdec_amd.h): several receivers of one payload, aligned and summed into one row for the clocked decoder.

    from habdec_amd.combine import Combiner, HostCombiner

Combiner is a side object of an Engine like Tones and Clocked; HostCombiner is one group of it in plain C++ on the host, no GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import HabdecError, check, lib
from .engine import Engine, _Handle, _params, _RowObject


def _lag_params(L, guard, kw):
    return _params(L, capi.hd_combine_lag_params, "hd_combine_lag_params_default", dict(kw, guard=guard), True)


def _lags(a) -> list:
    """[{stream, lag, peak, second, valid}]"""
    return [dict(stream=int(r["stream"]), lag=int(r["lag"]), peak=int(r["peak"]), second=int(r["second"]), valid=bool(r["valid"])) for r in a]


def _info(i) -> dict:
    return {k: int(getattr(i, k)) for k, _ in capi.hd_combine_info._fields_}


class Combiner(_RowObject):
    """Diversity combiner of an engine's streams: push one float row per stream (the tones' rows above all), get one summed row per group in device memory
    for Clocked.push_device.  Closed with its engine, in front of it."""
    _prefix, _ints = "hd_combine", True

    def __init__(self, eng: Engine, **params):
        super().__init__(eng, **params)
        eng._own(self)

    def set_group(self, streams):
        """A group of 1 to 8 distinct streams, the reference first (resets its members)."""
        a = np.ascontiguousarray(streams, dtype=np.uint32).reshape(-1)
        check(self.L.hd_combine_set_group(self.h, a.ctypes.data, a.size))

    def dissolve(self, ref):
        a = np.array([ref], np.uint32)
        check(self.L.hd_combine_set_group(self.h, a.ctypes.data, 0))

    def set_delay(self, s, delay):
        check(self.L.hd_combine_set_delay(self.h, s, int(delay)))

    def set_weight(self, s, weight):
        check(self.L.hd_combine_set_weight(self.h, s, int(weight)))

    def push_tones(self, tones):
        """Add the rows of the tone-filter demodulator's last push (hd_tones_rows), read in place in device memory."""
        self.push_device(*tones.rows())

    def rows(self):
        """(device address of row 0, stride in floats, the rows' lengths) of the last push: what Clocked.push_device takes."""
        ptr, stride, n = C.c_void_p(), C.c_size_t(), np.zeros(self.S, np.uint32)
        check(self.L.hd_combine_rows(self.h, C.byref(ptr), C.byref(stride), n.ctypes.data))
        return ptr.value, stride.value, n

    def output(self, s=0) -> np.ndarray:
        """A host copy of stream s's row of the last push (length 0 unless s is a group's reference)."""
        n = self.L.hd_combine_output(self.h, s, None, 0)
        check(min(n, 0))
        out = np.zeros(n, np.float32)
        if n:
            check(min(self.L.hd_combine_output(self.h, s, out.ctypes.data, out.size), 0))
        return out

    def stats(self, s=0) -> dict:
        i = capi.hd_combine_info()
        check(self.L.hd_combine_stats(self.h, s, C.byref(i)))
        return _info(i)

    def lags(self, ref, guard, **params) -> list:
        """The lag search of the group with reference ref: one entry per member, the reference's first."""
        out = np.zeros(capi.COMBINE_MAX_MEMBERS, capi.COMBINE_LAG_DTYPE)
        check(self.L.hd_combine_lags(self.h, ref, C.byref(_lag_params(self.L, guard, params)), out.ctypes.data, out.size))
        return _lags(out[:self.stats(ref)["members"]])

    def align(self, ref, guard, **params) -> list:
        """The search, then delays for the valid members and weight 0 for the others.  Reset the clocked decoder behind the combiner afterwards."""
        out = np.zeros(capi.COMBINE_MAX_MEMBERS, capi.COMBINE_LAG_DTYPE)
        n = self.L.hd_combine_align(self.h, ref, C.byref(_lag_params(self.L, guard, params)), out.ctypes.data, out.size)
        check(min(n, 0))
        return _lags(out[:self.stats(ref)["members"]])


    # ---- the library's test hooks (not part of the ABI)

    def debug_scores(self, s) -> np.ndarray:
        """Stream s's 2 L + 1 scores of the last search, lag -L first (empty where s was no member of it beside the reference)."""
        f = self.L.hd_debug_combine_scores
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]
        k = f(self.h, s, None, 0)
        check(min(k, 0))
        out = np.zeros(k, np.int32)
        if k:
            check(min(f(self.h, s, out.ctypes.data, out.size), 0))
        return out

    def debug_guards(self, s) -> int:
        """How many guard words around stream s's ring and row are damaged."""
        f = self.L.hd_debug_combine_guards
        f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_uint32]
        return f(self.h, s)


class HostCombiner(_Handle):
    """One group of the combiner in plain C++ on the host (hd_host_combine_*): the restatement the kernels are held to, no GPU.  Members are addressed by
    their position in the group."""
    _destroy = "hd_host_combine_destroy"

    def __init__(self, streams):
        self.L = lib()
        a = np.ascontiguousarray(streams, dtype=np.uint32).reshape(-1)
        self.count = a.size
        self.h = self.L.hd_host_combine_create(a.ctypes.data, a.size)
        if not self.h:
            raise HabdecError("hd_host_combine_create: 1 to 8 distinct streams")

    def _check(self, rc, what):
        if rc < 0:
            raise HabdecError(f"{what}: {rc}")
        return rc

    def set_delay(self, m, delay):
        self._check(self.L.hd_host_combine_set_delay(self.h, m, int(delay)), "hd_host_combine_set_delay (0 .. 8192)")

    def set_weight(self, m, weight):
        self._check(self.L.hd_host_combine_set_weight(self.h, m, int(weight)), "hd_host_combine_set_weight (0 .. 256)")

    def reset(self):
        self.L.hd_host_combine_reset(self.h)

    def push(self, rows) -> np.ndarray:
        """rows: float32 [members, n] (or [n] for a group of one); the combined row."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim == 1:
            rows = rows[None, :]
        assert rows.shape[0] == self.count, rows.shape
        out = np.zeros(rows.shape[1], np.float32)
        if out.size:
            self._check(self.L.hd_host_combine_push(self.h, rows.ctypes.data, rows.shape[1], None, rows.shape[1], out.ctypes.data), "hd_host_combine_push")
        return out

    def lags(self, guard, **params) -> list:
        out = np.zeros(self.count, capi.COMBINE_LAG_DTYPE)
        self._check(self.L.hd_host_combine_lags(self.h, C.byref(_lag_params(self.L, guard, params)), out.ctypes.data, out.size), "hd_host_combine_lags")
        return _lags(out)

    def align(self, guard, **params) -> list:
        out = np.zeros(self.count, capi.COMBINE_LAG_DTYPE)
        self._check(self.L.hd_host_combine_align(self.h, C.byref(_lag_params(self.L, guard, params)), out.ctypes.data, out.size), "hd_host_combine_align")
        return _lags(out)

    def scores(self, m) -> np.ndarray:
        """Member m's 2 L + 1 scores of the last search, lag -L first."""
        k = self._check(self.L.hd_host_combine_scores(self.h, m, None, 0), "hd_host_combine_scores")
        out = np.zeros(k, np.int32)
        if k:
            self.L.hd_host_combine_scores(self.h, m, out.ctypes.data, out.size)
        return out

    def stats(self, m=0) -> dict:
        i = capi.hd_combine_info()
        self._check(self.L.hd_host_combine_stats(self.h, m, C.byref(i)), "hd_host_combine_stats")
        return _info(i)
