"""Rates of packed IQ (hd_process_*_fmt, kernels/iq_unpack.hip): the unpack kernel beside a device-to-device copy, and the host-fed engine per format.

unpack:   1024 x 65536 samples of device-resident packed input into a cf32 slab, HIP events around the launch (hd_debug_iq_unpack_timed): the median of
          `timed` launches behind `warm` untimed ones, per format, ALTERNATING with a device-to-device copy of the kernel's own output size (512 MiB) in
          the same process.  The copy moves 16 bytes per sample, the kernel 10 (cs8, cu8) or 12 (cs16).  Criterion: the unpack takes no longer than the
          copy's median plus the copy's own max - min.
host:     hd_process_host_fmt against hd_process_host, samples/s per format beside cf32 on the same box, formats alternating, `rounds` rounds:
          1024 streams in batch mode from pageable memory (cfg4's shape), and 1 stream of a synchronous engine from hd_pinned_alloc memory (configs[0]).
          Expectation: up to 8 / bytes-per-sample times the cf32 rate until something other than the host link binds.  Beside each rate: the wall time
          of the calls themselves -- in batch mode a call returns when its copy and unpack have landed, so call time minus the unpack's time (above) is
          the copy's leg; from pinned memory of a synchronous engine there is no copy and the unpack reads over PCIe.
Usage: iq_format_rate.py [unpack|host|both] [warm=5] [timed=7] [rounds=5]"""
import ctypes as C
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import torch
import habdec_amd
from habdec_amd import capi

which = sys.argv[1] if len(sys.argv) > 1 else "both"
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 5
timed = int(sys.argv[3]) if len(sys.argv) > 3 else 7
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
FMTS = {"cs16": (capi.IQ_CS16, np.int16, 4), "cs8": (capi.IQ_CS8, np.int8, 2), "cu8": (capi.IQ_CU8, np.uint8, 2)}
FS, S, CH = 2.048e6, 1024, 65536


def unpack():
    eng = habdec_amd.Engine(n_streams=1, sampling_rate=FS, decimation=64)
    fn = eng.L.hd_debug_iq_unpack_timed
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                        C.POINTER(C.c_float)]
    src = torch.randint(0, 256, (S * CH * 4,), dtype=torch.uint8, device="cuda")
    dst = torch.zeros(S * CH * 2, dtype=torch.float32, device="cuda")
    other = torch.empty(S * CH * 2, dtype=torch.float32, device="cuda").normal_(0.0, 0.1)
    torch.cuda.synchronize()
    ms = C.c_float(0)
    for name, (code, _, bps) in FMTS.items():
        tk, tc = [], []
        for k in range(warm + timed):
            capi.check(fn(eng.h, code, src.data_ptr(), CH, None, CH, CH, S, dst.data_ptr(), CH, C.byref(ms)))
            tk.append(float(ms.value))
            capi.check(fn(eng.h, capi.IQ_CF32, other.data_ptr(), CH, None, CH, CH, S, dst.data_ptr(), CH, C.byref(ms)))
            tc.append(float(ms.value))
        k_, c_ = np.array(tk[warm:]), np.array(tc[warm:])
        km, cm, spread = float(np.median(k_)), float(np.median(c_)), float(c_.max() - c_.min())
        n = S * CH
        print(f"unpack {name}: median of {timed} behind {warm}: {km:.3f} ms (min {k_.min():.3f}, max {k_.max():.3f}) = {n / km / 1e6:.1f} GS/s, "
              f"{n * (bps + 8) / km / 1e9:.2f} TB/s of {bps + 8} B/sample | d2d copy of {n * 8 >> 20} MiB: {cm:.3f} ms (min {c_.min():.3f}, max {c_.max():.3f}) = "
              f"{n * 16 / cm / 1e9:.2f} TB/s | criterion unpack <= copy median + (max - min) = {cm + spread:.3f} ms: {'MET' if km <= cm + spread else 'MISSED'}",
              flush=True)
    eng.close()


def host_leg(label, eng, bufs, n_streams, calls):
    """bufs: name -> (array, push function); formats alternate within a round."""
    rates = {k: [] for k in bufs}
    call_ms = {k: [] for k in bufs}
    for name, (arr, push) in bufs.items():                # untimed: allocations, first-use slabs
        for _ in range(2):
            push(arr)
        eng.flush()
    for r in range(rounds):
        for name, (arr, push) in bufs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            per = []
            for _ in range(calls):
                c0 = time.perf_counter()
                push(arr)
                per.append(time.perf_counter() - c0)
            eng.flush()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / calls
            rates[name].append(n_streams * CH / dt)
            call_ms[name].append(1e3 * float(np.median(per)))
    base = float(np.median(rates["cf32"]))
    for name in bufs:
        bps = 8 if name == "cf32" else FMTS[name][2]
        med = float(np.median(rates[name]))
        print(f"host-fed {label} {name}: {med / 1e9:.3f} GS/s (rounds: " + " ".join(f"{v / 1e9:.3f}" for v in rates[name]) + f") = {med * bps / 1e9:.1f} GB/s of "
              f"packed bytes, {med / base:.2f} x cf32 (derived bound {8 / bps:.0f} x); median call {float(np.median(call_ms[name])):.2f} ms", flush=True)
    t = eng.timing()
    print(f"host-fed {label}: path {t['path']}, step_variant {t['step_variant']}, host_calls_in_place {t['host_calls_in_place']}", flush=True)


def host():
    rng = np.random.default_rng(1)
    # 1024 streams, batch mode, pageable memory
    eng = habdec_amd.Engine(n_streams=S, max_chunk=CH, sampling_rate=FS, decimation=64, baud=50, rtty_bits=7, rtty_stops=2, pipeline=1)
    bufs = {"cf32": ((rng.standard_normal((S, CH * 2), dtype=np.float32) * 0.2).view(np.complex64), lambda a: eng.process_host(a))}
    for name, (code, dt, bps) in FMTS.items():
        info = np.iinfo(dt)
        bufs[name] = (rng.integers(info.min, info.max + 1, size=(S, CH, 2), dtype=dt), lambda a: eng.process_host(a))
    host_leg("1024 streams, batch mode, pageable", eng, bufs, S, 4)
    eng.close()
    # 1 stream, synchronous, page-locked mapped memory (read in place)
    eng = habdec_amd.Engine(n_streams=1, max_chunk=CH, sampling_rate=FS, decimation=64)
    a = eng.pinned_array((1, CH), np.complex64)
    a[...] = (rng.standard_normal((1, CH * 2), dtype=np.float32) * 0.2).view(np.complex64)
    bufs = {"cf32": (a, lambda x: eng.process_host(x))}
    for name, (code, dt, bps) in FMTS.items():
        info = np.iinfo(dt)
        p = eng.pinned_array((1, CH, 2), dt)
        p[...] = rng.integers(info.min, info.max + 1, size=(1, CH, 2), dtype=dt)
        bufs[name] = (p, lambda x: eng.process_host(x))
    host_leg("1 stream, synchronous, pinned", eng, bufs, 1, 64)
    eng.close()


if which in ("unpack", "both"):
    unpack()
if which in ("host", "both"):
    host()
