"""Rate of the wideband survey (hd_survey_push_device, kernels/survey.hip), and the existing spectrum launch beside it.

survey:   one device-resident push of 2^27 samples (1 GiB): HIP events on the survey's queue around the push's launches (k_survey + k_survey_reduce), the
          median of `timed` pushes behind `warm` untimed ones issued back to back (an idle GPU drops its clocks within 20 ms, NOTES.md).  Prints samples/s,
          segments/s and the share of the 8 TB/s HBM peak at 8 algorithmic bytes per sample (every sample is read twice, hop = half a segment: the second
          read is the caches' business).
spectrum: 1024 streams at /64 with the DC blocker on (the separate-kernels path): every fourth 65536-sample call runs k_spectrum_wave over 1024 streams.
          Under `rocprofv3 --kernel-trace --stats -- python tools/micro/survey_rate.py spectrum` the k_spectrum_wave row / 1024 is the existing
          path's time per transform; `both` puts k_survey into the same table.
Usage: survey_rate.py [survey|spectrum|both] [log2_samples=27] [warm=5] [timed=7]"""
import ctypes as C
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import torch
import habdec_amd

which = sys.argv[1] if len(sys.argv) > 1 else "survey"
lg = int(sys.argv[2]) if len(sys.argv) > 2 else 27
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
timed = int(sys.argv[4]) if len(sys.argv) > 4 else 7
FS = 2.048e6


def survey():
    n = 1 << lg
    x = torch.empty(2 * n, dtype=torch.float32, device="cuda").normal_(0.0, 0.05)
    torch.cuda.synchronize()
    eng = habdec_amd.Engine(n_streams=1, sampling_rate=FS, decimation=64)
    sv = eng.survey()
    fn = eng.L.hd_debug_survey_push_timed
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float)]
    ms = C.c_float(0)
    out = []
    for k in range(warm + timed):
        habdec_amd.capi.check(fn(sv.h, x.data_ptr(), n, C.byref(ms)))
        out.append(float(ms.value))
    p, segs = sv.power()
    t = np.array(out[warm:])
    med = float(np.median(t))
    seg_per_push = segs // (warm + timed)
    print(f"survey: 2^{lg} samples per push, {seg_per_push} segments; pushes (ms): " + " ".join(f"{v:.3f}" for v in out))
    print(f"survey: median of {timed} behind {warm}: {med:.3f} ms (min {t.min():.3f}, max {t.max():.3f}) -> {n / med / 1e6:.2f} GS/s, "
          f"{seg_per_push / med / 1e3:.2f} M segments/s, {med * 1e6 / seg_per_push:.1f} ns per segment, {8 * n / med / 1e9:.3f} TB/s = {8 * n / med / 1e9 / 8 * 100:.1f} % of 8 TB/s; "
          f"median bin power {np.median(p):.6f} (2 sigma^2 = 0.005)", flush=True)
    sv.close(); eng.close()


def spectrum(calls=64):
    S, CH = 1024, 65536
    x = torch.empty(S * 2 * CH, dtype=torch.float32, device="cuda").normal_(0.0, 0.05)
    torch.cuda.synchronize()
    eng = habdec_amd.Engine(n_streams=S, sampling_rate=FS, decimation=64, dc_remove=True)
    for k in range(calls):
        eng.process_device(x.data_ptr(), CH, CH)
    print(f"spectrum: {calls} calls of {S} streams on path {eng.timing()['path']}, {eng.afc(0)['spectra']} spectra per stream "
          f"(k_spectrum_wave launches of {S} transforms each: see the kernel trace)", flush=True)
    eng.close()


if which in ("survey", "both"):
    survey()
if which in ("spectrum", "both"):
    spectrum()
