"""What the *_rate.py tools of this directory share: the arguments, an engine in batch mode fed from the benchmark's ring of one of its workloads, the
library's hd_debug_*_push_timed measurement hooks and the line a list of times is printed as.  Imported from a tool run as a script."""
import argparse, ctypes as C, statistics, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import torch, bench, habdec_amd

med = statistics.median


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4"); ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--reps", type=int, default=7)
    return ap


def fmt(v):
    return f"median {med(v):.1f} us (min {min(v):.1f} .. max {max(v):.1f})"


class Rig:
    """The ring of bench.WORKLOADS[workload] on the GPU and an engine (pipeline = 2) of its shape.  w: the workload; S, Cn: streams, samples per call."""

    def __init__(self, workload):
        self.w = w = dict(bench.WORKLOADS[workload]); self.S, self.Cn = w["S"], w["C"]
        self.dev = torch.device("cuda", 0)
        self.ring, self.rc, _ = bench.generate_ring(torch, self.dev, w, self.S, 0, 1234)
        self.eng = habdec_amd.Engine(n_streams=self.S, max_chunk=self.Cn, sampling_rate=w["fs"], decimation=w["D"], baud=w["baud"], rtty_bits=w["bits"],
                                     rtty_stops=w["stops"], lowpass_bw_hz=w["lp_bw"], lowpass_trans=w["lp_trans"], ungated=w["ungated"], pipeline=2)
        self.i = 0

    def feed(self, calls=1):
        """`calls` batch calls of the ring's next chunks, then hd_flush."""
        for _ in range(calls):
            self.eng.process_device(self.ring.data_ptr() + (self.i % self.rc) * self.S * self.Cn * 8, self.Cn, self.Cn); self.i += 1
        self.eng.flush()

    def timed(self, name, *extra):
        """The hook `name` (its arguments: the object, `extra` ctypes types, then the two outputs) as f(handle, *extra values) -> (kernel us, host us)."""
        f = getattr(self.eng.L, name)
        f.restype, f.argtypes = C.c_int, [C.c_void_p, *extra, C.POINTER(C.c_float), C.POINTER(C.c_double)]

        def call(h, *args):
            ms, us = C.c_float(0), C.c_double(0)
            habdec_amd.capi.check(f(h, *args, C.byref(ms), C.byref(us)))
            return ms.value * 1e3, us.value
        return call
