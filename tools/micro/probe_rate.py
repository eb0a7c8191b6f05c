"""What one hd_baud_probe_push_engine costs behind a drained batch call, beside the first hd_stream_spectrum behind a batch, in one process.

    python3 tools/micro/probe_rate.py [--workload cfg4] [--warmup 5] [--reps 7]

Per repetition: one batch call (pipeline = 2), hd_flush, then the probe's push through the library's measurement hook (host time of the whole call;
the kernel alone between two HIP events), then one more call, hd_flush and hd_stream_spectrum(0) (the getter that launches the lazy spectra).
Prints the medians and the spreads (min .. max) over the repetitions behind the warm-up."""
import argparse, ctypes as C, statistics, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import torch, bench, habdec_amd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4"); ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    w = dict(bench.WORKLOADS[a.workload]); S, Cn = w["S"], w["C"]
    dev = torch.device("cuda", 0)
    ring, rc, _ = bench.generate_ring(torch, dev, w, S, 0, 1234)
    base = ring.data_ptr()
    eng = habdec_amd.Engine(n_streams=S, max_chunk=Cn, sampling_rate=w["fs"], decimation=w["D"], baud=w["baud"], rtty_bits=w["bits"], rtty_stops=w["stops"],
                            lowpass_bw_hz=w["lp_bw"], lowpass_trans=w["lp_trans"], ungated=w["ungated"], pipeline=2)
    probe = eng.baud_probe()
    hook = eng.L.hd_debug_baud_probe_push_timed
    hook.restype, hook.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double)]
    host_us, kern_us, spec_us, step_us = [], [], [], []
    i = 0
    buf = np.zeros(8192, np.float32)
    for r in range(a.warmup + a.reps):
        for _ in range(4):                                  # (the spectrum completes every fourth call of this workload)
            eng.process_device(base + (i % rc) * S * Cn * 8, Cn, Cn); i += 1
        eng.flush()
        ms, us = C.c_float(0), C.c_double(0)
        habdec_amd.capi.check(hook(probe.h, C.byref(ms), C.byref(us)))
        for _ in range(4):
            eng.process_device(base + (i % rc) * S * Cn * 8, Cn, Cn); i += 1
        eng.flush()
        t0 = time.perf_counter()
        n = eng.L.hd_stream_spectrum(eng.h, 0, buf, 4096)
        t1 = time.perf_counter()
        assert n == 4096, n
        if r >= a.warmup:
            host_us.append(us.value); kern_us.append(ms.value * 1e3); spec_us.append((t1 - t0) * 1e6); step_us.append(eng.timing()["ms_front"] * 1e3)
    med = statistics.median
    fmt = lambda v: f"median {med(v):.1f} us (min {min(v):.1f} .. max {max(v):.1f})"
    print(f"workload {a.workload} S={S}: median of {a.reps} behind {a.warmup}")
    print("hd_baud_probe_push_engine, host time of the call:", fmt(host_us))
    print("k_baud_probe alone (HIP events):                 ", fmt(kern_us))
    print("first hd_stream_spectrum behind a batch:         ", fmt(spec_us))
    print("one step launch of the same engine (ms_front):   ", fmt(step_us))
    print("stream 0 after", probe.state(0)["samples"], "samples:", probe.estimate(0))
    eng.close()


if __name__ == "__main__":
    main()
