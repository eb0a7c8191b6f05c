"""What one hd_baud_probe_push_engine costs behind a drained batch call, beside the first hd_stream_spectrum behind a batch, in one process.

    python3 tools/micro/probe_rate.py [--workload cfg4] [--warmup 5] [--reps 7]

Per repetition: one batch call (pipeline = 2), hd_flush, then the probe's push through the library's measurement hook (host time of the whole call;
the kernel alone between two HIP events), then one more call, hd_flush and hd_stream_spectrum(0) (the getter that launches the lazy spectra).
Prints the medians and the spreads (min .. max) over the repetitions behind the warm-up."""
import time
import numpy as np
from _rate import Rig, fmt, parser


def main():
    a = parser().parse_args()
    rig = Rig(a.workload); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    probe = eng.baud_probe()
    hook = rig.timed("hd_debug_baud_probe_push_timed")
    host_us, kern_us, spec_us, step_us = [], [], [], []
    buf = np.zeros(8192, np.float32)
    for r in range(a.warmup + a.reps):
        rig.feed(4)                                         # (the spectrum completes every fourth call of this workload)
        kern, host = hook(probe.h)
        rig.feed(4)
        t0 = time.perf_counter()
        n = eng.L.hd_stream_spectrum(eng.h, 0, buf, 4096)
        t1 = time.perf_counter()
        assert n == 4096, n
        if r >= a.warmup:
            host_us.append(host); kern_us.append(kern); spec_us.append((t1 - t0) * 1e6); step_us.append(eng.timing()["ms_front"] * 1e3)
    print(f"workload {a.workload} S={S}: median of {a.reps} behind {a.warmup}")
    print("hd_baud_probe_push_engine, host time of the call:", fmt(host_us))
    print("k_baud_probe alone (HIP events):                 ", fmt(kern_us))
    print("first hd_stream_spectrum behind a batch:         ", fmt(spec_us))
    print("one step launch of the same engine (ms_front):   ", fmt(step_us))
    print("stream 0 after", probe.state(0)["samples"], "samples:", probe.estimate(0))
    eng.close()


if __name__ == "__main__":
    main()
