"""Rate of the waterfall (hd_waterfall_push_device: k_survey with run_len = L into the ring, k_waterfall_detect, k_waterfall_hits, the read-back of
528 bytes per row), beside the survey's push of the same samples.

A push returns when its rows' headers and marks are in host memory, so the clock is the host's: the median of `timed` pushes behind `warm` untimed
ones issued back to back (an idle GPU drops its clocks within 20 ms, NOTES.md).  One device-resident push of 2^lg samples; prints samples/s, rows/s,
microseconds per row and the bytes that crossed the link.  Under `rocprofv3 --kernel-trace --stats -- python tools/micro/waterfall_rate.py` the
k_waterfall_detect row / rows is the detector's time per row beside k_survey's.
Usage: waterfall_rate.py [log2_samples=25] [slot_segments=16] [warm=5] [timed=7]"""
import pathlib
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import torch
import habdec_amd

lg = int(sys.argv[1]) if len(sys.argv) > 1 else 25
L = int(sys.argv[2]) if len(sys.argv) > 2 else 16
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
timed = int(sys.argv[4]) if len(sys.argv) > 4 else 7
FS = 2.048e6

n = 1 << lg
x = torch.empty(2 * n, dtype=torch.float32, device="cuda").normal_(0.0, 0.05)
torch.cuda.synchronize()
eng = habdec_amd.Engine(n_streams=1, sampling_rate=FS, decimation=64)


def run(push, label, rows_of):
    out = []
    for k in range(warm + timed):
        t0 = time.perf_counter()
        push()
        out.append((time.perf_counter() - t0) * 1e3)
    t = np.array(out[warm:])
    med = float(np.median(t))
    rows = rows_of()
    print(f"{label}: 2^{lg} samples per push; pushes (ms): " + " ".join(f"{v:.3f}" for v in out))
    print(f"{label}: median of {timed} behind {warm}: {med:.3f} ms (min {t.min():.3f}, max {t.max():.3f}) -> {n / med / 1e6:.2f} GS/s"
          + (f", {rows} rows per push, {rows / med / 1e3:.2f} M rows/s, {med * 1e3 / rows:.2f} us per row, {528 * rows} bytes read back" if rows else ""), flush=True)


wf = eng.waterfall(slot_segments=L)
run(lambda: wf.push_device(x.data_ptr(), n), f"waterfall L={L}", lambda: wf.rows_total() // (warm + timed))
h = wf.headers()
hits, counted = wf.hits()
print(f"waterfall: {wf.rows_total()} rows, {counted} unflagged, {int(h['n_marked'].sum())} marks, {len(wf.tracks())} tracks (noise alone: 0 and 0); "
      f"median floor / (segments * sum w^2) = {np.median(wf.rows(wf.rows_total() - 1, 1, normalised=True)):.6f} (2 sigma^2 = 0.005)", flush=True)
wf.close()
sv = eng.survey()


def survey_push():
    sv.push_device(x.data_ptr(), n)
    sv.power()                                   # (the survey's push only queues: its read-back is the wait)


run(survey_push, "survey + power read-back", lambda: 0)
sv.close()
eng.close()
