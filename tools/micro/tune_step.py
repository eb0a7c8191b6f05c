"""The headline batch (bench.py cfg4: 1024 streams at /64, pipeline = 2) untuned and with every stream tuned (hd_stream_set_tune, offsets of 1..64 Hz:
every sample is rotated, and the payloads stay inside the low-pass, so that both batches decode the same text and run the same symbol work -- offsets
that move the payloads out of the low-pass leave the discriminator with noise, whose flips cost the tails more search work than the rotation costs):
the launch path, the step kernel's launch time from the engine's own HIP events (ms_front of the timed calls) and the wall time per step.
Usage: tune_step.py [steps=400] [untuned|tuned|both]   -- under `rocprofv3 --kernel-trace --stats -- python tools/micro/tune_step.py 400 tuned`, one
batch per process, the k_step_cu row of the stats is the number the two batches are compared by."""
import pathlib, sys, time
import numpy as np
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
import torch
import habdec_amd
import bench

n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
which = sys.argv[2] if len(sys.argv) > 2 else "both"
w = dict(bench.WORKLOADS["cfg4"]); S, fs, C = w["S"], w["fs"], w["C"]
ring, rc, _ = bench.generate_ring(torch, torch.device("cuda", 0), w, S, 0, seed=1234)
torch.cuda.synchronize()


def run(tuned: bool):
    eng = habdec_amd.Engine(n_streams=S, max_chunk=C, sampling_rate=fs, decimation=w["D"], baud=w["baud"], rtty_bits=w["bits"], rtty_stops=w["stops"],
                            lowpass_bw_hz=w["lp_bw"], lowpass_trans=w["lp_trans"], pipeline=2)
    if tuned:
        for s in range(S):
            eng.set_tune(s, 1.0 + (s % 64))
    eng.set_timing(4)
    us, seen, paths = [], 0, set()
    for k in range(n):
        if k == n // 4:
            torch.cuda.synchronize(); t0 = time.perf_counter()
        eng.process_device(ring[k % rc].data_ptr(), C, C)
        t = eng.timing()
        paths.add(t["path"])
        if t["timed_calls"] != seen:
            seen = t["timed_calls"]
            if k >= n // 4:
                us.append(t["ms_front"] * 1e3)
    eng.flush()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / (n - n // 4) * 1e6
    t = eng.timing()
    print(f"{'tuned' if tuned else 'untuned':8s} path {sorted(paths)} step_variant {t['step_variant']}  step launch median {np.median(us):.1f} us "
          f"(p10 {np.percentile(us, 10):.1f}, p90 {np.percentile(us, 90):.1f}, {len(us)} timed)  wall {wall:.1f} us/step  sentences {eng.sentences_ok()}",
          flush=True)
    eng.close()


for tuned in ([False, True] if which == "both" else [which == "tuned"]):
    run(tuned)
