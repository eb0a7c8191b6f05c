"""What one hd_combine_push_device of the tones' rows costs behind hd_tones_push_engine, in one process, and one lag search per group.

    python3 tools/micro/combine_rate.py [--workload cfg4] [--warmup 5] [--reps 7] [--members 4]

Per repetition: batch calls (pipeline = 2), hd_flush, the tone-filter demodulator's push of the call's decimated IQ, then the combiner's push of the tones'
rows (cfg4: 1024 streams in 256 groups of 4, 1024 samples each), both through the library's measurement hooks (host time of the whole call; the kernel
alone between two HIP events).  Prints the medians and the spreads (min .. max) over the repetitions behind the warm-up, k_combine against the yardstick
-- k_tones' median plus its max - min for the same calls -- and the wall time of hd_combine_lags over every group at the default window and lag range."""
import ctypes as C, time
import numpy as np
from _rate import Rig, fmt, med, parser
from habdec_amd import capi
from habdec_amd.combine import Combiner, _lag_params


def main():
    ap = parser()
    ap.add_argument("--members", type=int, default=4); ap.add_argument("--shift", type=float, default=500.0)
    a = ap.parse_args()
    rig = Rig(a.workload); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    tones, comb = eng.tones(), Combiner(eng)
    for s in range(S):
        tones.set_modem(s, 0, a.shift / 2, -a.shift / 2)
    groups = [list(range(g, min(g + a.members, S))) for g in range(0, S, a.members)]
    for g in groups:
        comb.set_group(g)
    t_tones = rig.timed("hd_debug_tones_push_timed")
    t_comb = rig.timed("hd_debug_combine_push_timed", C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32)
    host_us, kern_us = {"tones": [], "combine": []}, {"tones": [], "combine": []}

    def one(keep):
        rig.feed(4)
        kern, host = t_tones(tones.h)
        if keep:
            host_us["tones"].append(host); kern_us["tones"].append(kern)
        ptr, stride, n = tones.rows()
        kern, host = t_comb(comb.h, ptr, stride, n.ctypes.data, 0)
        if keep:
            host_us["combine"].append(host); kern_us["combine"].append(kern)

    for r in range(a.warmup + a.reps):
        one(r >= a.warmup)
    print(f"workload {a.workload} S={S} in {len(groups)} groups of {a.members}, {Cn // w['D']} decimated samples per stream and call: median of {a.reps} behind {a.warmup}")
    print("hd_tones_push_engine, host time of the call:                   ", fmt(host_us["tones"]))
    print("k_tones alone (HIP events):                                    ", fmt(kern_us["tones"]))
    print("hd_combine_push_device of the tones' rows, host time of the call:", fmt(host_us["combine"]))
    print("k_combine alone (HIP events):                                  ", fmt(kern_us["combine"]))
    bound = med(kern_us["tones"]) + max(kern_us["tones"]) - min(kern_us["tones"])
    print(f"k_combine median {med(kern_us['combine']):.1f} us against k_tones' median + (max - min) = {bound:.1f} us:",
          "HELD" if med(kern_us["combine"]) <= bound else "MISSED")
    p = _lag_params(eng.L, max(1, round(eng.L.hd_engine_decimated_rate(eng.h) / w["baud"])), {})
    while comb.stats(0)["samples"] < p.window + 2 * p.max_lag:
        one(False)
    out = np.zeros(capi.COMBINE_MAX_MEMBERS, capi.COMBINE_LAG_DTYPE)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for g in groups:
            capi.check(eng.L.hd_combine_lags(comb.h, g[0], C.byref(p), out.ctypes.data, out.size))
        times.append((time.perf_counter() - t0) * 1e3)
    print(f"hd_combine_lags over {len(groups)} groups (window {p.window}, max_lag {p.max_lag}, guard {p.guard}), wall time of the {len(groups)} calls: "
          f"{min(times):.2f} ms best of 3 ({min(times) / len(groups) * 1e3:.1f} us per group); samples per stream {comb.stats(0)['samples']}")
    row = comb.output(0)
    print("group 0: row of", row.size, "samples, mean |o|", float(abs(row).mean()) if row.size else 0.0, "last search:", out[:a.members].tolist())
    eng.close()


if __name__ == "__main__":
    main()
