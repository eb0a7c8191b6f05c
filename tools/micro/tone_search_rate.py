"""What one hd_tone_search_push_engine costs behind a drained batch call, beside one hd_survey_push_device of as many segments, in one process.

    python3 tools/micro/tone_search_rate.py [--workload cfg4] [--warmup 5] [--reps 7]

Per repetition: one batch call (pipeline = 2), hd_flush, then the tone search's push of the call's decimated IQ through the library's measurement hook
(host time of the whole call; the kernel alone between two HIP events).  At cfg4 (1024 streams, 1024 decimated samples per stream and call) every second
push completes one segment per stream -- 1024 transforms, one wave per SIMD -- and the pushes between only append to the carries: the two kinds are
reported separately, each as the median and the spread (min .. max) over the repetitions behind the warm-up.  The yardstick is hd_survey_push_device of
S segments (2048 (S - 1) + 4096 samples, one segment per wave) between HIP events on the survey's queue."""
import ctypes as C
from _rate import Rig, fmt, habdec_amd, med, parser, torch


def main():
    a = parser().parse_args()
    rig = Rig(a.workload); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    ts, sv = eng.tone_search(), eng.survey()
    timed = rig.timed("hd_debug_tone_search_push_timed")
    sv_timed = eng.L.hd_debug_survey_push_timed
    sv_timed.restype, sv_timed.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_float)]
    n_sv = 2048 * (S - 1) + 4096
    wide = torch.randn(2 * n_sv, device=rig.dev, dtype=torch.float32)
    torch.cuda.synchronize()
    host_us, kern_us, survey_us = {"light": [], "transform": []}, {"light": [], "transform": []}, []
    seen = {"light": 0, "transform": 0}
    while min(seen.values()) < a.warmup + a.reps:
        rig.feed()
        before = ts.stats(0)["segments"]
        kern, host = timed(ts.h)
        kind = "transform" if ts.stats(0)["segments"] > before else "light"
        seen[kind] += 1
        if seen[kind] > a.warmup and len(host_us[kind]) < a.reps:
            host_us[kind].append(host); kern_us[kind].append(kern)
    for r in range(a.warmup + a.reps):
        ms = C.c_float(0)
        habdec_amd.capi.check(sv_timed(sv.h, wide.data_ptr(), n_sv, C.byref(ms)))
        if r >= a.warmup:
            survey_us.append(ms.value * 1e3)
    print(f"workload {a.workload} S={S}, {Cn // w['D']} decimated samples per stream and call: median of {a.reps} behind {a.warmup}; stream 0: {ts.stats(0)}")
    print("hd_tone_search_push_engine, a push that completes no segment, host time:  ", fmt(host_us["light"]))
    print("k_tone_search of such a push (HIP events):                                ", fmt(kern_us["light"]))
    print(f"hd_tone_search_push_engine, a push that completes {S} segments, host time:", fmt(host_us["transform"]))
    print("k_tone_search of such a push (HIP events):                                ", fmt(kern_us["transform"]))
    print(f"hd_survey_push_device of {S} segments, k_survey + k_survey_reduce (HIP events):", fmt(survey_us))
    bound = 2 * med(survey_us) + max(survey_us) - min(survey_us)
    print(f"k_tone_search's transform push, median {med(kern_us['transform']):.1f} us, against twice the survey's median + (max - min) = {bound:.1f} us:",
          "HELD" if med(kern_us["transform"]) <= bound else "MISSED")
    p, k = ts.power(0)
    print("stream 0:", k, "segments, mean power", float(p.mean()), "survey segments", sv.power()[1])
    eng.close()


if __name__ == "__main__":
    main()
