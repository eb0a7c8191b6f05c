"""What one hd_afsk_push_engine costs behind a drained batch call, and one hd_fsk4_push_engine beside it on the same engine: 1024 streams x 4096 samples.

    python3 tools/micro/afsk_rate.py [--warmup 5] [--reps 7] [--decimation 16]

The benchmark's cfg4 ring through an engine at /16 instead of /64: a call of 65536 samples leaves 4096 decimated samples per stream at 128 kS/s, a whole
chunk of either slot kernel.  First as many calls and pushes as the longest walk (afsk) and a frame (fsk4) last, so that both scans have work.  Then per
repetition: batch calls, hd_flush, the AFSK modem's push of the last call's discriminator rows and the 4FSK modem's push of its decimated IQ, each
through the library's measurement hook (host time of the whole call; the slot launches, and the launches of the push's scan, each between two HIP
events).  The signal is the benchmark's RTTY ring, noise to both modems.  Prints the medians and the spreads over the repetitions behind the warm-up."""
from _rate import Rig, bench, fmt, med, parser


def main():
    ap = parser()
    ap.add_argument("--decimation", type=int, default=16)
    a = ap.parse_args()
    name = f"{a.workload}_d{a.decimation}"
    bench.WORKLOADS[name] = dict(bench.WORKLOADS[a.workload], D=a.decimation)
    rig = Rig(name); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    from habdec_amd.afsk import Afsk
    from habdec_amd.fsk4 import Fsk4
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    n = Cn // w["D"]
    af, f4 = Afsk(eng), Fsk4(eng)
    for s in range(S):
        eng.set_lowpass_bw(s, 11000.0)
        af.set_bell202(s)
        f4.set_modem(s, 100.0, -405.0, 270.0, 1)
    spb = fsd / 1200.0
    for _ in range(int(max(3196 * spb, f4.stats(0)["symbols"] * fsd / 100.0) / n) + 3):
        rig.feed(1)
        af.push_engine(); f4.push_engine()
    t = {k: [] for k in ("afsk host", "k_afsk_slots", "afsk scan (k_afsk_gate, k_afsk_frames)", "fsk4 host", "k_fsk4_slots", "k_fsk4_frames")}
    for r in range(a.warmup + a.reps):
        rig.feed(4)
        a_slots, a_scan, a_us = af.debug_push_timed()
        f_slots, f_frames, f_us = f4.debug_push_timed()
        if r >= a.warmup:
            for k, v in zip(t, (a_us, a_slots * 1e3, a_scan * 1e3, f_us, f_slots * 1e3, f_frames * 1e3)):
                t[k].append(v)
    print(f"S={S}, {n} decimated samples per stream and call at {fsd:.0f} S/s ({n / fsd * 1e3:.2f} ms of signal): median of {a.reps} behind {a.warmup}")
    print("afsk stream 0:", af.stats(0))
    print("fsk4 stream 0:", f4.stats(0))
    for k, v in t.items():
        print(f"{k}: {fmt(v)}")
    flags = sum(af.stats(s)["flags"] for s in range(S)); slots = sum(af.stats(s)["slots"] for s in range(S))
    print(f"afsk: slots {slots}, flags {flags} ({flags / max(slots, 1):.2e}), frames {sum(af.stats(s)['frames_plain'] + af.stats(s)['frames_repaired'] for s in range(S))}")
    for s in (0, S - 1):
        assert af.debug_guards(s) == 0
    eng.close()


if __name__ == "__main__":
    main()
