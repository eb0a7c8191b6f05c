"""What one hd_tones_push_engine costs behind a drained batch call, beside one hd_baud_probe_push_engine, in one process.

    python3 tools/micro/tones_rate.py [--workload cfg4] [--warmup 5] [--reps 7]

Per repetition: batch calls (pipeline = 2), hd_flush, then the tone-filter demodulator's push of the call's decimated IQ and the probe's push of the same
call's discriminator output (cfg4: 1024 streams, 1024 decimated samples each), both through the library's measurement hooks (host time of the whole call;
the kernel alone between two HIP events); which of the two goes first alternates.  Prints the medians and the spreads (min .. max) over the repetitions
behind the warm-up."""
from _rate import Rig, fmt, med, parser


def main():
    ap = parser()
    ap.add_argument("--shift", type=float, default=500.0, help="the tones are set shift / 2 above and below the centre")
    a = ap.parse_args()
    rig = Rig(a.workload); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    probe, tones = eng.baud_probe(), eng.tones()
    for s in range(S):
        tones.set_modem(s, 0, a.shift / 2, -a.shift / 2)
    hooks = {}
    for name, obj in (("probe", probe), ("tones", tones)):
        hooks[name] = (rig.timed("hd_debug_baud_probe_push_timed" if name == "probe" else "hd_debug_tones_push_timed"), obj)
    host_us, kern_us = {k: [] for k in hooks}, {k: [] for k in hooks}
    for r in range(a.warmup + a.reps):
        rig.feed(4)
        for name in (("probe", "tones") if r % 2 else ("tones", "probe")):
            f, obj = hooks[name]
            kern, host = f(obj.h)
            if r >= a.warmup:
                host_us[name].append(host); kern_us[name].append(kern)
    st = tones.stats(0)
    print(f"workload {a.workload} S={S}, {Cn // w['D']} decimated samples per stream and call: median of {a.reps} behind {a.warmup}; modem of stream 0: {st}")
    print("hd_tones_push_engine, host time of the call:     ", fmt(host_us["tones"]))
    print("k_tones alone (HIP events):                      ", fmt(kern_us["tones"]))
    print("hd_baud_probe_push_engine, host time of the call:", fmt(host_us["probe"]))
    print("k_baud_probe alone (HIP events):                 ", fmt(kern_us["probe"]))
    bound = med(kern_us["probe"]) + max(kern_us["probe"]) - min(kern_us["probe"])
    print(f"k_tones median {med(kern_us['tones']):.1f} us against the probe's median + (max - min) = {bound:.1f} us:",
          "within" if med(kern_us["tones"]) <= bound else "LONGER")
    row = tones.output(0)
    print("stream 0: row of", row.size, "samples, mean |o|", float(abs(row).mean()) if row.size else 0.0, "samples per stream so far", st["samples"])
    eng.close()


if __name__ == "__main__":
    main()
