"""What one hd_clocked_push_engine costs behind a drained batch call, beside one hd_baud_probe_push_engine, in one process.

    python3 tools/micro/clocked_rate.py [--workload cfg4] [--warmup 5] [--reps 7]

Per repetition: batch calls (pipeline = 2), hd_flush, then the clocked decoder's push and the probe's push of the same call's discriminator output
(cfg4: 1024 streams, 1024 decimated samples each), both through the library's measurement hooks (host time of the whole call; the kernel alone between two
HIP events); which of the two goes first alternates.  Prints the medians and the spreads (min .. max) over the repetitions behind the warm-up."""
from _rate import Rig, fmt, med, parser


def main():
    a = parser().parse_args()
    rig = Rig(a.workload); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    probe, clk = eng.baud_probe(), eng.clocked()
    hooks = {}
    for name, obj in (("probe", probe), ("clocked", clk)):
        hooks[name] = (rig.timed("hd_debug_baud_probe_push_timed" if name == "probe" else "hd_debug_clocked_push_timed"), obj)
    host_us, kern_us = {k: [] for k in hooks}, {k: [] for k in hooks}
    for r in range(a.warmup + a.reps):
        rig.feed(4)
        for name in (("probe", "clocked") if r % 2 else ("clocked", "probe")):
            f, obj = hooks[name]
            kern, host = f(obj.h)
            if r >= a.warmup:
                host_us[name].append(host); kern_us[name].append(kern)
    print(f"workload {a.workload} S={S}, {Cn // w['D']} decimated samples per stream and call: median of {a.reps} behind {a.warmup}")
    print("hd_clocked_push_engine, host time of the call:   ", fmt(host_us["clocked"]))
    print("k_clocked alone (HIP events):                    ", fmt(kern_us["clocked"]))
    print("hd_baud_probe_push_engine, host time of the call:", fmt(host_us["probe"]))
    print("k_baud_probe alone (HIP events):                 ", fmt(kern_us["probe"]))
    bound = med(kern_us["probe"]) + max(kern_us["probe"]) - min(kern_us["probe"])
    print(f"k_clocked median {med(kern_us['clocked']):.1f} us against the probe's median + (max - min) = {bound:.1f} us:",
          "within" if med(kern_us["clocked"]) <= bound else "LONGER")
    st = [clk.stats(s) for s in range(S)]
    print("characters", sum(x["characters"] for x in st), "rejects", sum(x["rejects"] for x in st), "dropped", sum(x["dropped"] for x in st),
          "over", st[0]["samples"], "samples per stream; stream 0 sentences:", clk.take_sentences(0)[:2])
    rj = sorted(x["rejects"] for x in st)
    print("rejects per stream: median", rj[S // 2], "max", rj[-1], "streams above 100:", sum(1 for v in rj if v > 100),
          "(a launch lasts as long as its slowest wave: one stream, one wave)")
    eng.close()


if __name__ == "__main__":
    main()
