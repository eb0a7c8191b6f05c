"""What one hd_fsk4_push_engine costs behind a drained batch call: streams x real-time factor of the slot kernel and of the frame kernel.

    python3 tools/micro/fsk4_rate.py [--workload cfg4] [--warmup 5] [--reps 7] [--baud 100] [--preset 1]

First as many calls and pushes as a frame is long, so that the scan has candidates to decide.  Then per repetition: batch calls (pipeline = 2),
hd_flush, then the 4FSK modem's push of the last call's decimated IQ through the library's measurement hook (host time of the whole call; the slot
launches and the frame launches of the push's scan each between two HIP events).  The signal is the benchmark's
RTTY ring, noise to this modem: every slot is a candidate whatever the signal, so the kernels' work is the same -- only the share of candidates behind
the unique-word gate (printed) is noise's.  A call's samples last n / fsd seconds; streams x real-time factor = S * that / the kernel's time.  Prints the
medians and the spreads (min .. max) over the repetitions behind the warm-up."""
from _rate import Rig, fmt, med, parser


def main():
    ap = parser()
    ap.add_argument("--baud", type=float, default=100.0); ap.add_argument("--preset", type=int, default=1)
    ap.add_argument("--f0", type=float, default=-405.0); ap.add_argument("--spacing", type=float, default=270.0)
    a = ap.parse_args()
    rig = Rig(a.workload); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    from habdec_amd.fsk4 import Fsk4
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    baud = min(max(a.baud, fsd / 2048.0), fsd / 8.0)                  # inside the modem's range at this decimated rate
    f = Fsk4(eng)
    for s in range(S):
        f.set_modem(s, baud, a.f0, a.spacing, a.preset)
    # a candidate is decided once its last symbol is in: pushes until the scan has work, so that the timed pushes launch both kernels
    n = Cn // w["D"]
    for _ in range(int(f.stats(0)["symbols"] * fsd / baud / n) + 2):
        rig.feed(1)
        f.push_engine()
    host_us, slots_us, frames_us = [], [], []
    for r in range(a.warmup + a.reps):
        rig.feed(4)
        slots_ms, frames_ms, us = f.debug_push_timed()
        if r >= a.warmup:
            host_us.append(us); slots_us.append(slots_ms * 1e3); frames_us.append(frames_ms * 1e3)
    st = f.stats(0)
    seconds = n / fsd
    print(f"workload {a.workload} S={S}, {n} decimated samples per stream and call at {fsd:.0f} S/s ({seconds * 1e3:.2f} ms of signal), {baud:g} baud, "
          f"preset {a.preset}: median of {a.reps} behind {a.warmup}; stream 0: {st}")
    print("hd_fsk4_push_engine, host time of the call:", fmt(host_us))
    print("k_fsk4_slots alone (HIP events):           ", fmt(slots_us))
    print("k_fsk4_frames alone (HIP events):          ", fmt(frames_us))
    for name, v in (("k_fsk4_slots", slots_us), ("k_fsk4_frames", frames_us), ("the whole call", host_us)):
        if med(v) > 0:
            print(f"streams x real-time factor, {name}: {S * seconds / (med(v) * 1e-6):.0f}")
    total = sum(f.stats(s)["candidates"] for s in range(S)); passes = sum(f.stats(s)["gate_passes"] for s in range(S))
    print(f"candidates decided so far {total}, behind the gate {passes} ({passes / max(total, 1):.2e}), frames {sum(f.stats(s)['frames'] for s in range(S))}")
    eng.close()


if __name__ == "__main__":
    main()
