"""What one hd_fsk4_track_push_engine costs behind a drained batch call: the whole push and, inside it, the comb detector.

    python3 tools/micro/fsk4_track_rate.py [--workload cfg4] [--warmup 5] [--reps 7] [--baud 100] [--epoch-segments 4]

Per repetition: batch calls (pipeline = 2) until every stream's epoch is one call short of its end, hd_flush, then the tracker's push of the last
call's decimated IQ through the library's measurement hook -- the push between two HIP events (its spectrum launches, its comb launch and the waits
between them), the comb launch alone between two more, and the host time of the whole call.  Every stream's epoch ends in the timed push, so the comb
launch serves all S streams.  The signal is the benchmark's RTTY ring, no comb to this detector: the search is exhaustive, so its work is the same
whatever the signal.  Prints the medians and the spreads (min .. max) over the repetitions behind the warm-up."""
from _rate import Rig, fmt, med, parser


def main():
    ap = parser()
    ap.add_argument("--baud", type=float, default=100.0); ap.add_argument("--epoch-segments", type=int, default=4)
    a = ap.parse_args()
    rig = Rig(a.workload); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    from habdec_amd.fsk4_track import Fsk4Track
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    baud = min(max(a.baud, fsd / 2048.0), fsd / 8.0)
    tr = Fsk4Track(eng, epoch_segments=a.epoch_segments)
    for s in range(S):
        tr.set_stream(s, baud, 2.0 * baud, 4.0 * baud, -0.375 * fsd, 0.375 * fsd)
    n = Cn // w["D"]
    E = a.epoch_segments

    def to_go():                                                      # samples to the end of stream 0's epoch
        st = tr.stats(0)
        return 2048 * ((st["epochs"] + 1) * E + 1) - st["samples"]

    push_us, comb_us, host_us, epochs = [], [], [], []
    for r in range(a.warmup + a.reps):
        while to_go() > n:                                            # untimed pushes up to the call in which the epoch ends
            rig.feed(1)
            tr.push_engine()
        before = tr.stats(0)["epochs"]
        rig.feed(1)
        push_ms, comb_ms, us = tr.debug_push_timed()
        if r >= a.warmup:
            push_us.append(push_ms * 1e3); comb_us.append(comb_ms * 1e3); host_us.append(us); epochs.append(tr.stats(0)["epochs"] - before)
    print(f"workload {a.workload} S={S}, {n} decimated samples per stream and call at {fsd:.0f} S/s, {baud:g} baud, epochs of {E} segments: "
          f"median of {a.reps} behind {a.warmup}; epochs ended per timed push {sorted(set(epochs))}; stream 0: {tr.stats(0)}, {tr.estimate(0)}")
    print("hd_fsk4_track_push_engine, host time of the call:", fmt(host_us))
    print("the whole push (HIP events):                      ", fmt(push_us))
    print("k_fsk4_comb alone (HIP events):                   ", fmt(comb_us))
    eng.close()


if __name__ == "__main__":
    main()
