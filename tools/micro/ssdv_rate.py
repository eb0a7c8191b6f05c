"""What one hd_ssdv_push_clocked costs behind a clocked push, in the worst case: every candidate fails all four trials.

    python3 tools/micro/ssdv_rate.py [--workload cfg4] [--warmup 5] [--reps 7]

cfg4's engine (1024 streams); every clocked stream gets a 300 baud 8N2 modem, so the engine's rows are noise to it and the characters it frames are
random bytes.  Per repetition: one batch call, hd_flush, hd_clocked_push_engine, then hd_ssdv_push_clocked (--calls N: once behind N such pushes), both through the library's measurement hooks
(host time of the whole call; the kernel alone between two HIP events).  Prints the medians and the spreads (min .. max) over the repetitions behind the
warm-up, the yardstick (k_clocked's median plus its max - min: HELD or MISSED, not a gate).  cfg4's rows turn out to give that modem too few characters
for any stream to reach a packet's length, so the tool then times hd_ssdv_scan under a stated load of random bytes (--per-stream per stream and scan),
where every candidate fails all four trials, and the restatement on one core for the same number of candidates."""
import ctypes as C, time
import numpy as np
from _rate import Rig, fmt, med, parser
from habdec_amd.ssdv import HostSsdv, Ssdv


def main():
    ap = parser()
    ap.add_argument("--calls", type=int, default=1, help="batch calls and clocked pushes per hd_ssdv_push_clocked (1: after each clocked push)")
    ap.add_argument("--lead", type=int, default=100, help="unmeasured calls in front, until every stream holds a packet's length of bytes")
    ap.add_argument("--per-stream", type=int, default=4, help="bytes per stream and scan of the stated load")
    a = ap.parse_args()
    rig = Rig(a.workload); eng, w, S, Cn = rig.eng, rig.w, rig.S, rig.Cn
    clk, v = eng.clocked(), Ssdv(eng)
    for s in range(S):
        clk.set_modem(s, 300.0, 8, 2)
    f_clk, f_v = rig.timed("hd_debug_clocked_push_timed"), rig.timed("hd_debug_ssdv_scan_timed", C.c_void_p)
    host_us, kern_us = {"clocked": [], "ssdv": []}, {"clocked": [], "ssdv": []}
    new_bytes = []
    for _ in range(a.lead):                                          # a stream decides nothing before it holds 256 bytes: about 75 calls' characters
        rig.feed()
        clk.push_engine()
    v.push_clocked(clk)
    for r in range(a.warmup + a.reps):
        kc = hc = 0.0
        for _ in range(a.calls):                                     # (one clocked push per batch call: a push takes the call delivered last)
            rig.feed()
            kc, hc = f_clk(clk.h)
        before = sum(v.stats(s)["bytes"] for s in range(S))
        kv, hv = f_v(v.h, clk.h)
        if r >= a.warmup:
            host_us["clocked"].append(hc); kern_us["clocked"].append(kc)
            host_us["ssdv"].append(hv); kern_us["ssdv"].append(kv)
            new_bytes.append(sum(v.stats(s)["bytes"] for s in range(S)) - before)
    print(f"workload {a.workload} S={S}, {a.calls} calls of {Cn // w['D']} decimated samples per repetition: median of {a.reps} behind {a.warmup}")
    print("hd_ssdv_push_clocked, host time of the call:  ", fmt(host_us["ssdv"]))
    print("k_ssdv_scan alone (HIP events):                ", fmt(kern_us["ssdv"]))
    print("hd_clocked_push_engine, host time of the call:", fmt(host_us["clocked"]))
    print("k_clocked alone (HIP events):                  ", fmt(kern_us["clocked"]))
    bound = med(kern_us["clocked"]) + max(kern_us["clocked"]) - min(kern_us["clocked"])
    print(f"yardstick: k_ssdv_scan median {med(kern_us['ssdv']):.1f} us against k_clocked's median + (max - min) = {bound:.1f} us:",
          "HELD" if med(kern_us["ssdv"]) <= bound else "MISSED")
    st = [v.stats(s) for s in range(S)]
    print("new bytes per repetition over all streams: median", med(new_bytes), "; decided", sum(x["decided"] for x in st), "crc_bad", sum(x["crc_bad"] for x in st),
          "packets", sum(sum(x["packets"]) for x in st))
    # The engine's rows give that modem few characters (a clean 50 baud signal has few edges a 300 baud clock frames): where no stream reaches a
    # packet's length, k_ssdv_scan is never launched above.  The kernel under a stated load instead: every stream holds 255 random bytes, then
    # per repetition --per-stream more (4: what a 300 baud stream brings in 128 ms) go in through hd_ssdv_push_bytes and hd_ssdv_scan is timed.
    w2 = Ssdv(eng)
    rng = np.random.default_rng(2)
    for s in range(S):
        w2.push_bytes(s, rng.integers(0, 256, 255, dtype=np.uint8), rng.integers(0, 1 << 24, 255, dtype=np.uint32))
    w2.scan()
    syn_host, syn_kern = [], []
    for r in range(a.warmup + a.reps):
        for s in range(S):
            w2.push_bytes(s, rng.integers(0, 256, a.per_stream, dtype=np.uint8), rng.integers(0, 1 << 24, a.per_stream, dtype=np.uint32))
        kv, hv = f_v(w2.h, None)
        if r >= a.warmup:
            syn_host.append(hv); syn_kern.append(kv)
    st2 = [w2.stats(s) for s in range(S)]
    print(f"stated load, {S * a.per_stream} candidates of random bytes per scan ({a.per_stream} per stream): hd_ssdv_scan host time", fmt(syn_host))
    print("k_ssdv_scan alone under that load (HIP events):", fmt(syn_kern), "; crc_bad", sum(x["crc_bad"] for x in st2), "of", sum(x["decided"] for x in st2), "decided")
    print(f"yardstick under the stated load: median {med(syn_kern):.1f} us against {bound:.1f} us:", "HELD" if med(syn_kern) <= bound else "MISSED")
    # the restatement on one core: as many random bytes as one scan of the stated load decides, in one stream
    n = S * a.per_stream
    rng = np.random.default_rng(1)
    h = HostSsdv()
    h.push_bytes(rng.integers(0, 256, 255, dtype=np.uint8))
    t0 = time.perf_counter()
    h.push_bytes(rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 1 << 24, n, dtype=np.uint32))
    print(f"host restatement, one core, {n} candidates of random bytes: {(time.perf_counter() - t0) * 1e6:.0f} us")
    eng.close()


if __name__ == "__main__":
    main()
