#!/usr/bin/env python3
"""Step launches by phase, from a rocprofv3 --kernel-trace csv: in the headline workload every fourth step launch carries the spectra of all streams
(1024 decimated samples per call, 4096 per buffer), so the launches of the step kernel fall into four classes by launch index mod 4.  Prints, per step
kernel (exact and fast apart), the median duration of each class over the launches behind the `skip`-th, the class that carries the spectra (the
slowest) and its excess over the median of the other three.

    step_phase_stats.py <kernel_trace.csv> [skip=150] [kernel=k_step_cu<212,2,69>]
"""
import collections, csv, statistics, sys

sys.path.insert(0, __file__.rsplit("/", 1)[0])
from steady_stats import short


def main():
    src = sys.argv[1]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 150
    want = sys.argv[3] if len(sys.argv) > 3 else "k_step_cu<212,2,69>"
    runs = collections.defaultdict(list)
    for r in csv.DictReader(open(src, newline="")):
        k = short(r["Kernel_Name"])
        if k and k.replace("[fast]", "") == want:
            runs[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for k in sorted(runs):
        v = sorted(runs[k])
        cls = [[(e - s) / 1e3 for i, (s, e) in enumerate(v) if i >= skip and i % 4 == c] for c in range(4)]
        if not all(cls):
            print(k, "fewer than", skip + 4, "launches"); continue
        med = [statistics.median(c) for c in cls]
        heavy = max(range(4), key=lambda c: med[c])
        light = statistics.median(x for c in range(4) if c != heavy for x in cls[c])
        print(f"{k:28s} launches {len(v)} (behind {skip}: {sum(map(len, cls))}); medians by index mod 4 (us): " + " ".join(f"{m:.1f}" for m in med) +
              f"; spectrum-carrying (mod 4 = {heavy}) {med[heavy]:.1f}, light {light:.1f}, excess {med[heavy] - light:.1f}")


if __name__ == "__main__":
    main()
