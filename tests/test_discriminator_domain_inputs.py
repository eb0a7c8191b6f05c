"""The streams of tests/discriminator_domain.py reach what they claim to reach -- on the CPU oracle alone, so that tests/test_gpu_discriminator_domain.py
compares the device with the oracle on inputs whose coverage is a checked fact:

  - every one of the 20 ordinary cells (4 quadrants x 5 reduction intervals) holds at least 8 products, in each clean stream and in each planted one;
  - a clean stream holds no product outside the straight-line function's domain behind its first two: product 0 of a stream is x0 * conj(x0), im = 0 exactly
    whatever the input (the reference seeds the discriminator with the first sample itself), and behind two stages the first decimated sample is 0;
  - no 192 consecutive products of a planted stream are all plain (a wave of the device spans 256 or more);
  - decimation = 1 reaches every special class of SPECIALS; the two-stage cases reach REQUIRED_TWO_STAGE;
  - the planted streams, whose bits are compared on the GPU, hold no NaN or Inf in the discriminator output; the wild ones do.

The tap count the GPU cases run with (5 on every route) is pinned here too."""
import numpy as np
import pytest

import discriminator_domain as dd


def test_classifier_on_hand_made_products():
    f = np.array([2 + 0j, 1 + 1j, 0j, 0j, -2 + 0j, 1 + 0j, 0 + 3j, 2.0 ** 100 + 0j, np.nan, 1e-30 + 1e-30j], np.complex64)
    cl = dd.classify(f, f[0])
    assert cl["im+0_re>0"][0] and cl["plain"][1] and cl["cell"][1] == 0 * 5 + 2            # 1: re = 2, im = 2 -> [11/16, 19/16)
    assert cl["both_zero"][2] and cl["both_zero"][3] and cl["both_zero"][4]
    assert cl["im-0_re<0"][5]                                                               # 1 * (-0) + 0 * (-2)
    assert cl["re0_im>0"][6] and cl["re0_im<0"][7] and cl["nan"][8] and cl["nan"][9]
    assert not cl["plain"][[0, 2, 3, 4, 5, 6, 7, 8, 9]].any()
    assert dd.longest_plain_run([1, 1, 0, 1, 1, 1, 0]) == 3
    # the four reduction edges are the bit patterns exact_math.h compares against
    assert [np.float32(e).view(np.uint32) for e in dd.EDGES] == list(dd.INTERVAL_BITS)


@pytest.mark.parametrize("case", list(dd.CASES))
def test_streams_cover_the_discriminator_domain(case):
    c = dd.CASES[case]
    assert all(call["ntaps"] in (0, dd.T) for p in dd.PATTERNS for call in dd.oracle_run(case, p))
    reached = {k: 0 for k in dd.SPECIALS + dd.OPTIONAL}
    for pattern in dd.PATTERNS:
        assert len(dd.stream(case, pattern)) == c["n"] * c["factor"]
        cells, counts, run, nonplain, bad = dd.census(case, pattern)
        print(case, pattern, "cells", cells.tolist(), "longest plain run", run, "non-plain", nonplain, "non-finite outputs", bad,
              {k: v for k, v in counts.items() if v})
        assert cells.min() >= 8, (pattern, cells)
        if pattern.startswith("clean"):
            first = dd.oracle_run(case, pattern)
            seen = 0
            for call in first:
                if len(call["filtered"]):
                    plain = dd.classify(call["filtered"], call["prev"])["plain"]
                    assert plain[2 if not seen else 0:].all(), (pattern, seen, np.nonzero(~plain)[0][:8])
                    seen += len(plain)
            assert seen == c["n"] and nonplain <= 2 and bad == 0
        else:
            assert run < 192, (pattern, run)
            assert (bad == 0) == (pattern == "planted"), (pattern, bad)
            for k in counts:
                reached[k] += counts[k]
    want = dd.SPECIALS if c["factor"] == 1 else dd.REQUIRED_TWO_STAGE
    assert not [k for k in want if not reached[k]], reached
    print(case, "optional classes reached:", {k: reached[k] for k in dd.OPTIONAL})


def test_flip_streams_put_the_nonfinite_stretches_where_they_claim():
    """The NaN / Inf stretches of the discriminator output end R/2 before one bit edge and begin R/2 behind another, the idle one is far from any edge, the oracle
    still decodes around them what it can -- and its flip points differ from the clean stream's in the calls that hold the stretches (the streams do reach the
    flip search)."""
    dd.flip_streams()
    e1, e2, R, span = dd._cache["flip_edges"]
    plain = dd.flip_results("plain")
    assert len(plain[-1]["sentences"]) == 2 and R == 26 and span > 2 * R
    for name in dd.FLIP_STREAMS[1:]:
        res = dd.flip_results(name)
        bad = dd.nonfinite_spans(np.concatenate([c["demod"] for c in res]))
        if name == "nan_idle":
            assert bad[1] < 1000 and e1 > 4000
        else:
            assert abs(bad[0] + span - 1 - (e1 - R // 2)) <= 1 and abs(bad[1] - span + 1 - (e2 + R // 2)) <= 1, (name, bad, e1, e2)
        differ = [k for k in range(len(res)) if not np.array_equal(res[k]["flips"], plain[k]["flips"])]
        print(name, "non-finite outputs", bad, "calls whose flip points differ from the clean stream's", differ)
        assert differ


def test_integer_weight_stream_has_interior_first_maxima():
    """lookup_mode = 0: in at least 10 edge zones the oracle's flip point is not the zone's first position -- the first maximum lies on a plateau of equal
    integer weights, which the device must resolve by index."""
    x, res = dd.integer_weight_stream()
    zones = [z for c in res for z in dd.zones(c, 26)]
    interior = sum(1 for lo, f in zones if f != lo)
    print("zones", len(zones), "with an interior first maximum", interior)
    assert interior >= 10 and len(res[-1]["sentences"]) == 2
    # no NaN and no Inf in this stream: (int)NaN is undefined in the reference
    assert all(np.isfinite(c["demod"]).all() for c in res)
