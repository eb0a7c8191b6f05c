"""CRC-guided repair (hd_host_chase_repair, host/chase_repair.hpp) on hand-made records: the rule of include/habdec_amd.h, case by case.  No GPU."""
import numpy as np
import pytest

from habdec_amd import synth


@pytest.fixture(scope="module")
def hd():
    from habdec_amd.build import build
    build()
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


def span_of(call, data):
    return synth.make_sentence(call, data).rstrip("\n")              # $$call,data*CRC


def soft(span, weak=(), strong=1000):
    """data[n][8]: +-strong by the character's bits; weak: [((character, bit), magnitude)]."""
    d = np.zeros((len(span), 8), np.int32)
    for c, ch in enumerate(span):
        for k in range(8):
            d[c, k] = strong if (ord(ch) >> k) & 1 else -strong
    for (c, k), mag in weak:
        d[c, k] = mag if d[c, k] > 0 else -mag
    return d


def flip(span, bits):
    s = list(span)
    for c, k in bits:
        s[c] = chr(ord(s[c]) ^ (1 << k))
    return "".join(s)


SPAN = span_of("CHASE", "17,12:00:01,52.1234,-0.5678,321")
# eight weak bits in the data field (characters 10 ..), low bits of digits and letters: every flip leaves a printable character
WEAK8 = [(10, 0), (12, 1), (13, 0), (15, 2), (16, 0), (19, 1), (21, 0), (22, 2)]


def test_the_span_is_a_sentence(hd):
    assert SPAN.startswith("$$CHASE,17,") and SPAN[-5] == "*"
    assert all(32 <= ord(c) <= 126 for b in WEAK8 for c in flip(SPAN, [b]))


@pytest.mark.parametrize("wrong", [[0], [7], [0, 1], [2, 7], [0, 1, 2], [3, 5, 7], [5, 6, 7]])
def test_up_to_three_wrong_bits_among_the_eight_least_confident_are_repaired(hd, wrong):
    weak = [(b, 10 + i) for i, b in enumerate(WEAK8)]
    bad = flip(SPAN, [WEAK8[i] for i in wrong])
    got = hd.chase_repair(bad, soft(bad, weak))
    assert got == (SPAN, len(wrong)), (wrong, got)
    # the same with seven data bits per character (bit 7 is not looked at)
    assert hd.chase_repair(bad, soft(bad, weak), nbits=7) == (SPAN, len(wrong))


def test_four_wrong_bits_are_not_repaired(hd):
    weak = [(b, 10 + i) for i, b in enumerate(WEAK8)]
    bad = flip(SPAN, WEAK8[:4])
    assert hd.chase_repair(bad, soft(bad, weak)) is None
    assert hd.chase_repair(bad, soft(bad, weak), repair_flips=4) == (SPAN, 4)       # (the limit is a parameter)


def test_a_wrong_bit_that_is_ninth_in_confidence_is_not_repaired(hd):
    weak = [(b, 10 + i) for i, b in enumerate(WEAK8)] + [((24, 0), 18)]
    bad = flip(SPAN, [(24, 0)])
    assert hd.chase_repair(bad, soft(bad, weak)) is None
    assert hd.chase_repair(bad, soft(bad, weak), repair_bits=9) == (SPAN, 1)
    weak[-1] = ((24, 0), 16)                                          # now it is eighth
    assert hd.chase_repair(bad, soft(bad, weak)) == (SPAN, 1)


def test_ties_go_to_the_earlier_character_then_the_lower_bit(hd):
    # nine bits of one magnitude: the list is the first eight by (character, bit)
    nine = [(10, 0), (10, 1), (12, 0), (12, 1), (13, 0), (15, 0), (15, 2), (16, 0), (16, 1)]
    for i, b in enumerate(nine):
        bad = flip(SPAN, [b])
        got = hd.chase_repair(bad, soft(bad, [(x, 7) for x in nine]))
        assert got == ((SPAN, 1) if i < 8 else None), (i, b, got)
    # bit before character would take (16, 0) in front of (15, 2) and both in front of (16, 1): the same answer; character first is what separates
    # (10, 1) from (12, 0)
    order = sorted(nine)
    assert order == nine


def test_a_trial_that_would_make_an_unprintable_character_is_skipped(hd):
    # a valid sentence whose data holds the byte 0x01; the span shows 'A' there, one weak bit (bit 6) away
    valid = span_of("CHASE", "1,\x01,2")
    at = valid.index("\x01")
    shown = flip(valid, [(at, 6)])
    assert shown[at] == "A"
    assert hd.chase_repair(shown, soft(shown, [((at, 6), 3)])) is None
    # the same distance to a printable byte is repaired
    valid2 = span_of("CHASE", "1,a,2")
    shown2 = flip(valid2, [(valid2.index("a"), 5)])
    assert hd.chase_repair(shown2, soft(shown2, [((valid2.index("a"), 5), 3)])) == (valid2, 1)


def test_the_first_accepted_trial_wins(hd):
    """The CRC's generator x^16 + x^12 + x^5 + 1 has four terms: two sentences that differ in bits 0, 4, 11 and 16 of the bit stream (most significant
    bit of a byte first) share their CRC.  Seen from the span two flips away from both, the order of the list decides."""
    a, b = span_of("CHASE", "1,abc,9"), span_of("CHASE", "1,p`s,9")
    assert a[-4:] == b[-4:]
    i = a.index("abc")
    bits = [(i, 4), (i, 0), (i + 1, 1), (i + 2, 4)]
    assert flip(a, bits) == b
    x = flip(a, bits[:2])
    assert x == flip(b, bits[2:])
    to_a = soft(x, [(bits[0], 1), (bits[1], 2), (bits[2], 3), (bits[3], 4)])
    assert hd.chase_repair(x, to_a) == (a, 2)
    to_b = soft(x, [(bits[2], 1), (bits[3], 2), (bits[0], 3), (bits[1], 4)])
    assert hd.chase_repair(x, to_b) == (b, 2)
    # sizes go first: one flip away from a and three from b, a wins wherever its bit stands in the list
    y = flip(a, bits[:1])
    assert hd.chase_repair(y, soft(y, [(bits[1], 1), (bits[2], 2), (bits[3], 3), (bits[0], 4)])) == (a, 1)


def test_limits_of_zero_switch_the_repair_off(hd):
    bad = flip(SPAN, WEAK8[:1])
    d = soft(bad, [(WEAK8[0], 1)])
    assert hd.chase_repair(bad, d) == (SPAN, 1)
    assert hd.chase_repair(bad, d, repair_bits=0) is None
    assert hd.chase_repair(bad, d, repair_flips=0) is None
    with pytest.raises(hd.HabdecError):
        hd.chase_repair(bad, d, repair_bits=17)
    with pytest.raises(hd.HabdecError):
        hd.chase_repair(bad, d, nbits=5)


def test_the_shape_must_hold(hd):
    """A flip that turns the '*' into another character leaves no sentence: the trial does not count, whatever the CRC field says."""
    star = len(SPAN) - 5
    bad = flip(SPAN, [(star, 0)])                                     # '*' -> '+'
    assert hd.chase_repair(bad, soft(bad, [((star, 0), 1)])) == (SPAN, 1)
    gone = flip(SPAN, [(10, 0)])
    # the only weak bit is the star's: flipping it away cannot count, the wrong bit is strong
    assert hd.chase_repair(gone, soft(gone, [((star, 0), 1)]), repair_bits=1) is None
