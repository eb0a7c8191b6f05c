"""The AFSK / AX.25 modem on the host (hd_host_afsk_*, hd_host_ax25_*) against the numpy model (tests/afsk_model.py), byte for byte -- no GPU.

Slot records, candidate records, delivered frames and counters of the restatement equal the model's for every case of tests/afsk_cases.py and every cut
of the input; the cases' own expectations (which frames come out, with how many flips) are asserted beside that."""
import json
from pathlib import Path

import numpy as np
import pytest

import afsk_cases as K
from afsk_model import AfskModel, crc16
from habdec_amd import afsk
from habdec_amd.afsk import HostAfsk

GOLDEN = Path(__file__).resolve().parent / "golden" / "afsk_ladder.json"


@pytest.fixture(scope="module")
def cases():
    return K.frame_cases()


def run_host(modem, params, row, pieces=None):
    h = HostAfsk(K.FS, *modem, **params)
    for a, b in pieces or [(0, row.size)]:
        h.push(row[a:b])
    return h


def run_model(modem, params, row):
    m = AfskModel(K.FS, *modem, **params)
    for a in range(0, row.size, 8192):
        m.push(row[a:a + 8192])
    return m


def same(h: HostAfsk, m: AfskModel):
    """Counters, frames, candidates and the newest slots of the restatement equal the model's."""
    assert h.stats() == m.stats()
    n = min(m.g - m.d0, 60000)
    assert np.array_equal(h.slots(m.g - n, n), m.slot(np.arange(m.g - n, m.g)))
    ch = afsk._frames(h.candidates())
    assert ch == m.candidates
    fh, fm = h.take_frames(), m.take_frames()
    assert fh == fm
    return fh, ch


def test_crc_check_value():
    assert afsk.crc16(b"123456789") == 0x906E == crc16(b"123456789")


def test_hand_assembled_frame_round_trips():
    # APRS <- N0CALL-11 via WIDE1-1* and WIDE2-2, UI, no layer 3, ">hi\x01"
    frame = bytes([0x82, 0xA0, 0xA4, 0xA6, 0x40, 0x40, 0x60,          # A P R S _ _, SSID 0
                   0x9C, 0x60, 0x86, 0x82, 0x98, 0x98, 0x76,          # N 0 C A L L, SSID 11
                   0xAE, 0x92, 0x88, 0x8A, 0x62, 0x40, 0xE2,          # W I D E 1 _, SSID 1, H
                   0xAE, 0x92, 0x88, 0x8A, 0x64, 0x40, 0x65,          # W I D E 2 _, SSID 2, last
                   0x03, 0xF0, 0x3E, 0x68, 0x69, 0x01])
    made = afsk.ax25_frame("N0CALL-11>APRS,WIDE1-1*,WIDE2-2", b">hi\x01")
    assert made[:-2] == frame and made[-2] | made[-1] << 8 == crc16(frame)
    assert afsk.ax25_format(frame) == "N0CALL-11>APRS,WIDE1-1*,WIDE2-2:>hi<0x01>"
    assert K.ui_frame(b">hi\x01", digis=(("WIDE1", 1, True), ("WIDE2", 2, False))) == made
    # the encoder's levels are the bits of this file, stuffed, flagged and NRZI-coded
    assert afsk.ax25_levels(made, 3, 2).tolist() == K.nrzi(K.on_air([made], before=3, after=2))
    assert afsk.ax25_encode("N0CALL-11>APRS,WIDE1-1*,WIDE2-2", b">hi\x01", 3, 2).tolist() == K.nrzi(K.on_air([made], before=3, after=2))
    with pytest.raises(afsk.HabdecError):
        afsk.ax25_format(frame[:28] + b"\x13\xf0")                    # an I frame is not UI
    with pytest.raises(afsk.HabdecError):
        afsk.ax25_frame("N0CALL-16>APRS")
    # the longest line: a frame of 332 bytes whose information is nothing printable, six characters a byte
    worst = afsk.ax25_frame("N0CALL-11>APRS", b"\xff" * (332 - 18))[:-2]
    assert afsk.ax25_format(worst) == "N0CALL-11>APRS:" + "<0xFF>" * 314
    import ctypes as C
    small = C.create_string_buffer(15 + 6 * 314)                      # one short of the line and its terminating 0
    d = np.frombuffer(worst, np.uint8)
    assert afsk.lib().hd_host_ax25_format(d.ctypes.data, d.size, small, len(small)) == -4
    assert afsk.lib().hd_host_ax25_format(d.ctypes.data, d.size, C.create_string_buffer(16 + 6 * 314), 16 + 6 * 314) == 15 + 6 * 314


def test_modem_limits():
    for fs, baud in ((9600.0, 1200.0), (2048.0 * 300.0, 300.0)):     # 8 and 2048 samples per bit
        mark, space = (1200.0, 2200.0) if baud == 1200.0 else (1600.0, 1800.0)
        h, m = HostAfsk(fs, baud, mark, space), AfskModel(fs, baud, mark, space)
        assert h.stats()["F"] == m.F and h.stats()["W"] == m.W == round(fs / baud) and h.stats()["step"] == m.phi
    for fs, baud in ((9599.0, 1200.0), (2049.0 * 300.0, 300.0)):
        with pytest.raises(afsk.HabdecError, match="error -3"):
            HostAfsk(fs, baud)
    for mark, space in ((0.0, 2200.0), (1200.0, 16000.0), (1200.0, 0.0), (16000.0, 2200.0), (1700.0, 1700.0)):
        with pytest.raises(afsk.HabdecError, match="error -1"):
            HostAfsk(K.FS, 1200.0, mark, space)
    for bad in (dict(max_frame_bytes=16), dict(max_frame_bytes=333), dict(repair_flips=5), dict(repair_bits=11), dict(repair_bits=64, repair_flips=1),
                dict(max_push=40000)):
        with pytest.raises(afsk.HabdecError):
            HostAfsk(K.FS, **bad)
    assert HostAfsk(K.FS, repair_bits=10).h and HostAfsk(K.FS, repair_bits=63, repair_flips=1).h and HostAfsk(K.FS, repair_bits=7, repair_flips=3).h


@pytest.mark.parametrize("name", sorted(K.frame_cases()))
def test_case_equals_model_and_delivers_what_it_should(cases, name):
    modem, params, row, expect = cases[name]
    frames, cands = same(run_host(modem, params, row), run_model(modem, params, row))
    print(name, [(f["flips"], f["phase"], f["len"]) for f in frames], np.bincount([c["result"] for c in cands], minlength=7))
    assert [(f["data"], f["flips"]) for f in frames] == expect
    if name == "abort_inside":
        assert any(c["result"] == afsk.ABORT and c["bits"] > 100 for c in cands)
    if name == "open_walk":
        assert any(c["result"] == afsk.OPEN for c in cands)
    if name in ("16_bytes_unshaped", "one_byte_more_unshaped"):
        assert any(c["result"] == afsk.UNSHAPED and c["bits"] > 100 for c in cands)
    if name in ("repair_3_fails", "repair_off", "false_closing_flag"):
        assert any(c["result"] == afsk.FCS_FAILED for c in cands) and not any(c["result"] in (afsk.PLAIN, afsk.REPAIRED) for c in cands)
    if name == "false_closing_flag":
        assert any(c["result"] == afsk.FCS_FAILED and c["len"] == 17 for c in cands)     # the walk closed behind 17 bytes, and no pattern may move that
    if name in ("repair_refused_callsign", "plain_refused_callsign"):
        assert any(c["result"] == afsk.REFUSED for c in cands)


@pytest.mark.parametrize("name", ["plain", "shared_flag", "repair_2", "max_332"])
def test_cuts_do_not_matter(cases, name):
    modem, params, row, expect = cases[name]
    row = K.specials(row) if name == "shared_flag" else row
    whole = run_host(modem, params, row)
    for shift in (0, 3):
        cut = run_host(modem, params, row, list(K.cuts(row.size, shift=shift)))
        assert cut.stats() == whole.stats()
        n = min(whole.stats()["slots"], 30000)
        first = whole.stats()["slots"] - n
        assert np.array_equal(cut.slots(first, n), whole.slots(first, n))
        assert np.array_equal(cut.candidates(), run_host(modem, params, row).candidates())
        assert cut.take_frames() == run_host(modem, params, row).take_frames()
    m = run_model(modem, params, row)
    same(whole, m)


def test_specials_in_the_row(cases):
    modem, params, row, _ = cases["plain"]
    bad = K.specials(row)
    assert np.isnan(bad).sum() == 8 and np.isinf(bad).sum() == 16
    same(run_host(modem, params, bad), run_model(modem, params, bad))
    # a row of nothing but specials
    odd = np.tile(np.array([np.nan, np.inf, -np.inf, 5, -5, 0.25], np.float32), 3000)
    same(run_host(modem, params, odd), run_model(modem, params, odd))


def test_reset_and_set_modem_start_the_stream_again(cases):
    modem, params, row, expect = cases["plain"]
    h = run_host(modem, params, row)
    first = (h.stats(), h.candidates().tobytes())
    h.reset()
    assert h.stats()["samples"] == 0 and h.stats()["F"] == first[0]["F"] and len(h.take_frames()) == 1      # frames not taken stay
    h.push(row)
    assert (h.stats(), h.candidates().tobytes()) == first
    h.set_modem(*K.HF)
    assert h.stats()["samples"] == 0 and h.stats()["W"] == 107
    assert HostAfsk(K.FS).push(row) == 0                                  # no modem: passed by


def test_noise_delivers_nothing():
    """60 s of Gaussian noise at 32 kS/s through the model (and the restatement) with the defaults: no frame.  DESIGN.md item 17 expects about 2^-8 of
    the bit positions of a phase to be flags and roughly a percent of those to walk to a shaped frame; the counts are printed beside that, the
    condition is on the frames alone."""
    rng = np.random.default_rng(2026)
    row = (0.5 * rng.standard_normal(int(60 * K.FS))).astype(np.float32)
    m, h = AfskModel(K.FS, *K.BELL), HostAfsk(K.FS, *K.BELL)
    for a in range(0, row.size, 4096):
        m.push(row[a:a + 4096])
        h.push(row[a:a + 4096])
    s = m.stats()
    shaped = sum(c["result"] >= afsk.FCS_FAILED for c in m.candidates)
    print("slots", s["slots"], "flags", s["flags"], "expected about", s["slots"] / 256, "unshaped", s["unshaped"], "shaped", shaped)
    assert h.stats() == s
    assert m.take_frames() == [] and h.take_frames() == []
    assert s["frames_plain"] == s["frames_repaired"] == 0


def ladder_row(entry, sigma, seed):
    f = K.ui_frame(bytes(entry["info"], "latin-1"))
    row = K.row_of(K.nrzi(K.on_air([f])), K.BELL, dict(max_frame_bytes=entry["max_frame_bytes"]), start=entry["start"])
    rng = np.random.default_rng(seed)
    return f, (row + sigma * rng.standard_normal(row.size)).astype(np.float32)


def test_ladder_replays_through_the_restatement():
    gold = json.loads(GOLDEN.read_text())
    seen = set()
    for level in gold["levels"]:
        outcomes = []
        for run in level["runs"]:
            f, row = ladder_row(gold, level["sigma"], run["seed"])
            h = HostAfsk(K.FS, *K.BELL, max_frame_bytes=gold["max_frame_bytes"])
            h.push(row)
            got = [fr for fr in h.take_frames() if fr["data"] == f[:-2]]
            outcome = "lost" if not got else "repaired" if got[0]["flips"] else "plain"
            assert (outcome, got[0]["flips"] if got else 0) == (run["outcome"], run["flips"]), (level["sigma"], run)
            outcomes.append(outcome)
        print(level["sigma"], outcomes)
        seen.add(frozenset(outcomes))
    assert any("repaired" in s for s in seen) and frozenset({"lost"}) in seen
