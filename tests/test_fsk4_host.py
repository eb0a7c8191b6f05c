"""The Horus Binary 4FSK modem without a GPU: the numpy model of the definition (tests/fsk4_model.py) against itself, and the host restatement
(hd_host_fsk4_*, host/fsk4.hpp) against the model, byte for byte -- slot records, candidate records, delivered frames and counters."""
import json
from pathlib import Path

import numpy as np
import pytest

import fsk4_model as FM
import tones_model as TM

GOLDEN = Path(__file__).resolve().parent / "golden" / "fsk4_ladder.json"
PRESETS = {1: FM.V1, 2: FM.V2}
PUSHES = (1, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def F4():
    from habdec_amd.build import build
    build()
    from habdec_amd import fsk4
    return fsk4


def payload_kinds(fr):
    rng = np.random.default_rng(77)
    return [FM.with_crc(bytes(fr["P"] - 2)), FM.with_crc(b"\xff" * (fr["P"] - 2)), FM.with_crc(rng.integers(0, 256, fr["P"] - 2, dtype=np.uint8).tobytes()),
            bytes(fr["P"]), b"\xff" * fr["P"]]                    # (the last two: all-zero and all-one frames whose CRC is wrong)


# ---------------------------------------------------------------- the model against itself and the encoder

@pytest.mark.parametrize("preset", [1, 2], ids=["v1", "v2"])
def test_format_constants_and_round_trip_on_clean_symbols(F4, preset):
    fr = PRESETS[preset]
    P, K, B = fr["P"], FM.codewords(fr["P"]), FM.body_bytes(fr["P"])
    assert (P, K, B, FM.n_symbols(P)) == ((22, 15, 43, 180) if preset == 1 else (32, 22, 63, 260))
    assert list(FM.scrambler(0x4A80, 16)) == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0]
    assert fr["mul"] == max(p for p in range(2, 8 * B) if all(p % d for d in range(2, int(p ** 0.5) + 1))) and np.gcd(fr["mul"], 8 * B) == 1
    FM.codebook(fr["poly"])                                          # x^23 + 1 mod g = 0, minimum weight 7
    assert FM.crc16(b"123456789") == 0x29B1 == F4.crc16(b"123456789")
    f = F4.frame(preset)
    assert (f.payload_bytes, bytes(f.uw), f.interleave_mul, f.scrambler_seed, f.golay_poly) == (P, bytes(fr["uw"]), fr["mul"], fr["seed"], fr["poly"])
    for payload in payload_kinds(fr):
        frame = FM.encode(payload, fr)
        assert len(frame) == 2 + B and frame[:2] == b"\x24\x24"
        assert F4.horus_encode(payload, preset) == frame                 # the C++ encoder and the model's agree
        if FM.crc16(payload[:-2]) == (payload[-2] | payload[-1] << 8):
            assert F4.horus_encode(payload[:-2], preset) == frame        # (the CRC appended)
        for chase in (0, 4):
            c = FM.decode_candidate(FM.clean_records(FM.symbols(frame)), fr, chase_bits=chase)
            assert c["payload"] == payload and c["corrected"] == 0 and c["uw_errors"] == 0 and c["metric"] == 1000 * FM.n_symbols(P)
            assert c["crc_ok"] == int(FM.crc16(payload[:-2]) == (payload[-2] | payload[-1] << 8))
    assert np.array_equal(F4.symbols(frame), FM.symbols(frame))


@pytest.mark.parametrize("preset", [1, 2], ids=["v1", "v2"])
def test_model_error_handling(preset):
    fr = PRESETS[preset]
    K, nsym = FM.codewords(fr["P"]), FM.n_symbols(fr["P"])
    payload = FM.make_payload(fr, 40 + preset)
    # three wrong bits in every codeword: the hard decoder alone corrects them -- and the default max_corrected refuses the frame
    flips = [(k, b) for k in range(K) for b in (1, 13, 19)]
    c = FM.decode_candidate(FM.clean_records(FM.symbols(FM.encode(payload, fr, flips=flips))), fr, chase_bits=0)
    assert c["payload"] == payload and c["crc_ok"] == 1 and c["corrected"] == 3 * K
    c["slot"] = 0
    assert FM.select([c], fr, 8 << 16, 16)[1]["refused"] == 1 and FM.select([c], fr, 8 << 16, 16, max_corrected=3 * K)[1]["frames"] == 1
    # four wrong bits in one codeword, two of them on unsure symbols: only the soft values repair it
    four = [(5, 2), (5, 7), (5, 13), (5, 20)]
    right, wrong = FM.symbols(FM.encode(payload, fr, flips=four[:2])), FM.symbols(FM.encode(payload, fr, flips=four))
    E = FM.clean_records(wrong)
    for m in np.flatnonzero(right != wrong):
        E[m, wrong[m]], E[m, right[m]] = 650, 350
    hard, soft = FM.decode_candidate(E, fr, chase_bits=0), FM.decode_candidate(E, fr, chase_bits=4)
    assert hard["crc_ok"] == 0 and hard["payload"] != payload and hard["corrected"] == 3
    assert soft["crc_ok"] == 1 and soft["payload"] == payload and soft["corrected"] == 4
    # 0, 2 and 3 wrong bits in the unique word: found, found, passed by at the default gate
    clean = FM.symbols(FM.encode(payload, fr))
    for wrong_bits, xors in ((0, {}), (2, {3: 3}), (2, {0: 1, 7: 2}), (3, {2: 3, 5: 1})):
        s = clean.copy()
        for m, x in xors.items():
            s[m] ^= x
        c = FM.decode_candidate(FM.clean_records(s), fr)
        assert (c is None) == (wrong_bits == 3), (wrong_bits, xors)
        if c:
            assert c["uw_errors"] == wrong_bits and c["payload"] == payload
        assert FM.decode_candidate(FM.clean_records(s), fr, uw_max_errors=3)["uw_errors"] == wrong_bits
    assert nsym == len(clean)


# ---------------------------------------------------------------- the host restatement against the model

def host_run(F4, iq, fsd, baud, f0, spacing, preset, cuts=(4096,), **params):
    """The restatement over iq, pushed in pieces of `cuts` in turn: (every slot record, candidates, frames, counters)."""
    h = F4.HostFsk4(fsd, baud, f0, spacing, preset, **params)
    slots, cands, frames, at, k = [], [], [], 0, 0
    while at < iq.size:
        n, before = min(cuts[k % len(cuts)], iq.size - at), h.stats()["slots"]
        h.push(iq[at:at + n])
        slots.append(h.slots(before, h.stats()["slots"] - before))
        cands.append(h.candidates())
        frames += h.take_frames()
        at += n; k += 1
    return np.concatenate(slots), np.concatenate(cands), frames, h.stats()


def against_model(F4, iq, fsd, baud, f0, spacing, preset, cuts=(4096,), **params):
    fr = PRESETS[preset]
    slots, cands, frames, st = host_run(F4, iq, fsd, baud, f0, spacing, preset, cuts, **params)
    m_slots, m_cands, m_frames, m_cnt = FM.receive(iq, fsd, baud, f0, spacing, fr, **{k: v for k, v in params.items() if k != "max_push"})
    assert slots.dtype == m_slots.dtype and slots.tobytes() == m_slots.tobytes(), np.flatnonzero((slots != m_slots).any(axis=1))[:8]
    assert len(cands) == len(m_cands)
    for c, m in zip(cands, m_cands):
        assert (int(c["slot"]), int(c["metric"]), int(c["crc_ok"]), int(c["corrected"]), int(c["uw_errors"]), c["payload"].tobytes()[:fr["P"]]) == \
            (m["slot"], m["metric"], m["crc_ok"], m["corrected"], m["uw_errors"], m["payload"]), (c, m)
        assert not c["payload"][fr["P"]:].any()
    assert frames == m_frames, (frames, m_frames)
    assert {k: st[k] for k in m_cnt} == m_cnt, (st, m_cnt)
    want = FM.modem(fsd, baud, f0, spacing, params.get("window_q8", 256))
    assert (st["F"], st["W"], st["step"], st["symbols"], st["codewords"]) == (want["F"], want["W"], want["step"], FM.n_symbols(fr["P"]), FM.codewords(fr["P"]))
    return frames, st


def with_specials(iq, at, seed, n=600):
    """NaN, Inf, +-8 and beyond over a stretch of the signal."""
    sp = TM.specials_iq(n=n, seed=seed)
    iq = iq.copy()
    iq[at:at + sp.size] = sp
    return iq


# (samples per symbol; preset; baud, f0, spacing at 32 kS/s; the tones): 8, 2048 and a non-integer number; tones at 0, at the band's edges, all negative
HOST_CASES = {
    "spb8_v1": (1, 4000.0, -6000.0, 4000.0),
    "spb8_v2_tone_at_0": (2, 4000.0, 0.0, 4000.0),
    "spb2048_v1_negative": (1, 15.625, -1500.0, 270.0),
    "spb704_v2_band_edge": (2, 45.45, -15999.99, 10000.0),
}


@pytest.mark.parametrize("case", list(HOST_CASES))
def test_host_restatement_equals_the_model(F4, case):
    preset, baud, f0, spacing = HOST_CASES[case]
    fr, fsd = PRESETS[preset], 32000.0
    spb = fsd / baud
    payload = FM.make_payload(fr, 50 + preset)
    nsym = FM.n_symbols(fr["P"])
    n = int((nsym + 9) * spb)
    iq = FM.fsk4_iq(FM.symbols(FM.encode(payload, fr)), fsd, baud, f0, spacing, sigma=0.2, seed=len(case), start=4.3 * spb, n_samples=n)
    iq = with_specials(iq, int((nsym + 4.8) * spb), 5, min(600, int(3 * spb)))      # behind the frame: they stay in the window for up to a symbol
    frames, st = against_model(F4, iq, fsd, baud, f0, spacing, preset)
    assert [f["payload"] for f in frames] == [payload] and st["gate_passes"] >= 1, (frames, st)
    assert abs(frames[0]["start_sample"] - 4.3 * spb) <= spb / 4 and frames[0]["phase"] == frames[0]["slot"] % 8


def test_host_restatement_equals_the_model_on_noise_and_on_other_parameters(F4):
    """Noise with specials all over it; a narrower window, a wider gate, another chase depth, the guard off."""
    fsd, baud, f0, spacing = 32000.0, 4000.0, -6000.0, 4000.0
    rng = np.random.default_rng(9)
    iq = (0.7 * (rng.standard_normal(9000) + 1j * rng.standard_normal(9000))).astype(np.complex64)
    iq = with_specials(with_specials(iq, 100, 1), 4000, 2)
    against_model(F4, iq, fsd, baud, f0, spacing, 1)
    _, st = against_model(F4, iq, fsd, baud, f0, spacing, 1, window_q8=128, uw_max_errors=4, chase_bits=2, max_corrected=23 * 15)
    assert st["W"] == 4 and st["gate_passes"] > 20


# ---------------------------------------------------------------- cuts

def test_frames_and_counters_do_not_depend_on_the_cuts(F4):
    """8 samples per symbol, so a slot per sample: the restatement's ring holds 8192 slots (max_push 4096), and the second frame straddles its wrap."""
    fsd, baud, f0, spacing = 32000.0, 4000.0, -6000.0, 4000.0
    p = [FM.make_payload(FM.V1, 60), FM.make_payload(FM.V1, 61)]
    one = lambda k, start: FM.fsk4_iq(FM.symbols(FM.encode(p[k], FM.V1)), fsd, baud, f0, spacing, start=start, n_samples=11000)
    rng = np.random.default_rng(3)
    iq = (one(0, 1501.0) + one(1, 7400.0) + 0.25 * (rng.standard_normal(11000) + 1j * rng.standard_normal(11000))).astype(np.complex64)
    whole = host_run(F4, iq, fsd, baud, f0, spacing, 1, cuts=(11000,), max_push=11000)
    assert [f["payload"] for f in whole[2]] == p and whole[2][1]["slot"] < 8192 < whole[2][1]["slot"] + 1440
    for cuts in [(1,), (63,), (64,), (65,), (4097,), PUSHES, (4096,)]:
        got = host_run(F4, iq, fsd, baud, f0, spacing, 1, cuts=cuts, max_push=4097 if 4097 in cuts else 4096)
        assert got[0].tobytes() == whole[0].tobytes() and got[1].tobytes() == whole[1].tobytes(), cuts
        assert got[2] == whole[2] and got[3] == whole[3], (cuts, got[2], got[3])
    m = FM.receive(iq, fsd, baud, f0, spacing, FM.V1)
    assert whole[2] == m[2]


# ---------------------------------------------------------------- the guard against noise

def test_noise_alone_delivers_no_frame(F4):
    fsd, baud, f0, spacing = 32000.0, 4000.0, -6000.0, 4000.0
    rng = np.random.default_rng(2026)
    n = 120000
    iq = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    figures = {}
    for name, max_corrected in (("default", -1), ("off", 23 * 15)):
        h = F4.HostFsk4(fsd, baud, f0, spacing, 1, max_corrected=max_corrected)
        for k in range(0, n, 4096):
            h.push(iq[k:k + 4096])
        figures[name] = (h.stats(), np.array([c["corrected"] for c in h.candidates()]))
    st, corr = figures["default"]
    print("noise:", {k: st[k] for k in ("candidates", "gate_passes", "crc_failures", "refused", "frames")}, "corrected bits per candidate: mean %.2f, min %d, max %d"
          % (corr.mean(), corr.min(), corr.max()), "; guard off (CRC only):", {k: figures["off"][0][k] for k in ("gate_passes", "crc_failures", "refused", "frames")})
    assert st["candidates"] >= 100000 and st["gate_passes"] > 0 and st["frames"] == 0
    assert st["gate_passes"] == st["crc_failures"] + st["refused"]
    # noise corrects about 2.85 bits per codeword -- 1, 23, 253 and 1771 patterns of weight 0 .. 3 -- less what the chase saves: far above 2 K = 30
    assert abs((0 * 1 + 1 * 23 + 2 * 253 + 3 * 1771) / 2048 - 2.85) < 0.005 and corr.min() > 30
    assert figures["off"][0]["refused"] == 0 and figures["off"][0]["gate_passes"] == st["gate_passes"]


# ---------------------------------------------------------------- sensitivity

def ladder_counts(F4, rung, chase_bits):
    """Frames of the rung's signal that the restatement delivers with the right payload."""
    g = json.loads(GOLDEN.read_text())
    fr = PRESETS[g["preset"]]
    iq, payloads = FM.ladder_signal(g, rung)
    h = F4.HostFsk4(g["fsd"], g["baud"], g["f0"], g["spacing"], g["preset"], chase_bits=chase_bits)
    for k in range(0, iq.size, 4096):
        h.push(iq[k:k + 4096])
    frames = h.take_frames()
    assert all(f["payload"] in payloads for f in frames), "a frame nobody sent"
    return len(frames)


def test_sensitivity_ladder(F4):
    """From every frame delivered to none; the fixture's counts are the model's (tools/gen_golden_fsk4.py), the restatement must reproduce them, and the
    soft decoder never delivers fewer frames than the hard one."""
    g = json.loads(GOLDEN.read_text())
    rows = []
    for rung in g["rungs"]:
        hard, soft = ladder_counts(F4, rung, 0), ladder_counts(F4, rung, 4)
        rows.append((rung["sigma"], hard, soft))
        assert (hard, soft) == (rung["delivered_chase0"], rung["delivered_chase4"]), rung
        assert soft >= hard, rung
    print("sigma, delivered of %d at chase_bits 0 and 4:" % g["frames"], rows)
    assert rows[0][1] == rows[0][2] == g["frames"] and rows[-1][1] == rows[-1][2] == 0
