"""The 4FSK tone tracker and the modem's retune without a GPU: the host restatement (hd_host_fsk4_comb_detect, hd_host_fsk4_track_*, hd_host_fsk4_retune)
against the numpy model (tests/fsk4_track_model.py), byte for byte -- detector records, record lists, sums, slot and candidate records, frames."""
import json
from pathlib import Path

import numpy as np
import pytest

import fsk4_model as FM
import fsk4_track_model as M

GOLDEN = Path(__file__).resolve().parent / "golden" / "fsk4_track_ladder.json"
PUSHES = (1, 63, 64, 65, 4097)
FSD, BAUD, SP = M.FSD, M.BAUD, M.SPACING
F0 = -4050.0
DRIFT_BAUD = 1.5                 # case (b): chosen on the CPU -- the untracked model delivers 7 of 12 frames, the tracked model 12 (NOTES.md)


@pytest.fixture(scope="module")
def FT():
    from habdec_amd.build import build
    build()
    from habdec_amd import fsk4_track
    return fsk4_track


@pytest.fixture(scope="module")
def F4(FT):
    from habdec_amd import fsk4
    return fsk4


def pushed(obj, iq, step):
    for at in range(0, iq.size, step or iq.size):
        obj.push(iq[at:at + (step or iq.size)])
    return obj


def est_dicts(a):
    return [dict(M.record_dict(r["rec"]), end_sample=int(r["end_sample"]), epoch=int(r["epoch"])) for r in a]


def frame_key(f):
    return {k: f[k] for k in ("slot", "start_sample", "metric", "payload_bytes", "corrected", "phase", "uw_errors", "payload")}


# ---------------------------------------------------------------- the detector on built spectra

@pytest.mark.parametrize("case", M.built_spectra(), ids=lambda c: c[0])
def test_detector_on_built_spectra(FT, case):
    name, acc, search, valid = case
    plan = M.comb_plan(FSD, *search)
    want = M.comb_detect(acc, plan)
    got = M.record_dict(FT.comb_detect(acc, FSD, *search))
    assert got == want
    assert got["valid"] == valid
    if name in ("zeros", "nan"):
        assert got == M.ZERO
    if name == "clean":
        assert abs(M.f0_hz(got, FSD) - (1500.3 - 2048) * M.BIN) < 0.02 * BAUD and abs(M.spacing_hz(got, FSD) - 345.6 * M.BIN) < 0.01 * BAUD
    if name == "edges":
        assert (plan["b_lo"], plan["b_hi"], plan["d_lo"], plan["d_hi"]) == (1000, 2101, 1382, 1382) and (got["c0"], got["d"]) == (1032, 1382)
    if name == "tie":
        # a window of 65 lies inside a plateau of 101 over 37 centres: the lowest d that puts four windows inside is 1336, its lowest c0 1518
        assert (got["c0"], got["d"]) == (1518, 1336)
    if name == "known_spacing":
        assert got["d"] == round(4 * SP / M.BIN) and got["spacing_q8"] == 64 * got["d"]
    if name in ("three_of_four", "carrier", "rtty_pair"):
        assert got["quality_q8"] < 16                                # the weakest window holds the floor alone


def test_segments_and_quality_gate_validity(FT):
    _, acc, search, _ = M.built_spectra()[0]
    assert FT.comb_detect(acc, FSD, *search, segments_ok=False)["valid"] == 0
    q = int(FT.comb_detect(acc, FSD, *search)["quality_q8"])
    assert FT.comb_detect(acc, FSD, *search, min_quality_q8=q)["valid"] == 1 and FT.comb_detect(acc, FSD, *search, min_quality_q8=q + 1)["valid"] == 0


def test_refusals(FT):
    from habdec_amd import HabdecError
    acc = M.built_spectra()[0][1]
    assert M.comb_plan(FSD, BAUD, 1.99 * BAUD, 3 * BAUD, -12000, 12000) == "unsupported"
    with pytest.raises(HabdecError, match="error -"):
        FT.comb_detect(acc, FSD, BAUD, 1.99 * BAUD, 3 * BAUD, -12000, 12000)          # a spacing below 2 baud
    assert M.comb_plan(FSD, BAUD, 2 * BAUD, 3 * BAUD, -1000, 1000) == "invalid"
    with pytest.raises(HabdecError):
        FT.comb_detect(acc, FSD, BAUD, 2 * BAUD, 3 * BAUD, -1000, 1000)               # a band that holds no comb
    with pytest.raises(HabdecError):
        FT.HostFsk4Track(FSD, BAUD, 1.0 * BAUD, 1.0 * BAUD, -12000, 12000)            # known spacing, below 2 baud
    lib = FT.lib()
    import ctypes as C
    from habdec_amd import capi
    p = capi.hd_fsk4_comb_params(BAUD, 1.99 * BAUD, 3 * BAUD, -12000.0, 12000.0, 0, 1)
    out = np.ones(1, capi.FSK4_COMB_RECORD_DTYPE)
    assert lib.hd_host_fsk4_comb_detect(acc.ctypes.data, FSD, C.byref(p), out.ctypes.data) < 0
    assert M.record_dict(out[0]) == M.ZERO


# ---------------------------------------------------------------- the object: however the samples are cut

@pytest.fixture(scope="module")
def signal():
    return M.frames_signal(4, F0, 0.4 * BAUD)                        # 31232 samples: three epochs of four segments, their ends inside pushes


def test_object_against_the_model_however_it_is_cut(FT, signal):
    iq, _ = signal
    args = M.ladder_args(M.LADDER)
    want, acc, _ = M.track(FT, iq, *args, decay_q8=160)
    assert len(want) == 3 and [r["end_sample"] for r in want] == [10240, 18432, 26624] and all(r["valid"] for r in want)
    for step in PUSHES + (0,):
        h = pushed(FT.HostFsk4Track(*args, decay_q8=160), iq, step)
        assert est_dicts(h.records()) == want, step
        assert np.array_equal(h.acc(), acc)
        assert h.stats() == dict(samples=iq.size, segments=(iq.size - 4096) // 2048 + 1, epochs=3, valid_epochs=3, retunes=0)
    e = h.records()[-1]
    assert float(e["f0_hz"]) == M.f0_hz(want[-1], FSD) and float(e["spacing_hz"]) == M.spacing_hz(want[-1], FSD)


# ---------------------------------------------------------------- the modem's retune

RETUNES = [(3001, F0 + 21.0, SP - 6.0), (7919, F0 - 13.0, SP + 9.0)]


@pytest.fixture(scope="module")
def two_frames():
    return M.frames_signal(2, F0, 0.0, sigma=0.3)[0]


def test_a_retune_to_the_same_tones_changes_nothing(F4, two_frames):
    iq = two_frames
    plain = pushed(F4.HostFsk4(FSD, BAUD, F0, SP, 1), iq, 0)
    for at in (1, 777, 4096, 9001):
        h = F4.HostFsk4(FSD, BAUD, F0, SP, 1)
        h.retune(F0, SP, at)
        pushed(h, iq, 4097)
        g = h.stats()["slots"]
        assert np.array_equal(h.slots(0, g), plain.slots(0, g))
        assert h.retune_stats() == dict(retunes=1, late=0, waiting=0, psi=[0, 0, 0, 0])
        assert [frame_key(f) for f in h.take_frames()] == [frame_key(f) for f in pushed(F4.HostFsk4(FSD, BAUD, F0, SP, 1), iq, 0).take_frames()]


def test_two_retunes_against_the_model_for_every_cut(F4, two_frames):
    iq = two_frames
    slots, cands, frames, counters = M.receive_retuned(iq, FSD, BAUD, F0, SP, FM.V1, RETUNES)
    assert len(frames) == 2                                          # small steps with a continuous phase cost no frame
    assert not np.array_equal(slots, FM.slot_records(iq, FSD, BAUD, F0, SP))
    for step in PUSHES + (0,):
        h = F4.HostFsk4(FSD, BAUD, F0, SP, 1, max_push=16384)
        for at, f0, sp in RETUNES:
            h.retune(f0, sp, at)
        pushed(h, iq, step)
        g = h.stats()["slots"]
        assert g == slots.shape[0]
        assert np.array_equal(h.slots(0, g), slots)
        got = h.candidates()
        assert [(int(c["slot"]), int(c["metric"]), int(c["crc_ok"]), int(c["corrected"]), int(c["uw_errors"]), c["payload"].tobytes()[:22]) for c in got] == \
            [(c["slot"], c["metric"], c["crc_ok"], c["corrected"], c["uw_errors"], c["payload"]) for c in cands]
        assert [frame_key(f) for f in h.take_frames()] == [frame_key(f) for f in frames]
        assert h.retune_stats()["retunes"] == 2 and h.retune_stats()["late"] == 0


def test_a_late_retune_is_counted_and_takes_effect_at_once(F4, two_frames):
    iq = two_frames
    h = F4.HostFsk4(FSD, BAUD, F0, SP, 1, max_push=16384)
    h.push(iq[:5000])
    h.retune(F0 + 21.0, SP - 6.0, 3001)                              # behind the stream's index: in force from sample 5000
    assert h.retune_stats()["late"] == 1 and h.retune_stats()["retunes"] == 1 and h.stats()["step"] == M.steps(FSD, F0 + 21.0, SP - 6.0)
    h.push(iq[5000:])
    want = M.slot_records_retuned(iq, FSD, BAUD, F0, SP, [(5000, F0 + 21.0, SP - 6.0)])
    g = h.stats()["slots"]
    assert np.array_equal(h.slots(0, g), want)
    from habdec_amd import HabdecError
    with pytest.raises(HabdecError):
        h.retune(15000.0, SP, 0)                                     # a tone outside +- fsd / 2
    with pytest.raises(HabdecError):
        F4.HostFsk4(FSD).retune(F0, SP, 0)                           # no modem


# ---------------------------------------------------------------- the accuracy ladder and noise alone

def test_ladder(FT):
    g = json.loads(GOLDEN.read_text())
    assert {k: g[k] for k in M.LADDER} == M.LADDER
    got = M.ladder(g, M.host_detect(FT, g))
    assert got == g["cells"]                                         # the restatement reproduces the model's file
    for c in got:
        print(c)
        if c["sigma"] == 0.6 and c["segments"] >= 4:
            assert max(c["err_baud"]) <= 0.1                         # NOTES.md's nothing-lost bound of the modem


def test_noise_alone_is_never_valid(FT):
    """200 epochs of noise through a tracker at the default parameters: no valid record.  And where the default threshold lies."""
    g = json.loads(GOLDEN.read_text())
    rng = np.random.default_rng(M.NOISE["seed"])
    n = M.HOP * (M.NOISE["epochs"] * 4 + 1)
    h = FT.HostFsk4Track(*M.ladder_args(g))                         # the defaults: epochs of 4 segments, decay 128, min_quality_q8 192
    h.push((M.NOISE["sigma"] * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64))
    assert h.stats()["epochs"] == M.NOISE["epochs"] and h.stats()["valid_epochs"] == 0 and not h.records()["rec"]["valid"].any()
    q = M.noise_qualities(FT, g)                                     # the same noise, every epoch on its own and no threshold
    threshold = M.DEFAULTS["min_quality_q8"]
    import ctypes as C
    from habdec_amd import capi
    p = capi.hd_fsk4_track_params()
    FT.lib().hd_fsk4_track_params_default(C.byref(p))
    assert p.min_quality_q8 == threshold
    weakest = min(c["quality_min"] for c in g["cells"] if c["sigma"] == 1.0)
    print("largest quality of noise", max(q), "with decay", int(h.records()["rec"]["quality_q8"].max()), "default", threshold,
          "weakest of the ladder's sigma 1.0 row", weakest)
    assert max(q) < threshold < weakest


# ---------------------------------------------------------------- end to end: tracker and modem, model and restatement

def end_to_end(FT, F4, iq, f0_modem, tracked, step=0):
    m = F4.HostFsk4(FSD, BAUD, f0_modem, SP, 1)
    t = FT.HostFsk4Track(*M.ladder_args(M.LADDER))
    if tracked:
        t.attach(m)
    for at in range(0, iq.size, step or iq.size):                    # the documented order: the tracker first
        t.push(iq[at:at + (step or iq.size)])
        m.push(iq[at:at + (step or iq.size)])
    return m.take_frames(), m.candidates(), t


def model_end_to_end(FT, iq, f0_modem, tracked):
    retunes = M.track(FT, iq, *M.ladder_args(M.LADDER), modem_phi=M.steps(FSD, f0_modem, SP))[2] if tracked else []
    return M.receive_retuned(iq, FSD, BAUD, f0_modem, SP, FM.V1, retunes), retunes


@pytest.mark.parametrize("case", ["acquisition", "drift"])
def test_end_to_end(FT, F4, case):
    f0_modem, drift = (F0 - 1.0 * BAUD, 0.0) if case == "acquisition" else (F0, DRIFT_BAUD * BAUD)
    iq, payloads = M.frames_signal(12, F0, drift)
    (_, _, plain, _), _ = model_end_to_end(FT, iq, f0_modem, False)
    (_, cands, tracked, _), retunes = model_end_to_end(FT, iq, f0_modem, True)
    good_plain, good = [f["payload"] for f in plain if f["payload"] in payloads], [f["payload"] for f in tracked if f["payload"] in payloads]
    print(case, "untracked", len(good_plain), "tracked", len(good), "retunes", [r[0] for r in retunes])
    if case == "acquisition":
        assert len(plain) == 0
        first = retunes[0][0]
        assert good == [p for k, p in enumerate(payloads) if k * 180 * 32 >= first] and len(good) == 10
    else:
        assert len(good_plain) <= 8 and good == payloads
    assert len(tracked) == len(good)
    for step in (0, 4097):
        frames, hc, t = end_to_end(FT, F4, iq, f0_modem, True, step)
        assert [frame_key(f) for f in frames] == [frame_key(f) for f in tracked]
        assert [(int(c["slot"]), int(c["metric"]), int(c["corrected"])) for c in hc] == [(c["slot"], c["metric"], c["corrected"]) for c in cands]
        assert t.stats()["retunes"] == len(retunes)
    assert [frame_key(f) for f in end_to_end(FT, F4, iq, f0_modem, False)[0]] == [frame_key(f) for f in plain]
