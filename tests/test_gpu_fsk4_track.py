"""The 4FSK tone tracker and the modem's retune on the GPU (hd_fsk4_track_*, hd_fsk4_retune; kernels/fsk4_track.hip, kernels/fsk4.hip).

The detector is integer arithmetic behind the quantisation: k_fsk4_comb's records are compared byte for byte with the host restatement on the same sums,
and the retuned modem's slot and candidate records with the restatement's.  The spectrum in front of the detector is the tone search's: the device makes it
with a float transform, the restatement with a double one, so sums agree to the float transform's error (tests/test_gpu_tone_search.py) and not to the bit.
The object's records are therefore held (a) to the host detector on the device's own sums, byte for byte, (b) to each other however the samples are
cut and through either door, byte for byte, and (c) to the restatement's within the transform's error."""
import numpy as np
import pytest

import fsk4_model as FM
import fsk4_track_model as M

pytestmark = pytest.mark.gpu
PUSHES = (1, 63, 64, 65, 4097)
HD_ERR_INVALID, HD_ERR_UNSUPPORTED, HD_ERR_CAPACITY = -1, -3, -4
FSD, BAUD, SP = M.FSD, M.BAUD, M.SPACING                        # 32000: the decimated rate of a default engine
F0 = -4050.0
SEARCH = M.ladder_args(M.LADDER)[1:]


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def F4(hd):
    from habdec_amd import fsk4
    return fsk4


@pytest.fixture(scope="module")
def FT(hd):
    from habdec_amd import fsk4_track
    return fsk4_track


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def frame_key(f):
    return {k: f[k] for k in ("slot", "start_sample", "metric", "payload_bytes", "corrected", "phase", "uw_errors", "payload")}


# ---------------------------------------------------------------- the comb kernel on built spectra

def test_comb_records_equal_the_host_restatement_on_built_spectra(hd, FT):
    """One launch over all the built spectra as streams, and one stream that is not due: its record and its sums stay."""
    cases = M.built_spectra()
    S = len(cases) + 1
    eng = hd.Engine(n_streams=S)
    assert eng.L.hd_engine_decimated_rate(eng.h) == FSD
    tr = FT.Fsk4Track(eng, decay_q8=192)
    spectra = np.zeros((S, 4096))
    for s, (_, acc, search, _) in enumerate(cases):
        tr.set_stream(s, *search)
        spectra[s] = acc
    spectra[S - 1] = cases[0][1]
    tr.set_stream(S - 1, *cases[0][2])
    due = np.ones(S, np.uint32)
    due[S - 1] = 0
    got = tr.debug_comb(spectra, due, np.ones(S, np.uint32))
    for s, (name, acc, search, valid) in enumerate(cases):
        want = FT.comb_detect(acc, FSD, *search)
        assert got[s].tobytes() == want.tobytes(), (name, M.record_dict(got[s]), M.record_dict(want))
        assert int(got[s]["valid"]) == valid, name
        after = tr.debug_acc(s)
        if name != "nan":
            assert np.array_equal(after, acc * 0.75), name             # the decay: one rounding per bin
        else:
            assert np.isnan(after[777]) and np.array_equal(np.delete(after, 777), np.delete(acc, 777) * 0.75)
    assert got[S - 1].tobytes() == bytes(64) and np.array_equal(tr.debug_acc(S - 1), spectra[S - 1])      # not due: untouched
    without = tr.debug_comb(spectra, due, np.zeros(S, np.uint32))
    assert not without["valid"].any() and np.array_equal(without["quality_q8"], got["quality_q8"])         # no segments, no validity
    for s in range(S):
        assert tr.debug_guards(s) == 0
    eng.close()


# ---------------------------------------------------------------- the object

def reference_run(hd, FT, iq_rows, decay):
    """Every stream pushed whole, one epoch at a time: records, and the sums behind every epoch's end."""
    S = len(iq_rows)
    eng = hd.Engine(n_streams=S)
    tr = FT.Fsk4Track(eng, max_push=40000, decay_q8=decay)
    for s in range(S):
        tr.set_stream(s, *SEARCH)
    sums, at = [[] for _ in range(S)], 0
    for end in (10240, 18432, 26624, len(iq_rows[0])):
        tr.push_host(np.stack([r[at:end] for r in iq_rows]))
        for s in range(S):
            sums[s].append(tr.debug_acc(s))
        at = end
    out = [tr.debug_records(s) for s in range(S)], sums, [tr.debug_acc(s) for s in range(S)]
    eng.close()
    return out


@pytest.fixture(scope="module")
def rows():
    return [M.frames_signal(4, F0 + 300.0 * s, 0.3 * BAUD * s, seed=50 + s)[0] for s in range(3)]           # 31232 samples: three epochs


def test_records_are_the_host_detectors_on_the_devices_own_sums(hd, FT, rows):
    """Without decay the sums behind an epoch's end are the sums its detector saw."""
    recs, sums, _ = reference_run(hd, FT, rows, 256)
    for s in range(len(rows)):
        assert len(recs[s]) == 3 and [int(e) for e in recs[s]["end_sample"]] == [10240, 18432, 26624] and recs[s]["rec"]["valid"].all()
        for k in range(3):
            want = FT.comb_detect(sums[s][k], FSD, *SEARCH)
            assert recs[s][k]["rec"].tobytes() == want.tobytes(), (s, k)
            assert float(recs[s][k]["f0_hz"]) == M.f0_hz(M.record_dict(want), FSD) and float(recs[s][k]["spacing_hz"]) == M.spacing_hz(M.record_dict(want), FSD)
        # and the restatement, whose transform is a double one: its sums within the float transform's error, its tones within a hundredth of a baud
        h = FT.HostFsk4Track(FSD, *SEARCH, decay_q8=256)
        h.push(rows[s])
        assert np.allclose(sums[s][3], h.acc(), rtol=1e-3, atol=1e-6 * h.acc().max())
        mine = h.records()
        assert np.abs(mine["f0_hz"] - recs[s]["f0_hz"]).max() < 0.01 * BAUD and np.abs(mine["spacing_hz"] - recs[s]["spacing_hz"]).max() < 0.01 * BAUD


def test_object_through_both_doors_however_it_is_cut(hd, FT, torch, rows):
    """Push sizes 1, 63, 64, 65 and 4097 in turn, shifted from stream to stream, one stream empty in every third push, one push longer than
    HD_TONE_SEARCH_CHUNK, a stream without a search: record lists and sums (after the decay) equal those of whole-epoch pushes, byte for byte."""
    S, N = len(rows) + 1, len(rows[0])
    big = np.tile(rows[0], 4)[:100000]                                # stream 0 takes one push of 70000 samples: epochs end inside it
    data = [big] + list(rows[1:])
    want_recs, _, want_acc = {}, None, {}
    eng0 = hd.Engine(n_streams=1)
    t0 = FT.Fsk4Track(eng0, max_push=100000, decay_q8=160)
    for s, d in enumerate(data):
        t0.set_stream(0, *SEARCH)
        t0.push_host(d[None, :])
        want_recs[s], want_acc[s] = t0.debug_records(0), t0.debug_acc(0)
    eng0.close()
    assert len(want_recs[0]) == 11 and len(want_recs[1]) == 3
    eng = hd.Engine(n_streams=S)
    doors = {"host memory": FT.Fsk4Track(eng, max_push=100000, decay_q8=160), "device memory": FT.Fsk4Track(eng, max_push=100000, decay_q8=160)}
    for tr in doors.values():
        for s in range(S - 1):
            tr.set_stream(s, *SEARCH)
    at, push, stride = [0] * S, 0, 70000
    sizes = [len(d) for d in data] + [5000]
    while any(at[s] < sizes[s] for s in range(S)):
        n = np.array([PUSHES[(push + 2 * s) % len(PUSHES)] for s in range(S)], np.uint32)
        if push == 4:
            n[0] = 70000                                             # longer than HD_TONE_SEARCH_CHUNK
        if push > 8:
            n[:] = 8000 - 7 * np.arange(S)                           # (the rest in larger steps)
        if push % 3 == 0:
            n[push // 3 % S] = 0
        n = np.minimum(n, [sizes[s] - at[s] for s in range(S)]).astype(np.uint32)
        slab = np.full((S, stride), np.nan + 1j * np.nan, np.complex64)
        for s in range(S):
            slab[s, :n[s]] = data[s][at[s]:at[s] + n[s]] if s < S - 1 else 1.0
            at[s] += int(n[s])
        doors["host memory"].push_host(slab, n)
        d = torch.from_numpy(slab.view(np.float32)).cuda()
        doors["device memory"].push_device(d.data_ptr(), stride, n)
        del d
        push += 1
    for what, tr in doors.items():
        for s in range(S - 1):
            assert tr.debug_records(s).tobytes() == want_recs[s].tobytes(), (what, s)
            assert tr.debug_acc(s).tobytes() == want_acc[s].tobytes(), (what, s)
            st = tr.stats(s)
            assert (st["samples"], st["epochs"], st["segments"]) == (sizes[s], len(want_recs[s]), (sizes[s] - 4096) // 2048 + 1), (what, s, st)
            assert tr.estimate(s)["end_sample"] == int(want_recs[s][-1]["end_sample"])
        assert tr.stats(S - 1) == dict(samples=0, segments=0, epochs=0, valid_epochs=0, retunes=0)       # no search: no samples taken
        for s in range(S):
            assert tr.debug_guards(s) == 0, (what, s)
    tr = doors["host memory"]
    tr.reset(1)
    assert tr.stats(1)["samples"] == 0 and len(tr.debug_records(1)) == 0 and not tr.debug_acc(1).any() and len(tr.debug_records(2)) == 3
    eng.close()


# ---------------------------------------------------------------- the modem's retune

RETUNES = [(3001, F0 + 21.0, SP - 6.0), (7919, F0 - 13.0, SP + 9.0)]


@pytest.mark.parametrize("step", [4097, 6000])
def test_retuned_slot_and_candidate_records_equal_the_restatement(hd, F4, step):
    iq = M.frames_signal(2, F0, 0.0, sigma=0.3)[0]
    ref = F4.HostFsk4(FSD, BAUD, F0, SP, 1, max_push=16384)
    eng = hd.Engine(n_streams=2)
    f = F4.Fsk4(eng, max_push=16384)
    f.set_modem(0, BAUD, F0, SP, 1)
    f.set_modem(1, BAUD, F0, SP, 1)                                  # stream 1 is not retuned: the cut of stream 0 must not touch it
    plain = F4.HostFsk4(FSD, BAUD, F0, SP, 1, max_push=16384)
    for at, f0, sp in RETUNES:
        ref.retune(f0, sp, at)
        f.retune(0, f0, sp, at)
    assert f.retune_stats(0) == dict(retunes=0, late=0, waiting=2, psi=[0, 0, 0, 0])
    for at in range(0, iq.size, step):
        part = iq[at:at + step]
        ref.push(part); plain.push(part)
        f.push_host(np.stack([part, part]))
    g = ref.stats()["slots"]
    assert f.stats(0) == ref.stats() and f.stats(1) == plain.stats() and f.stats(0)["step"] != f.stats(1)["step"]
    assert f.debug_slots(0, 0, g).tobytes() == ref.slots(0, g).tobytes()
    assert f.debug_slots(1, 0, g).tobytes() == plain.slots(0, g).tobytes()
    assert f.debug_candidates(0).tobytes() == ref.candidates().tobytes()
    assert [frame_key(x) for x in f.take_frames(0)] == [frame_key(x) for x in ref.take_frames()]
    assert f.retune_stats(0) == ref.retune_stats() and f.retune_stats(0)["retunes"] == 2 and f.retune_stats(1)["retunes"] == 0
    f.retune(0, F0, SP, 5)                                           # late: at once
    ref.retune(F0, SP, 5)
    assert f.retune_stats(0) == ref.retune_stats() and f.retune_stats(0)["late"] == 1 and f.stats(0)["step"] == ref.stats()["step"]
    for s in range(2):
        assert f.debug_guards(s) == 0
    eng.close()


# ---------------------------------------------------------------- closing the loop

@pytest.mark.parametrize("case", ["acquisition", "drift"])
def test_end_to_end_through_attach(hd, F4, FT, case):
    """Twelve V1 frames, the tracker attached to the modem, tracker first: the frames are the restatement's.  (Payloads and order: the device's estimate
    differs from the restatement's in its last bits -- the float transform -- and with it the retuned steps and the metrics.)"""
    f0_modem, drift = (F0 - 1.0 * BAUD, 0.0) if case == "acquisition" else (F0, 1.5 * BAUD)
    iq, payloads = M.frames_signal(12, F0, drift)
    m = F4.HostFsk4(FSD, BAUD, f0_modem, SP, 1)
    t = FT.HostFsk4Track(FSD, *SEARCH)
    t.attach(m)
    eng = hd.Engine(n_streams=2)
    f, plain = F4.Fsk4(eng, max_push=8192), F4.Fsk4(eng, max_push=8192)
    tr = FT.Fsk4Track(eng, max_push=8192)
    for x in (f, plain):
        x.set_modem(0, BAUD, f0_modem, SP, 1)
    tr.set_stream(0, *SEARCH)
    tr.set_stream(1, *SEARCH)                                        # stream 1 has no modem: left alone
    tr.attach(f)
    for at in range(0, iq.size, 8000):
        part = iq[at:at + 8000]
        t.push(part); m.push(part)
        rows = np.stack([part, part])
        tr.push_host(rows); f.push_host(rows); plain.push_host(rows)
    want = [x["payload"] for x in m.take_frames()]
    got, untracked = [x["payload"] for x in f.take_frames(0)], [x["payload"] for x in plain.take_frames(0)]
    assert got == want and (want == payloads[2:] if case == "acquisition" else want == payloads)
    assert len(untracked) == 0 if case == "acquisition" else len([p for p in untracked if p in payloads]) <= 8
    assert tr.stats(0)["retunes"] == f.retune_stats(0)["retunes"] >= 1 and f.retune_stats(0)["late"] == 0
    assert abs(tr.stats(0)["retunes"] - t.stats()["retunes"]) <= 1                       # (an estimate on the deadband's edge may fall either way)
    assert tr.stats(1)["retunes"] == 0 and tr.stats(1)["valid_epochs"] == tr.stats(0)["valid_epochs"]
    assert np.abs(tr.debug_records(0)["f0_hz"] - t.records()["f0_hz"]).max() < 0.01 * BAUD
    eng.close()


# ---------------------------------------------------------------- errors

def test_errors(hd, F4, FT):
    eng = hd.Engine(n_streams=2)
    f, tr = F4.Fsk4(eng), FT.Fsk4Track(eng, max_push=5000)
    L = eng.L
    assert L.hd_fsk4_retune(f.h, 0, F0, SP, 0) == HD_ERR_INVALID                       # no modem
    f.set_modem(0, BAUD, F0, SP, 1)
    assert L.hd_fsk4_retune(f.h, 0, 8000.0, SP, 0) == HD_ERR_INVALID                   # tone 3 out of band
    assert L.hd_fsk4_retune(f.h, 2, F0, SP, 0) == HD_ERR_INVALID                       # no such stream
    assert L.hd_fsk4_retune(f.h, 0, F0 + 5.0, SP, 0) == 0 and f.retune_stats(0)["retunes"] == 1 and f.retune_stats(0)["late"] == 0
    assert L.hd_fsk4_track_set_stream(tr.h, 0, BAUD, 1.99 * BAUD, 3.0 * BAUD, -9000.0, 9000.0) == HD_ERR_UNSUPPORTED      # a spacing under 2 baud
    assert L.hd_fsk4_track_set_stream(tr.h, 0, BAUD, 2.0 * BAUD, 3.0 * BAUD, -1000.0, 1000.0) == HD_ERR_INVALID           # no comb fits
    assert L.hd_fsk4_track_set_stream(tr.h, 2, *SEARCH) == HD_ERR_INVALID
    tr.set_stream(0, *SEARCH)
    with pytest.raises(hd.HabdecError, match="max_push"):
        tr.push_host(np.zeros((2, 5001), np.complex64))
    assert tr.stats(0)["samples"] == 0
    with pytest.raises(hd.HabdecError):
        tr.estimate(0)                                                                   # no epoch has ended
    with pytest.raises(hd.HabdecError):
        FT.Fsk4Track(eng, decay_q8=257)
    other = hd.Engine(n_streams=1)
    assert L.hd_fsk4_track_attach(tr.h, F4.Fsk4(other).h) == HD_ERR_INVALID
    other.close()
    eng.close()
