"""The tone search on the host: the spectrum's restatement (hd_host_tone_search_*) and the detector (hd_host_tone_search_detect) against the numpy model
of their definition (tests/tone_search_model.py), the detector's accuracy on weak signals, what it must refuse, and the noise ladder's last rung with
tones nobody told it.  No GPU.

Figures of the build this was written with (NOTES.md, "Tone search"):
  worst tone error per signal of ACCURACY over seeds 3 and 4, in Hz: 1.1, 1.0, 8.1, 8.8, 1.0, 4.3 (limits baud / 12: 4.2, 4.2, 25, 25, 4.2, 8.3)
  noise alone: quality * sqrt(w * segments) at most 6.2, the threshold is 10; a lone carrier: quality 0.058
  ladder at sigma 1.0: found tones within 7.0 Hz of +-250 on all 8 streams; sentences plain / with repair 25 / 39 with the true tones, 24 / 37 with the found"""
import ctypes as C

import numpy as np
import pytest

import tone_search_model as SM
import tones_model as TM
from habdec_amd import capi

HD_ERR_INVALID, HD_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def hd():
    from habdec_amd.build import build
    build()
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


def host_spectrum(hd, x, cut=None):
    """power, segments of the host restatement fed x in pushes of `cut` samples (None: one push)."""
    h = hd.HostToneSearch()
    for at in range(0, len(x), cut or max(len(x), 1)):
        h.push(x[at:at + (cut or len(x))])
    return h.power()


@pytest.fixture(scope="module")
def spectra(hd):
    """{(case name, seed): (case, power, segments)} of the ACCURACY signals through the host restatement: computed once."""
    out = {}
    for case in SM.ACCURACY:
        for seed in SM.SEEDS:
            p, k = host_spectrum(hd, SM.signal(case, seed), 4000)
            out[(case[0], seed)] = (case, p, k)
    return out


# ---------------------------------------------------------------- the spectrum

def test_host_spectrum_against_the_model(hd):
    case = SM.ACCURACY[2]
    x = SM.signal(case, 3)[:SM.N + 9 * SM.HOP + 777]
    want, segs, _, carry = SM.spectrum(x)
    assert segs == 10 and carry == 777 + SM.HOP
    for cut in (None, 1, 63, 2047, 2048, 2049, 4095, 4097):
        p, k = host_spectrum(hd, x, cut)
        err = float(np.max(np.abs(p - want)) / np.max(want))
        assert k == segs and err <= 1e-9, (cut, k, err)
    first = host_spectrum(hd, x)[0]
    assert all(host_spectrum(hd, x, cut)[0].tobytes() == first.tobytes() for cut in (1, 2049))        # however the stream is cut
    p, k = host_spectrum(hd, x[:4095])
    assert k == 0 and not p.any()
    h = hd.HostToneSearch()
    h.push(x[:5000])
    h.reset()
    h.push(x)
    assert h.power()[0].tobytes() == first.tobytes()
    bad = x.copy()
    bad[5000] = np.nan
    p, k = host_spectrum(hd, bad)
    assert k == segs and not np.isfinite(p).any()


# ---------------------------------------------------------------- the detector against the model

def same(got, want, what):
    assert isinstance(want, dict), (what, want)
    for k in ("w", "bin_lo", "shift_bins", "valid", "segments"):
        assert got[k] == want[k], (what, k, got, want)
    assert abs(got["f_hi_hz"] - want["f_hi_hz"]) <= 1e-6 and abs(got["f_lo_hz"] - want["f_lo_hz"]) <= 1e-6, (what, got, want)
    assert abs(got["quality"] - want["quality"]) <= 1e-9 and abs(got["floor"] - want["floor"]) <= 1e-9 * max(want["floor"], 1.0), (what, got, want)


def test_detector_against_the_model_on_the_signals(hd, spectra):
    for (name, seed), (case, p, k) in spectra.items():
        fsd, baud, lo, hi = case[4], case[1], case[8], case[9]
        same(hd.tone_search_detect(p, k, fsd, baud=baud, shift_lo_hz=lo, shift_hi_hz=hi), SM.detect(p, k, fsd, baud, lo, hi), (name, seed))


def test_detector_against_the_model_on_edge_inputs(hd):
    fsd = 8000.0
    inputs = {}
    inputs["noise"] = (host_spectrum(hd, SM.noise(SM.N + 15 * SM.HOP, 1.0, 21)), 300.0, {})
    inputs["carrier"] = (host_spectrum(hd, SM.carrier(fsd, 250.0, 0.35, 6.0, 22)), 300.0, {})
    inputs["zeros"] = ((np.zeros(SM.N), 16), 300.0, {})
    nan = np.ones(SM.N)
    nan[1234] = np.nan
    inputs["nan"] = ((nan, 16), 300.0, {})
    inf = np.ones(SM.N)
    inf[7] = np.inf
    inputs["inf"] = ((inf, 16), 300.0, {})
    # a pair whose refinement windows touch both edges of the array: r = 77 bins at 500 baud, the tones 40 bins inside either end
    edge = np.ones(SM.N)
    edge[30:51] += 50.0
    edge[SM.N - 51:SM.N - 30] += 60.0
    inputs["edges"] = ((edge, 16), 500.0, dict(shift_lo_hz=7000.0, shift_hi_hz=7990.0))
    flat = np.ones(SM.N)
    inputs["flat"] = ((flat, 16), 50.0, {})                             # every score 0: the first pair wins, the centroids stay
    for name, ((p, k), baud, kw) in inputs.items():
        got, want = hd.tone_search_detect(p, k, fsd, baud=baud, **kw), SM.detect(p, k, fsd, baud, **kw)
        same(got, want, name)
        if name in ("zeros", "nan", "inf", "noise", "carrier", "flat"):
            assert got["valid"] == 0, (name, got)
        if name == "zeros":
            assert got["floor"] == 0 and got["quality"] == 0
        if name in ("nan", "inf"):
            assert (got["bin_lo"], got["shift_bins"], got["f_hi_hz"], got["f_lo_hz"], got["quality"]) == (0, 0, 0.0, 0.0, 0.0) and got["w"] == 77
        if name == "edges":
            r = int(np.rint(0.3 * 500.0 / (fsd / SM.N)))
            c_lo, c_hi = (int(np.rint(got[k] / (fsd / SM.N))) + SM.N // 2 for k in ("f_lo_hz", "f_hi_hz"))
            assert got["valid"] == 1 and c_lo - r < 0 and c_hi + r > SM.N - 1, (got, r)                  # the later rounds' windows are clamped at either end
            assert abs(got["f_lo_hz"] - (40 - 2048) * fsd / SM.N) < 20 and abs(got["f_hi_hz"] - (SM.N - 41 - 2048) * fsd / SM.N) < 20, got


def test_detector_errors(hd):
    L = hd.lib()
    p = np.ones(SM.N)
    r = capi.hd_tone_search_result()

    def rc(segments=16, fsd=8000.0, power=p, out=r, **kw):
        par = capi.hd_tone_search_detect_params()
        L.hd_tone_search_detect_params_default(C.byref(par))
        for k, v in kw.items():
            setattr(par, k, v)
        code = L.hd_host_tone_search_detect(None if power is None else power.ctypes.data, segments, fsd, C.byref(par), None if out is None else C.byref(out))
        want = SM.detect(p, segments, fsd, par.baud, par.shift_lo_hz, par.shift_hi_hz, par.min_quality) if power is not None and out is not None else HD_ERR_INVALID
        assert code == (want if isinstance(want, int) else 0), (segments, fsd, kw, code, want)
        return code
    par = capi.hd_tone_search_detect_params()
    L.hd_tone_search_detect_params_default(C.byref(par))
    assert (par.baud, par.shift_lo_hz, par.shift_hi_hz, par.min_quality) == (0.0, 170.0, 1000.0, 0.5)
    assert rc(baud=300.0) == 0
    assert rc(baud=300.0, segments=8) == 0 and rc(baud=300.0, segments=7) == HD_ERR_UNSUPPORTED         # fewer than 8 segments
    assert rc() == HD_ERR_INVALID and rc(baud=-1.0) == HD_ERR_INVALID and rc(baud=float("nan")) == HD_ERR_INVALID      # baud <= 0
    assert rc(baud=0.0, segments=7) == HD_ERR_INVALID
    assert rc(baud=300.0, shift_hi_hz=160.0) == HD_ERR_INVALID                                          # no d between the two
    assert rc(baud=300.0, shift_lo_hz=7900.0, shift_hi_hz=9000.0) == HD_ERR_INVALID                     # no d that fits beside two windows of 77 bins
    assert rc(baud=300.0, shift_lo_hz=7800.0, shift_hi_hz=9000.0) == 0
    assert rc(baud=300.0, shift_lo_hz=0.0) == HD_ERR_INVALID and rc(baud=300.0, min_quality=-0.1) == HD_ERR_INVALID
    assert rc(baud=300.0, fsd=0.0) == HD_ERR_INVALID and rc(baud=20000.0) == HD_ERR_INVALID             # w >= 4096
    assert rc(baud=300.0, power=None) == HD_ERR_INVALID and rc(baud=300.0, out=None) == HD_ERR_INVALID
    assert L.hd_host_tone_search_detect(p.ctypes.data, 16, 8000.0, None, C.byref(r)) == HD_ERR_INVALID
    seg = C.c_uint64(0)
    h = hd.HostToneSearch()
    assert L.hd_host_tone_search_power(None, p.ctypes.data, SM.N, C.byref(seg)) == HD_ERR_INVALID
    assert L.hd_host_tone_search_power(h.h, None, SM.N, C.byref(seg)) == HD_ERR_INVALID
    assert L.hd_host_tone_search_power(h.h, p.ctypes.data, SM.N - 1, C.byref(seg)) == 0 and p.all()


# ---------------------------------------------------------------- accuracy

def test_tones_of_weak_signals_within_a_twelfth_of_the_baud_rate(hd, spectra):
    """Each found tone within baud / 12 of the truth and every signal valid: the project's own tolerance -- both tones 25 Hz off at 300 baud cost 3 of 55
    sentences on the sigma 0.85 ladder (NOTES.md, "Tone filters")."""
    worst = {}
    for (name, seed), (case, p, k) in spectra.items():
        baud, fsd, f0, lo, hi = case[1], case[4], case[7], case[8], case[9]
        got = hd.tone_search_detect(p, k, fsd, baud=baud, shift_lo_hz=lo, shift_hi_hz=hi)
        err = max(abs(got["f_hi_hz"] - (f0 + SM.SHIFT / 2)), abs(got["f_lo_hz"] - (f0 - SM.SHIFT / 2)))
        thr = max(0.5, 10.0 / np.sqrt(got["w"] * k))
        print(f"tone search accuracy: {name} seed {seed}: {k} segments, tones {got['f_lo_hz']:.1f} {got['f_hi_hz']:.1f}, error {err:.2f} Hz of {baud / 12:.1f}, "
              f"quality {got['quality']:.2f} = {got['quality'] / thr:.1f} thresholds")
        worst[name] = max(worst.get(name, 0.0), err)
        assert got["valid"] == 1 and err <= baud / 12, (name, seed, got, err)
    print("tone search accuracy, worst error per signal (Hz):", {k: round(v, 2) for k, v in worst.items()})


# ---------------------------------------------------------------- not valid

@pytest.mark.parametrize("fsd,baud,w", [(8000.0, 300.0, 77), (39062.5, 50.0, 3)], ids=["8k_300", "39k_50"])
def test_noise_alone_is_not_valid(hd, fsd, baud, w):
    worst = 0.0
    for seed in range(31, 37):
        x = SM.noise(SM.N + 44 * SM.HOP, 1.0, seed)
        h, at = hd.HostToneSearch(), 0
        for k in (8, 16, 45):
            end = SM.N + (k - 1) * SM.HOP
            h.push(x[at:end])
            at = end
            got = h.detect(fsd, baud=baud)
            assert got["segments"] == k and got["w"] == w and got["valid"] == 0, (seed, k, got)
            worst = max(worst, got["quality"] * np.sqrt(w * k))
    print(f"tone search, noise alone at fsd {fsd} baud {baud}: quality * sqrt(w * segments) at most {worst:.2f} (threshold 10)")


def test_a_lone_carrier_is_not_valid(hd):
    p, k = host_spectrum(hd, SM.carrier(8000.0, 250.0, 0.35, 12.0, 41))
    got = hd.tone_search_detect(p, k, 8000.0, baud=300.0)
    print("tone search, a lone carrier at +250 Hz, sigma 0.35:", k, "segments, quality %.3f" % got["quality"])
    assert k == 45 and got["valid"] == 0, got


# ---------------------------------------------------------------- the ladder's last rung: sigma 1.0, tones nobody told

def test_ladder_last_rung_with_found_tones(hd):
    """tones_model.weak_iq(1.0) through the oracle as test_tones_host.py::ladder_counts takes it: its decimated IQ through the host tone search, the found
    tones into the host tone filters, their row into the host clocked decoder -- against the same chain with the true tones +-250 Hz."""
    iq, sent = TM.weak_iq(1.0)
    fsd = TM.WEAK["fs"] / TM.WEAK["D"]
    counts = dict(true=0, true_repaired=0, found=0, found_repaired=0, false=0)
    worst = 0.0
    for s, (_, decim, _) in enumerate(TM.weak_oracle(iq)):
        h = hd.HostToneSearch()
        for d in decim:
            h.push(d)
        got = h.detect(fsd, baud=TM.WEAK["baud"])
        err = max(abs(got["f_hi_hz"] - TM.SHIFT / 2), abs(got["f_lo_hz"] + TM.SHIFT / 2))
        worst = max(worst, err)
        assert got["valid"] == 1 and err <= 25.0, (s, got)
        for key, (f_hi, f_lo) in (("true", (TM.SHIFT / 2, -TM.SHIFT / 2)), ("found", (got["f_hi_hz"], got["f_lo_hz"]))):
            t = hd.HostTones(fsd, TM.WEAK["baud"], f_hi, f_lo)
            rows = [t.push(d) for d in decim]
            for suffix, kw in (("", dict(repair_bits=0)), ("_repaired", dict())):
                c = hd.HostClocked(fsd, TM.WEAK["baud"], TM.WEAK["bits"], TM.WEAK["stops"], **kw)
                for r in rows:
                    c.push(r)
                texts = [x for (_, _, x) in c.take_sentences(256)]
                counts[key + suffix] += len(texts)
                counts["false"] += len([x for x in texts if x not in sent[s]])
    print("tone search ladder at sigma 1.0: worst tone error %.1f Hz; sentences plain / with repair: true tones" % worst, counts["true"], "/", counts["true_repaired"],
          "found tones", counts["found"], "/", counts["found_repaired"], "not sent", counts["false"])
    assert counts["false"] == 0, counts                               # nothing delivered that was not sent
    assert counts["found"] >= counts["true"] - 3 and counts["found_repaired"] >= counts["true_repaired"] - 3, counts
