"""Host side of the wideband survey (include/habdec_amd_host.h: hd_host_survey_window, hd_host_survey_detect) -- no GPU.

The detector is compared with a plain-Python restatement of its six steps on hand-made spectra, then run on float64 numpy Welch spectra (the model the
GPU tests compare the kernel with: `welch` below) of noise alone and of one capture with five payloads."""
import ctypes as C
import math

import numpy as np
import pytest

from habdec_amd import capi, synth

N, HOP = 4096, 2048
FS = 2.048e6
BINW = FS / N


@pytest.fixture(scope="module")
def L():
    from habdec_amd.build import build
    build()
    return capi.lib()


# ---- the model: window, segmentation, Welch average (float64; also what tests/test_gpu_survey.py holds the kernel against)
def window():
    return np.float32(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))


def segments_of(n):
    return 0 if n < N else 1 + (n - N) // HOP


def periodograms(x, w=None):
    """|FFT|^2 of every whole segment of ONE push, fftshifted, [n_seg, 4096] float64 (not normalised)."""
    w = window().astype(np.float64) if w is None else w
    x = np.asarray(x).astype(np.complex128)
    k = segments_of(len(x))
    if not k:
        return np.zeros((0, N))
    seg = np.lib.stride_tricks.sliding_window_view(x, N)[::HOP][:k]
    return np.abs(np.fft.fftshift(np.fft.fft(seg * w, axis=1), axes=1)) ** 2


def welch(pushes):
    """(power[4096], segments, Ppk): the survey of these pushes; Ppk = the largest single-segment bin power, normalised by sum w^2 like the average."""
    sw2 = float(np.sum(window().astype(np.float64) ** 2))
    acc, k, pk = np.zeros(N), 0, 0.0
    for x in pushes:
        p = periodograms(x)
        if len(p):
            acc += p.sum(axis=0); k += len(p); pk = max(pk, float(p.max()))
    return (acc / (k * sw2) if k else acc), k, pk / sw2


# ---- the detector, restated
def model_detect(power, segments, fs, threshold_db=6.0, merge_hz=1500.0, dc_guard_hz=0.0, max_width_hz=0.0):
    if segments < 16:
        return -3
    if any(not (p >= 0.0) for p in power) or not threshold_db >= 0 or not merge_hz >= 0 or not dc_guard_hz >= 0 or not max_width_hz >= 0:
        return -1
    binw = fs / N
    f = [(i - N // 2) * binw for i in range(N)]
    elig = [i for i in range(N) if dc_guard_hz == 0 or abs(f[i]) >= dc_guard_hz]
    srt = sorted(power[i] for i in elig)
    floor = srt[len(srt) // 2] if len(srt) % 2 else 0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2])
    level = floor * max(10.0 ** (threshold_db / 10.0), 1.0 + 8.0 / math.sqrt(segments))
    marked = [i for i in elig if power[i] >= level]
    g = math.ceil(merge_hz / binw)
    clusters = []
    for i in marked:
        if clusters and i - clusters[-1][-1] - 1 <= g:
            clusters[-1].append(i)
        else:
            clusters.append([i])
    out = []
    for c in clusters:
        sw = sum(power[i] - floor for i in c)
        width = (c[-1] - c[0] + 1) * binw
        if max_width_hz > 0 and width > max_width_hz:
            continue
        out.append(dict(offset_hz=sum(f[i] * (power[i] - floor) for i in c) / sw, snr_db=10.0 * math.log10(sw / floor), width_hz=width, bin_lo=c[0], bin_hi=c[-1]))
    out.sort(key=lambda d: (-d["snr_db"], d["offset_hz"]))
    return out


def c_detect(L, power, segments, fs=FS, cap=64, **params):
    p = capi.hd_survey_params()
    L.hd_survey_params_default(C.byref(p))
    for k, v in params.items():
        setattr(p, k, v)
    out, found = (capi.hd_survey_candidate * max(cap, 1))(), C.c_uint32(77)
    rc = L.hd_host_survey_detect(np.ascontiguousarray(power, np.float64), segments, fs, C.byref(p), out, cap, C.byref(found))
    if rc:
        assert found.value == 0
        return rc
    return found.value, [dict(offset_hz=c.offset_hz, snr_db=c.snr_db, width_hz=c.width_hz, bin_lo=c.bin_lo, bin_hi=c.bin_hi) for c in out[:min(cap, found.value)]]


def same(got, want):
    assert len(got) == len(want), (got, want)
    for a, b in zip(got, want):
        assert (a["bin_lo"], a["bin_hi"]) == (b["bin_lo"], b["bin_hi"]), (a, b)
        assert a["width_hz"] == b["width_hz"]
        assert a["offset_hz"] == pytest.approx(b["offset_hz"], rel=1e-12, abs=1e-9) and a["snr_db"] == pytest.approx(b["snr_db"], rel=1e-12, abs=1e-12), (a, b)


def spectrum(bins):
    p = np.ones(N)
    for i, v in bins.items():
        p[i] = v
    return p


def test_defaults_and_window(L):
    p = capi.hd_survey_params()
    L.hd_survey_params_default(C.byref(p))
    assert (p.threshold_db, p.merge_hz, p.dc_guard_hz, p.max_width_hz) == (6.0, 1500.0, 0.0, 0.0)
    w = np.zeros(N, np.float32)
    L.hd_host_survey_window(w)
    assert np.array_equal(w.view(np.uint32), window().view(np.uint32))
    assert w[0] == 0.0 and w[N // 2] == 1.0


# gap g = ceil(1500 / 500) = 3 unmarked bins at the default merge_hz and 2.048 MS/s
CASES = {
    "nothing_marked": (spectrum({}), {}, 0),
    "below_threshold": (spectrum({700: 3.9}), {}, 0),
    "one_bin": (spectrum({1000: 10.0}), {}, 1),
    "gap_exactly_g": (spectrum({100: 10.0, 101: 7.0, 105: 20.0}), {}, 1),
    "gap_g_plus_1": (spectrum({100: 10.0, 101: 7.0, 106: 20.0}), {}, 2),
    "merge_hz_0_adjacent_only": (spectrum({100: 10.0, 101: 7.0, 103: 20.0}), dict(merge_hz=0.0), 2),
    "edges_do_not_wrap": (spectrum({0: 10.0, 1: 5.0, 4094: 8.0, 4095: 30.0}), {}, 2),
    "dc_guard": (spectrum({2046: 9.0, 2047: 50.0, 2048: 900.0, 2049: 50.0, 3000: 12.0}), dict(dc_guard_hz=1000.0), 2),
    "no_dc_guard": (spectrum({2046: 9.0, 2047: 50.0, 2048: 900.0, 2049: 50.0, 3000: 12.0}), {}, 2),
    "max_width": (spectrum({**{i: 10.0 for i in range(500, 510)}, 900: 6.0, 901: 6.0}), dict(max_width_hz=3000.0), 1),
    "max_width_exact_fit": (spectrum({i: 10.0 for i in range(500, 506)}), dict(max_width_hz=3000.0), 1),
    "tie_in_snr": (spectrum({3000: 10.0, 1000: 10.0, 2000: 10.0, 50: 11.0}), {}, 4),
    "threshold_0_is_the_noise_term": (spectrum({10: 1.99, 20: 2.0, 30: 2.01}), dict(threshold_db=0.0), 2),     # 64 segments: 1 + 8 / 8 = 2
}


@pytest.mark.parametrize("name", list(CASES))
def test_detector_against_its_restatement(L, name):
    power, params, n = CASES[name]
    want = model_detect(list(power), 64, FS, **params)
    found, got = c_detect(L, power, 64, **params)
    assert found == n == len(want), (found, n, want)
    same(got, want)
    if name == "one_bin":
        assert got[0] == dict(offset_hz=(1000 - 2048) * BINW, snr_db=pytest.approx(10 * math.log10(9.0)), width_hz=BINW, bin_lo=1000, bin_hi=1000)
    if name == "gap_exactly_g":
        assert (got[0]["bin_lo"], got[0]["bin_hi"]) == (100, 105)
        assert got[0]["offset_hz"] == pytest.approx(((100 - 2048) * 9 + (101 - 2048) * 6 + (105 - 2048) * 19) * BINW / 34)
    if name == "edges_do_not_wrap":
        assert [(c["bin_lo"], c["bin_hi"]) for c in got] == [(4094, 4095), (0, 1)]
    if name == "dc_guard":
        assert [(c["bin_lo"], c["bin_hi"]) for c in got] == [(3000, 3000), (2046, 2046)]       # |f| = 1000 Hz is outside the guard
    if name == "no_dc_guard":
        assert (got[0]["bin_lo"], got[0]["bin_hi"]) == (2046, 2049)
    if name == "max_width":
        assert (got[0]["bin_lo"], got[0]["bin_hi"]) == (900, 901)
    if name == "tie_in_snr":
        assert [c["bin_lo"] for c in got] == [50, 1000, 2000, 3000]


def test_cap_smaller_than_found(L):
    power = spectrum({100: 10.0, 1000: 30.0, 2000: 20.0})
    found, got = c_detect(L, power, 64, cap=1)
    assert found == 3 and [c["bin_lo"] for c in got] == [1000]
    found, got = c_detect(L, power, 64, cap=2)
    assert found == 3 and [c["bin_lo"] for c in got] == [1000, 2000]
    p = capi.hd_survey_params()
    L.hd_survey_params_default(C.byref(p))
    n = C.c_uint32(0)
    assert L.hd_host_survey_detect(power, 64, FS, C.byref(p), None, 0, C.byref(n)) == 0 and n.value == 3     # cap 0: count only


def test_errors_of_step_1(L):
    ok = spectrum({100: 10.0})
    assert c_detect(L, ok, 15) == -3 and model_detect(list(ok), 15, FS) == -3
    assert c_detect(L, ok, 16)[0] == 1
    for bad in (float("nan"), -1e-300, -1.0):
        p = ok.copy(); p[4000] = bad
        assert c_detect(L, p, 64) == -1 and model_detect(list(p), 64, FS) == -1, bad
    for params in (dict(threshold_db=-0.1), dict(merge_hz=-1.0), dict(dc_guard_hz=-1.0), dict(max_width_hz=-1.0), dict(threshold_db=float("nan"))):
        assert c_detect(L, ok, 64, **params) == -1 and model_detect(list(ok), 64, FS, **params) == -1, params
    par = capi.hd_survey_params()
    L.hd_survey_params_default(C.byref(par))
    out, n = (capi.hd_survey_candidate * 4)(), C.c_uint32(0)
    assert L.hd_host_survey_detect(ok, 64, FS, None, out, 4, C.byref(n)) == -1
    assert L.hd_host_survey_detect(ok, 64, FS, C.byref(par), None, 4, C.byref(n)) == -1
    assert L.hd_host_survey_detect(ok, 64, FS, C.byref(par), out, 4, None) == -1
    assert L.hd_host_survey_detect(ok, 64, 0.0, C.byref(par), out, 4, C.byref(n)) == -1
    assert c_detect(L, ok, 64, dc_guard_hz=2e6) == -1              # the guard leaves no bin
    assert c_detect(L, np.zeros(N), 64) == -3                       # no floor to hold a threshold against


# ---- noise alone: 1 + 8 / sqrt(K) is where it ends
NOISE_K = (16, 64, 255)


@pytest.mark.parametrize("seed", range(20))
def test_noise_alone_gives_no_candidate(L, seed):
    nz = synth._noise(N + (max(NOISE_K) - 1) * HOP, seed)
    x = 0.05 * (nz[0::2] + 1j * nz[1::2])
    for k in NOISE_K:
        power, segs, _ = welch([x[:N + (k - 1) * HOP]])
        assert segs == k
        found, got = c_detect(L, power, segs, threshold_db=0.0)
        assert found == 0, (seed, k, got, float(np.max(power) / np.median(power) - 1) * math.sqrt(k))
        assert np.median(power) == pytest.approx(2 * 0.05 ** 2, rel=0.05)       # white noise of complex variance s^2 reads about s^2


# ---- five payloads in one capture
FIVE = dict(fs=FS, n_push=8, push=65536, noise=0.05, seed=7,
            payloads=[(-600e3, 0.5, 500.0, 50), (250e3, 0.05, 425.0, 300), (5e3, 0.02, 850.0, 50), (1011.7e3, 0.01, 1000.0, 300), (-1023e3, 0.2, 170.0, 50)])


def five_capture():
    fs, n = FIVE["fs"], FIVE["n_push"] * FIVE["push"]
    rec = np.zeros(n, np.complex128)
    for j, (f0, amp, shift, baud) in enumerate(FIVE["payloads"]):
        bits = synth.rtty_bits(synth.make_sentence(f"FIVE{j}", f"{j},52.1,21.4") * 2, 8, 2, 2, 10)
        rec += synth.fsk_iq(bits, fs, baud, shift=shift, f0=f0, amp=amp, sigma=0.0, n_samples=n)
    nz = synth._noise(n, FIVE["seed"])
    return (rec + FIVE["noise"] * (nz[0::2] + 1j * nz[1::2])).astype(np.complex64)


def test_five_payloads_in_one_capture(L):
    rec = five_capture()
    power, segs, _ = welch(np.split(rec, FIVE["n_push"]))
    assert segs == FIVE["n_push"] * 31
    found, got = c_detect(L, power, segs)
    same(got, model_detect(list(power), segs, FS))
    assert found == 5, got
    got.sort(key=lambda c: c["offset_hz"])
    for c, (f0, amp, shift, baud) in zip(got, sorted(FIVE["payloads"])):
        err = abs(c["offset_hz"] - f0)
        print(f"carrier {f0:12.1f} Hz: surveyed {c['offset_hz']:12.1f} Hz, off by {err:6.1f} Hz, snr {c['snr_db']:5.1f} dB, width {c['width_hz']:.0f} Hz")
        assert err <= shift / 2 + FS / N, (c, f0)        # a centroid lies between the two tones, give or take the window's lobe
