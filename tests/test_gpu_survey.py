"""The wideband survey on the GPU (hd_survey_*, include/habdec_amd.h; kernels/survey.hip).

Model: float64 numpy -- the float window table, np.fft.fft per segment in complex128, the same segmentation (tests/test_survey_host.py: welch).

Gate per bin:   |P_gpu[i] - P_ref[i]| <= 2e-5 sqrt(P_ref[i] Ppk) + 1e-10 Ppk + 66 * 2^-24 P_ref[i]
Ppk is the largest single-segment bin power of the model, normalised by sum w^2 like the average.  Where it comes from: the project's spectrum gate
holds every bin of one transform within 1e-5 of that segment's peak AMPLITUDE, so a bin's power |X|^2 is off by at most 2 |X| 1e-5 Apk + (1e-5 Apk)^2;
averaged over the segments (mean |X| <= sqrt(mean |X|^2)) that is the first term and the second; the third is the float sums: a run adds up to 64
non-negative terms (each product, the sum of the two squares and every addition rounded once: 66 roundings of at most 2^-24 relative), and the double
sums over the runs add nothing visible.  Largest measured excess (error over bound) per case: NOTES.md."""
import ctypes as C

import numpy as np
import pytest

import test_survey_host as host
from habdec_amd import capi, synth

pytestmark = pytest.mark.gpu

N, HOP, CH = 4096, 2048, 65536
FS = 2.048e6


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def eng(hd):
    e = hd.Engine(n_streams=1, sampling_rate=FS, decimation=64)
    yield e
    e.close()


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.complex64).view(np.float32).copy()).cuda()


def noise_and_tone(n, seed, f=123456.7, amp=0.3, sigma=0.05):
    nz = synth._noise(n, seed)
    k = np.arange(n)
    return (amp * np.exp(2j * np.pi * f / FS * k) + sigma * (nz[0::2] + 1j * nz[1::2])).astype(np.complex64)


def excess(p_gpu, p_ref, ppk):
    """largest error over bound; 0 where both are 0"""
    bound = 2e-5 * np.sqrt(p_ref * ppk) + 1e-10 * ppk + 66 * 2.0 ** -24 * p_ref
    err = np.abs(p_gpu - p_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def survey_of(eng, pushes, how="device"):
    """power, segments of a fresh survey fed `pushes` (complex64 arrays)"""
    sv = eng.survey()
    keep = []
    for x in pushes:
        if how == "device":
            d = to_dev(x)
            keep.append(d)
            sv.push_device(d.data_ptr(), len(x))
        else:
            sv.push_host(x)
    out = sv.power()
    sv.close()
    return out


def check(eng, pushes, label):
    p_ref, segs, ppk = host.welch(pushes)
    p, k = survey_of(eng, pushes)
    assert k == segs, (label, k, segs)
    ex = excess(p, p_ref, ppk)
    print(f"{label}: {segs} segments, largest error over bound {ex:.4f}")
    assert ex <= 1.0, (label, ex)
    return p


# ---- 1. sizes
SIZES = {"4096_one_segment": (4096, None), "6144": (6144, None), "one_full_run": (N + 63 * HOP, 1), "second_run_of_one": (N + 64 * HOP, 1),
         "unused_tail": (N + 3 * HOP + 1777, None), "65536_31_waves": (CH, None)}


@pytest.mark.parametrize("name", list(SIZES))
def test_sizes(eng, monkeypatch, name):
    n, runs = SIZES[name]
    if runs:
        monkeypatch.setenv("HD_SURVEY_RUNS", str(runs))
    check(eng, [noise_and_tone(n, seed=n % 1000)], name)


def test_a_push_below_one_segment_adds_nothing(eng):
    sv = eng.survey()
    d = to_dev(noise_and_tone(4095, 1))
    sv.push_device(d.data_ptr(), 4095)
    sv.push_host(noise_and_tone(4095, 2))
    p, k = sv.power()
    assert k == 0 and not p.any()
    sv.close()


# ---- 2. basis inputs
@pytest.mark.parametrize("at", [0, 63, 64, 4095])
def test_unit_impulse(eng, at):
    x = np.zeros(N, np.complex64)
    x[at] = 1.0
    p = check(eng, [x], f"impulse at {at}")
    w = float(host.window()[at])
    assert np.allclose(p, w * w / np.sum(host.window().astype(np.float64) ** 2), rtol=1e-3, atol=0)     # flat: |w[at]|^2 in every bin (0 at sample 0)


@pytest.mark.parametrize("k", [0, 1, 63, 64, 2047, 2048, 4095])
def test_unit_exponential_on_a_bin_centre(eng, k):
    """The peak must sit at index (k + 2048) & 4095, its Hann neighbours a quarter of it: pins the lane / register / half-swap mapping."""
    x = np.exp(2j * np.pi * k * np.arange(N) / N).astype(np.complex64)
    p = check(eng, [x], f"exponential on bin {k}")
    i = (k + 2048) & 4095
    assert int(np.argmax(p)) == i, (k, int(np.argmax(p)), i)
    for j in ((i - 1) % N, (i + 1) % N):
        assert p[j] == pytest.approx(p[i] / 4, rel=1e-3)
    assert np.sort(p)[-4] < 1e-6 * p[i]


# ---- 3. several launches
def test_several_launches(eng, monkeypatch):
    """259 segments at HD_SURVEY_RUNS=2: r = 64, five runs, three launches, a last run of three segments."""
    monkeypatch.setenv("HD_SURVEY_RUNS", "2")
    check(eng, [noise_and_tone(N + 258 * HOP, seed=3)], "259 segments in three launches")


# ---- 4. accumulation over pushes, reset
def test_accumulation_over_pushes_and_reset(eng):
    sizes = [CH, 4096, 6144, 10000]
    x = noise_and_tone(sum(sizes), seed=4)
    pushes = np.split(x, np.cumsum(sizes)[:-1])
    p_ref, segs, ppk = host.welch(pushes)
    assert segs == 31 + 1 + 2 + 3
    sv = eng.survey()
    keep = [to_dev(q) for q in pushes]
    for d, q in zip(keep, pushes):
        sv.push_device(d.data_ptr(), len(q))
    p, k = sv.power()
    ex = excess(p, p_ref, ppk)
    print(f"four pushes: {k} segments, largest error over bound {ex:.4f}")
    assert k == segs and ex <= 1.0, (k, ex)
    sv.reset()
    p0, k0 = sv.power()
    assert k0 == 0 and not p0.any()
    sv.push_device(keep[0].data_ptr(), CH)                       # and the survey goes on from zero
    p1, k1 = sv.power()
    assert k1 == 31 and np.array_equal(p1, survey_of(eng, [pushes[0]])[0])
    sv.close()


def test_rows_are_added_in_run_order(eng):
    """Three segments, one run each (r = 1), the first 2^36 times stronger than the others: the double sums are no longer exact, so their order shows.
    Each run's float row is read back from a survey of that segment alone (power * sum w^2 rounds back to the float); the survey of the whole push must be,
    bit for bit, ((0 + row 0) + row 1) + row 2 over 3 sum w^2 -- the mutant that adds the rows in descending order differs in most bins."""
    x = noise_and_tone(N + 2 * HOP, seed=6)
    x[:HOP] *= np.float32(2.0 ** 18)
    sw2 = 0.0
    for v in host.window():
        sw2 += float(v) * float(v)                                   # in table order, as the engine sums it
    rows = []
    for s in range(3):
        p, k = survey_of(eng, [x[s * HOP:s * HOP + N]])
        assert k == 1
        rows.append((p * sw2).astype(np.float32).astype(np.float64))
        assert np.array_equal(rows[-1] / (1.0 * sw2), p)             # the float row is recovered exactly
    want = ((rows[0] + rows[1]) + rows[2]) / (3.0 * sw2)
    other = ((rows[2] + rows[1]) + rows[0]) / (3.0 * sw2)
    assert np.count_nonzero(want != other) > 100                     # the order is observable on this input
    p, k = survey_of(eng, [x])
    assert k == 3 and np.array_equal(p, want), int(np.count_nonzero(p != want))


# ---- 5. determinism
@pytest.mark.parametrize("runs", [None, 2], ids=["default", "RUNS=2"])
def test_same_pushes_same_bytes_from_device_and_host(eng, monkeypatch, runs):
    """(300 segments at the default run count: r = 1 and two staging slabs; 259 at HD_SURVEY_RUNS=2: r = 64, a slab of four runs and one of one)"""
    if runs:
        monkeypatch.setenv("HD_SURVEY_RUNS", str(runs))
    sizes = [N + (258 if runs else 299) * HOP + 5, CH, 6144]
    x = noise_and_tone(sum(sizes), seed=5)
    pushes = np.split(x, np.cumsum(sizes)[:-1])
    a, ka = survey_of(eng, pushes)
    b, kb = survey_of(eng, pushes)
    assert ka == kb == sum(host.segments_of(n) for n in sizes) and a.tobytes() == b.tobytes()
    c, kc = survey_of(eng, pushes, how="host")                    # pageable memory
    assert kc == ka and c.tobytes() == a.tobytes()
    pinned = []
    for q in pushes:
        buf = eng.pinned_array(len(q))
        buf[:] = q
        pinned.append(buf)
    d, kd = survey_of(eng, pinned, how="host")
    assert kd == ka and d.tobytes() == a.tobytes()


# ---- 6. the engine is left alone
def test_the_engine_is_left_alone(hd):
    """A pipeline = 1 engine, 64 streams, /64, six 65536-sample calls from device memory; with a survey push of the same buffer between every two calls the
    discriminator checksums and the characters of every stream are those of the run without a survey, on the same launch path."""
    import torch
    S, n_calls = 64, 6
    base = np.stack([synth.fsk_iq(synth.rtty_bits(synth.make_sentence(f"SV{s}", f"{s},1.5,2.5") * 3, 8, 2, 6 + 3 * s, 10), FS, 300, sigma=0.05, seed=80 + s,
                                  n_samples=n_calls * CH, f0=100.0 * s) for s in range(4)])
    dev = [to_dev(base[:, k * CH:(k + 1) * CH]).reshape(4, 2 * CH).repeat(S // 4, 1).contiguous() for k in range(n_calls)]
    torch.cuda.synchronize()
    results = []
    for with_survey in (False, True):
        e = hd.Engine(n_streams=S, sampling_rate=FS, decimation=64, pipeline=1)
        sv = e.survey() if with_survey else None
        paths = []
        for k in range(n_calls):
            e.process_device(dev[k].data_ptr(), CH, CH)
            paths.append(e.timing()["path"])
            if sv and k + 1 < n_calls:
                sv.push_device(dev[k].data_ptr(), S * CH)
        e.flush()
        if sv:
            p, segs = sv.power()
            assert segs == (n_calls - 1) * host.segments_of(S * CH) and np.all(p > 0)
        results.append((paths, [e.demod_checksum_total(s) for s in range(S)], [e.take_chars(s) for s in range(S)]))
        e.close()
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert results[0][1] == results[1][1] and all(c[0] == n_calls for c in results[0][1])
    assert results[0][2] == results[1][2]


# ---- 7. what it is for
FAN = dict(fs=2.048e6, n_calls=56, offsets=[-600e3, 250e3, 5e3], calls=["WIDEA", "WIDEB", "WIDEC"], noise=0.05)


def fan_recording():
    fs, n = FAN["fs"], FAN["n_calls"] * CH
    texts = ["".join(synth.make_sentence(c, str(i)) for i in range(3)) for c in FAN["calls"]]
    rec = np.zeros(n, np.complex128)
    for j, (f, t) in enumerate(zip(FAN["offsets"], texts)):
        rec += synth.fsk_iq(synth.rtty_bits(t, 8, 2, 6 + 3 * j, 10), fs, 300, sigma=0.0, seed=j, n_samples=n, f0=f)
    nz = synth._noise(n, 7)
    return (rec + FAN["noise"] * (nz[0::2] + 1j * nz[1::2])).astype(np.complex64), texts


def test_survey_then_front_tune_decodes_three_payloads(hd):
    """One 2.048 MS/s recording with payloads at -600 kHz, +250 kHz and +5 kHz that nobody tells the engine about: the survey of its 56 pushes finds exactly
    three candidates, each within 250 + 500 Hz (half the shift, one bin) of a payload; streams front-tuned to the candidates decode the first two
    sentences of their own callsign and nothing else, the untuned stream nothing."""
    fs, n_calls = FAN["fs"], FAN["n_calls"]
    rec, texts = fan_recording()
    dev = to_dev(rec)
    eng = hd.Engine(n_streams=4, sampling_rate=fs, decimation=64)
    sv = eng.survey()
    for k in range(n_calls):
        sv.push_device(dev.data_ptr() + k * CH * 8, CH)
    cands = sv.detect()
    assert sv.power()[1] == n_calls * 31
    assert len(cands) == 3, cands
    cands.sort(key=lambda c: c["offset_hz"])
    for c, f in zip(cands, sorted(FAN["offsets"])):
        print(f"payload at {f:10.1f} Hz: surveyed {c['offset_hz']:10.1f} Hz, snr {c['snr_db']:.1f} dB, width {c['width_hz']:.0f} Hz")
        assert abs(c["offset_hz"] - f) <= 250 + 500, (c, f)
    for s, c in enumerate(cands):
        eng.set_front_tune(s, c["offset_hz"])
    for k in range(n_calls):
        eng.process_device(dev.data_ptr() + k * CH * 8, 0, CH)
    got = [eng.take_sentences(s) for s in range(4)]
    order = np.argsort(FAN["offsets"])                              # streams 0-2 took the candidates in ascending frequency
    for s in range(3):
        want = [t.strip().lstrip("$") for t in texts[order[s]].split("\n") if t][:2]
        assert got[s] == want, (s, got[s], want)
    assert got[3] == []
    eng.close()


# ---- 8. errors: all host-side checks, nothing reaches a kernel
def test_errors(eng):
    L = eng.L
    d = to_dev(noise_and_tone(CH, 8))
    sv = eng.survey()
    h = C.c_void_p()
    assert L.hd_survey_create(None, C.byref(h)) == -1 and L.hd_survey_create(eng.h, None) == -1
    assert L.hd_survey_push_device(None, d.data_ptr(), CH) == -1 and L.hd_survey_push_host(None, d.data_ptr(), CH) == -1
    assert L.hd_survey_push_device(sv.h, None, CH) == -1 and L.hd_survey_push_host(sv.h, None, CH) == -1
    assert L.hd_survey_push_device(sv.h, d.data_ptr() + 4, CH - 1) == -1 and b"8-byte" in L.hd_last_error()
    pageable = noise_and_tone(CH, 9)
    assert L.hd_survey_push_device(sv.h, pageable.ctypes.data, CH) == -1              # host memory HIP does not know: refused, not launched
    assert L.hd_survey_reset(None) == -1
    p = np.zeros(N)
    seg = C.c_uint64(7)
    assert L.hd_survey_power(None, p.ctypes.data, N, C.byref(seg)) == -1 and L.hd_survey_power(sv.h, None, N, C.byref(seg)) == -1
    assert sv.power()[1] == 0                                                          # nothing above was counted
    sv.push_device(d.data_ptr() + 8, 6144)                                             # 8-byte aligned is enough; two segments
    assert L.hd_survey_power(sv.h, p.ctypes.data, N - 1, C.byref(seg)) == 0 and seg.value == 2 and not p.any()
    par = capi.hd_survey_params()
    L.hd_survey_params_default(C.byref(par))
    out, n = (capi.hd_survey_candidate * 4)(), C.c_uint32(9)
    assert L.hd_survey_detect(sv.h, C.byref(par), out, 4, C.byref(n)) == -3 and n.value == 0      # fewer than 16 segments
    with pytest.raises(Exception, match="error -3"):
        sv.detect()
    assert L.hd_survey_detect(None, C.byref(par), out, 4, C.byref(n)) == -1
    assert L.hd_survey_detect(sv.h, None, out, 4, C.byref(n)) == -1 and L.hd_survey_detect(sv.h, C.byref(par), out, 4, None) == -1
    sv.push_device(d.data_ptr(), CH)
    assert L.hd_survey_detect(sv.h, C.byref(par), out, 4, C.byref(n)) == 0 and n.value == 1 and abs(out[0].offset_hz - 123456.7) <= 500
    par.threshold_db = -1.0
    assert L.hd_survey_detect(sv.h, C.byref(par), out, 4, C.byref(n)) == -1
    sv.close()
    L.hd_survey_destroy(None)
