"""The tone search on the GPU (hd_tone_search_*, include/habdec_amd.h; kernels/tone_search.hip).

Model: float64 numpy (tests/tone_search_model.py) -- the float window table with one rounded float product per part, np.fft.fft per segment of the
STREAM, the accumulation in segment order.

Gate per bin, the survey's (tests/test_gpu_survey.py has where it comes from):
    |P_gpu[i] - P_ref[i]| <= 2e-5 sqrt(P_ref[i] Ppk) + 1e-10 Ppk + 66 * 2^-24 P_ref[i]
The accumulation here is the survey's run length 1 -- every segment's float row goes into the double sums by itself -- so the third term, which allows
for 64 float additions, holds a fortiori.  Largest measured excess (error over bound) per case: NOTES.md.

That the stream may be cut anywhere is checked byte for byte: no float sum crosses a segment, so the accumulators are a function of the samples alone."""
import ctypes as C

import numpy as np
import pytest

import tone_search_model as SM
import tones_model as TM
from habdec_amd import capi, synth

pytestmark = pytest.mark.gpu
N, HOP = SM.N, SM.HOP
LEN = N + 5 * HOP + 777
HD_ERR_INVALID, HD_ERR_UNSUPPORTED, HD_ERR_CAPACITY = -1, -3, -4


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def eng(hd):
    e = hd.Engine(n_streams=3)
    yield e
    e.close()


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.complex64).view(np.float32).copy()).cuda()


def excess(p_gpu, p_ref, ppk):
    """largest error over bound; 0 where both are 0"""
    bound = 2e-5 * np.sqrt(p_ref * ppk) + 1e-10 * ppk + 66 * 2.0 ** -24 * p_ref
    err = np.abs(p_gpu - p_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))


def fsk_noise(n, seed, sigma=0.3):
    text = "".join(synth.make_sentence("TS", str(k)) for k in range(4))
    return synth.fsk_iq(synth.rtty_bits(text, 8, 2, 3, 0), 8000.0, 300.0, sigma=sigma, seed=seed, n_samples=n)


@pytest.fixture(scope="module")
def rows():
    """Three rows of LEN samples -- a unit impulse, a unit exponential on a bin centre, FSK plus noise -- and the model's spectrum of each: computed once."""
    x = np.zeros((3, LEN), np.complex64)
    x[0, 2048 + 100] = 1.0                                              # in segments 0 and 1, at window positions 2148 and 100
    x[1] = np.exp(2j * np.pi * 100 * np.arange(LEN) / N)
    x[2] = fsk_noise(LEN, 9)
    x.setflags(write=False)
    return x, [SM.spectrum(r) for r in x]


def state(ts, S):
    return [(ts.power(s)[0].tobytes(), ts.power(s)[1], tuple(sorted(ts.stats(s).items()))) for s in range(S)]


def pushed(eng, x, cut=None, n_per_stream=None, how="device"):
    """A fresh tone search fed the rows x in pushes of `cut` samples (None: one push), stream s up to n_per_stream[s] samples."""
    S, L = x.shape
    n_per_stream = np.full(S, L) if n_per_stream is None else np.asarray(n_per_stream)
    ts = eng.tone_search(max_push=max(L, 1))
    d = to_dev(x) if how == "device" else None
    for at in range(0, L, cut or L):
        n = np.clip(n_per_stream - at, 0, cut or L).astype(np.uint32)
        if how == "device":
            ts.push_device(d.data_ptr() + 8 * at, L, n)
        else:
            ts.push_host(np.ascontiguousarray(x[:, at:at + (cut or L)]), n)
    return ts


# ---------------------------------------------------------------- the rows against the model

def test_rows_against_the_float64_model(eng, rows):
    x, ref = rows
    ts = pushed(eng, x)
    for s, name in enumerate(("a unit impulse", "a unit exponential on bin 100", "FSK plus noise")):
        p_ref, segs, ppk, carry = ref[s]
        p, k = ts.power(s)
        ex = excess(p, p_ref, ppk)
        print(f"tone search, {name}: {k} segments, largest error over bound {ex:.4f}")
        assert k == segs == 6 and ts.stats(s) == dict(samples=LEN, segments=6, carry=carry) and carry == 777 + HOP, (name, k, ts.stats(s))
        assert ex <= 1.0, (name, ex)
    # what the basis inputs pin: the impulse's two segments weigh it with w[2148] and w[100], flat over the bins; the exponential's peak sits at the
    # fftshifted bin with its Hann neighbours a quarter of it
    w, sw2 = SM.window().astype(np.float64), SM.sum_w2()
    assert np.allclose(ts.power(0)[0], (w[2148] ** 2 + w[100] ** 2) / (6 * sw2), rtol=1e-3, atol=0)
    p = ts.power(1)[0]
    i = 100 + 2048
    assert int(np.argmax(p)) == i and p[i - 1] == pytest.approx(p[i] / 4, rel=1e-3) and p[i + 1] == pytest.approx(p[i] / 4, rel=1e-3)
    assert np.sort(p)[-4] < 1e-6 * p[i]
    assert all(eng.L.hd_debug_tone_search_guards(ts.h, s) == 0 for s in range(3))
    ts.close()


# ---------------------------------------------------------------- however the stream is cut

@pytest.fixture(scope="module")
def whole(eng, rows):
    ts = pushed(eng, rows[0])
    out = state(ts, 3)
    ts.close()
    return out


@pytest.mark.parametrize("cut", [63, 2047, 2048, 2049, 4095, 4097])
def test_however_the_stream_is_cut(eng, rows, whole, cut):
    ts = pushed(eng, rows[0], cut)
    assert state(ts, 3) == whole, cut
    assert all(eng.L.hd_debug_tone_search_guards(ts.h, s) == 0 for s in range(3))
    ts.close()


def test_pushes_of_one_sample(eng, rows):
    x = np.ascontiguousarray(rows[0][:, :N + HOP + 5])
    a, b = pushed(eng, x), pushed(eng, x, 1)
    assert a.stats(2) == dict(samples=N + HOP + 5, segments=2, carry=HOP + 5) and state(a, 3) == state(b, 3)
    assert all(eng.L.hd_debug_tone_search_guards(b.h, s) == 0 for s in range(3))
    a.close(); b.close()


def test_a_row_longer_than_one_launch_holds(eng):
    """HD_TONE_SEARCH_CHUNK + 4097 samples in one push are two launches; the same stream in pushes of 30000 must give the same bytes."""
    L = capi.TONE_SEARCH_CHUNK + 4097
    x = np.stack([fsk_noise(L, 20 + s) for s in range(3)])
    n = [L, 0, L - 1]
    a, b = pushed(eng, x, None, n), pushed(eng, x, 30000, n)
    assert a.stats(0)["segments"] == SM.segments_of(L) and a.stats(1) == dict(samples=0, segments=0, carry=0) and state(a, 3) == state(b, 3)
    p_ref, segs, ppk, _ = SM.spectrum(x[2, :L - 1])
    assert a.power(2)[1] == segs and excess(a.power(2)[0], p_ref, ppk) <= 1.0
    a.close(); b.close()


# ---------------------------------------------------------------- unequal rows

def test_unequal_rows_in_one_launch(eng):
    first, then = [0, 5000, 12000], [1, 4095, 2048]
    x = np.stack([fsk_noise(12000 + 4095, 30 + s) for s in range(3)])
    ts = eng.tone_search(max_push=12000)
    ts.push_host(np.ascontiguousarray(x[:, :12000]), first)
    assert [ts.stats(s)["segments"] for s in range(3)] == [0, 1, 4]
    y = np.zeros((3, 4095), np.complex64)
    for s in range(3):
        y[s, :then[s]] = x[s, first[s]:first[s] + then[s]]
    ts.push_host(y, then)
    assert [ts.stats(s)["segments"] for s in range(3)] == [0, 3, 5]
    for s in range(3):                                                # each stream against its own single-stream run: one push, the neighbours empty
        n = np.zeros(3, np.uint32)
        n[s] = first[s] + then[s]
        alone = eng.tone_search(max_push=20000)
        alone.push_host(x, n)
        assert state(alone, 3)[s] == state(ts, 3)[s], s
        assert ts.stats(s) == dict(samples=first[s] + then[s], segments=[0, 3, 5][s], carry=first[s] + then[s] - HOP * [0, 3, 5][s])
        alone.close()
    assert all(eng.L.hd_debug_tone_search_guards(ts.h, s) == 0 for s in range(3))
    ts.close()


# ---------------------------------------------------------------- the three doors

def test_host_door_equals_device_door(eng, rows, whole):
    ts = pushed(eng, rows[0], 4097, how="host")
    assert state(ts, 3) == whole
    ts.close()


def test_engine_door_equals_push_device_of_the_decimated_copies(hd):
    W = TM.WEAK
    iq, _ = TM.weak_iq(1.0)
    S, n = W["S"], W["n"]
    e = hd.Engine(n_streams=S, max_chunk=n, sampling_rate=W["fs"], decimation=W["D"], baud=W["baud"], rtty_bits=8, rtty_stops=2, lowpass_bw_hz=W["bw"])
    door, copies = e.tone_search(), e.tone_search()
    door.push_engine()                                                # no call yet: adds nothing
    assert door.stats(0) == dict(samples=0, segments=0, carry=0)
    for k in range(2):
        e.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        door.push_engine()
        dec = np.stack([e.decimated(s) for s in range(S)])
        assert dec.shape == (S, n // W["D"])
        d = to_dev(dec)
        copies.push_device(d.data_ptr(), dec.shape[1], np.full(S, dec.shape[1], np.uint32))
        door.push_engine()                                            # a second push without a new call adds nothing
        assert state(door, S) == state(copies, S), k
    assert door.stats(3) == dict(samples=8000, segments=2, carry=8000 - 2 * HOP)
    assert all(e.L.hd_debug_tone_search_guards(door.h, s) == 0 for s in range(S))
    e.close()


# ---------------------------------------------------------------- reset, NaN and Inf

def test_reset_of_one_stream_and_of_all(eng, rows, whole):
    x = rows[0]
    ts = pushed(eng, x, 4097)
    ts.reset(1)
    assert ts.stats(1) == dict(samples=0, segments=0, carry=0) and ts.power(1)[1] == 0 and not ts.power(1)[0].any()
    assert state(ts, 3)[0] == whole[0] and state(ts, 3)[2] == whole[2]
    n = np.array([0, LEN, 0], np.uint32)
    ts.push_host(x, n)                                                # and the stream goes on from zero
    assert state(ts, 3) == whole
    ts.reset()
    assert all(ts.stats(s) == dict(samples=0, segments=0, carry=0) and not ts.power(s)[0].any() for s in range(3))
    ts.push_host(x)
    assert state(ts, 3) == whole
    ts.close()


def test_nan_and_inf_stay_in_their_stream(eng):
    L = N + 9 * HOP
    x = np.stack([fsk_noise(L, 40 + s) for s in range(3)])
    clean = pushed(eng, x, 5000)
    bad = x.copy()
    bad[1, 3000] = np.nan
    bad[1, 17000] = np.inf
    ts = pushed(eng, bad, 5000)
    assert state(ts, 3)[0] == state(clean, 3)[0] and state(ts, 3)[2] == state(clean, 3)[2]
    p, k = ts.power(1)
    assert k == 10 and not np.isfinite(p).any()
    assert ts.detect(1, baud=300.0)["valid"] == 0 and ts.detect(0, baud=300.0)["segments"] == 10
    ts.reset(1)
    ts.push_host(x, np.array([0, L, 0], np.uint32))                   # the reset clears it
    assert state(ts, 3) == state(clean, 3)
    ts.close(); clean.close()


# ---------------------------------------------------------------- errors

def test_errors(eng, rows):
    L = eng.L
    x = rows[0]
    h = C.c_void_p()
    assert L.hd_tone_search_create(None, None, C.byref(h)) == HD_ERR_INVALID and L.hd_tone_search_create(eng.h, None, None) == HD_ERR_INVALID
    par = capi.hd_tone_search_params(max_push=(1 << 28) + 1)
    assert L.hd_tone_search_create(eng.h, C.byref(par), C.byref(h)) == HD_ERR_INVALID
    ts = eng.tone_search(max_push=LEN)
    d = to_dev(x)
    n = np.full(3, LEN, np.uint32)
    assert L.hd_tone_search_push_engine(None) == HD_ERR_INVALID and L.hd_tone_search_reset(None, 0) == HD_ERR_INVALID and L.hd_tone_search_reset(ts.h, 3) == HD_ERR_INVALID
    assert L.hd_tone_search_push_device(None, d.data_ptr(), LEN, n.ctypes.data, 0) == HD_ERR_INVALID
    assert L.hd_tone_search_push_device(ts.h, None, LEN, n.ctypes.data, 0) == HD_ERR_INVALID and L.hd_tone_search_push_host(ts.h, None, LEN, None, LEN) == HD_ERR_INVALID
    assert L.hd_tone_search_push_device(ts.h, d.data_ptr() + 4, LEN, None, LEN - 1) == HD_ERR_INVALID and b"8-byte" in L.hd_last_error()      # misaligned rows
    assert L.hd_tone_search_push_host(ts.h, x.ctypes.data + 4, LEN, None, LEN - 1) == HD_ERR_INVALID
    assert L.hd_tone_search_push_device(ts.h, x.ctypes.data, LEN, None, LEN) == HD_ERR_INVALID            # host memory is not device memory
    long = np.array([LEN, LEN + 1, 3], np.uint32)
    assert L.hd_tone_search_push_host(ts.h, x.ctypes.data, LEN, long.ctypes.data, 0) == HD_ERR_INVALID    # a row longer than the stride
    big = np.zeros((3, LEN + 1), np.complex64)
    assert L.hd_tone_search_push_host(ts.h, big.ctypes.data, LEN + 1, None, LEN + 1) == HD_ERR_CAPACITY   # longer than max_push: nothing is added
    assert all(ts.stats(s) == dict(samples=0, segments=0, carry=0) for s in range(3))
    p, seg, info, res = np.ones(N), C.c_uint64(7), capi.hd_tone_search_info(), capi.hd_tone_search_result()
    dpar = capi.hd_tone_search_detect_params()
    L.hd_tone_search_detect_params_default(C.byref(dpar))
    assert L.hd_tone_search_power(None, 0, p.ctypes.data, N, C.byref(seg)) == HD_ERR_INVALID and L.hd_tone_search_power(ts.h, 3, p.ctypes.data, N, C.byref(seg)) == HD_ERR_INVALID
    assert L.hd_tone_search_power(ts.h, 0, None, N, C.byref(seg)) == HD_ERR_INVALID
    assert L.hd_tone_search_stats(ts.h, 0, None) == HD_ERR_INVALID and L.hd_tone_search_stats(ts.h, 3, C.byref(info)) == HD_ERR_INVALID
    assert L.hd_tone_search_detect(ts.h, 0, None, C.byref(res)) == HD_ERR_INVALID and L.hd_tone_search_detect(ts.h, 0, C.byref(dpar), None) == HD_ERR_INVALID
    assert L.hd_tone_search_detect(None, 0, C.byref(dpar), C.byref(res)) == HD_ERR_INVALID
    ts.push_device(d.data_ptr(), LEN, n)
    assert L.hd_tone_search_power(ts.h, 0, p.ctypes.data, N - 1, C.byref(seg)) == 0 and seg.value == 6 and p.all()       # cap < 4096: the count alone
    assert L.hd_tone_search_detect(ts.h, 2, C.byref(dpar), C.byref(res)) == HD_ERR_INVALID               # baud = 0
    dpar.baud = 300.0
    assert L.hd_tone_search_detect(ts.h, 2, C.byref(dpar), C.byref(res)) == HD_ERR_UNSUPPORTED           # six segments
    with pytest.raises(Exception, match="error -3"):
        ts.detect(2, baud=300.0)
    ts.push_device(d.data_ptr(), LEN, n)
    assert ts.stats(2)["segments"] == SM.segments_of(2 * LEN) >= 8
    dpar.shift_hi_hz = 100.0
    assert L.hd_tone_search_detect(ts.h, 2, C.byref(dpar), C.byref(res)) == HD_ERR_INVALID
    dpar.shift_hi_hz = 1000.0
    assert L.hd_tone_search_detect(ts.h, 2, C.byref(dpar), C.byref(res)) == 0 and res.segments == ts.stats(2)["segments"]
    want = SM.detect(ts.power(2)[0], res.segments, L.hd_engine_decimated_rate(eng.h), 300.0)
    assert (res.bin_lo, res.shift_bins, res.w, res.valid) == (want["bin_lo"], want["shift_bins"], want["w"], want["valid"])
    assert all(L.hd_debug_tone_search_guards(ts.h, s) == 0 for s in range(3))
    ts.close()
    L.hd_tone_search_destroy(None)


# ---------------------------------------------------------------- what it is for: a weak signal whose tones nobody knows, end to end

def test_found_tones_decode_a_signal_below_the_discriminators_threshold(hd):
    W = TM.WEAK
    iq, sent = TM.weak_iq(1.0)
    S, n, calls, fsd = W["S"], W["n"], W["calls"], W["fs"] / W["D"]
    cfg = dict(n_streams=S, max_chunk=n, sampling_rate=W["fs"], decimation=W["D"], baud=W["baud"], rtty_bits=8, rtty_stops=2, lowpass_bw_hz=W["bw"])
    # pass 1: the search
    eng = hd.Engine(**cfg)
    ts = eng.tone_search()
    found = {}
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        ts.push_engine()
        if k + 1 in (6, calls):
            found[k + 1] = [ts.detect(s, baud=W["baud"]) for s in range(S)]
    for after, res in found.items():
        for s, r in enumerate(res):
            a = eng.afc(s)
            err = max(abs(r["f_hi_hz"] - TM.SHIFT / 2), abs(r["f_lo_hz"] + TM.SHIFT / 2))
            print(f"tone search after {after} calls, stream {s}: {r['segments']} segments, tones {r['f_lo_hz']:.1f} {r['f_hi_hz']:.1f} (error {err:.1f} Hz), quality "
                  f"{r['quality']:.2f}; the AFC's peaks {(a['peak_l'] - 2048) * fsd / 4096:.1f} {(a['peak_r'] - 2048) * fsd / 4096:.1f}")
            assert r["valid"] == 1 and err <= 25.0 and r["segments"] == SM.segments_of(after * n // W["D"]), (after, s, r)
    assert all(eng.L.hd_debug_tone_search_guards(ts.h, s) == 0 for s in range(S))
    eng.close()
    # pass 2, a fresh engine: tone filters with the found tones and with the true ones, each into a clocked decoder
    eng = hd.Engine(**cfg)
    ordinary = []
    eng.on_sentence(lambda s, call, data, crc: ordinary.append((s, call, data)))
    tones = dict(found=eng.tones(), true=eng.tones())
    clocked = dict(found=eng.clocked(), true=eng.clocked())
    for s in range(S):
        tones["found"].set_modem(s, W["baud"], found[calls][s]["f_hi_hz"], found[calls][s]["f_lo_hz"])
        tones["true"].set_modem(s, W["baud"], TM.SHIFT / 2, -TM.SHIFT / 2)
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        for key in tones:
            tones[key].push_engine()
            clocked[key].push_tones(tones[key])
    eng.flush()
    count = {}
    for key in tones:
        plain = total = 0
        for s in range(S):
            got = clocked[key].take_sentences(s, 256)
            assert all(t in sent[s] for (_, _, t) in got), (key, s, got)                # nothing delivered that was not sent
            plain += len([1 for g in got if g[1] == 0]); total += len(got)
        count[key] = (plain, total)
    print("tone search end to end at sigma 1.0: sentences plain / with repair: true tones", count["true"], "found tones", count["found"], "of", 12 * S, "sent")
    assert count["found"][0] >= count["true"][0] - 3 and count["found"][1] >= count["true"][1] - 3, count
    assert ordinary == []                                             # the ordinary chain delivers nothing at this level
    eng.close()
