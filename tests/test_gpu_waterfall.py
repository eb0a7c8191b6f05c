"""The waterfall on the GPU (hd_waterfall_*, include/habdec_amd.h; kernels/waterfall.hip and, for the rows, kernels/survey.hip).

Rows: the float64 numpy model of tests/test_waterfall_host.py (model_rows: the survey's window, np.fft.fft per segment in complex128, summed per row),
held against the GPU's rows with the gate of tests/test_gpu_survey.py per row, on the sums normalised by segments * sum w^2:
    |P_gpu[i] - P_ref[i]| <= 2e-5 sqrt(P_ref[i] Ppk) + 1e-10 Ppk + 66 * 2^-24 P_ref[i]
(Ppk: the largest single-segment bin power of the row's model; derived in that file's docstring for one run of at most 64 segments, which is what a row
is).  Largest measured error over bound per case: NOTES.md.

Detector: byte equality with hd_host_waterfall_detect_row, and with the numpy model of the GPU's own rows.

What it is for (test 7): the three-payload recording of tests/test_gpu_survey.py with the +250 kHz payload switched on only from T_ON.  Its third
sentence ends 33 bit times before the recording does; the text stage holds a last line until more text follows (as in the survey's test, whose streams
deliver two of three sentences), so neither the CPU oracle nor the engine can deliver it: of the second and third sentences, which lie wholly inside
the on-time, the oracle fed the rotated recording from T_ON delivers the second, and the test holds the engine to exactly what the oracle delivers."""
import ctypes as C

import numpy as np
import pytest

import test_survey_host as sh
import test_waterfall_host as wh
from habdec_amd import capi, synth
from iq_formats_util import FMTS, convert, quantise

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


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def state(wf):
    """(headers, marks, rows still in the ring) of a waterfall"""
    total = wf.rows_total()
    kept = min(total, wf.params.rows_cap)
    return wf.headers(), wf.marks(), wf.rows(total - kept, kept)


def same_state(a, b):
    return all(same(x, y) for x, y in zip(a, b))


def check_detector_of_own_rows(wf, **params):
    """the marks the GPU made are the numpy model's marks of the GPU's rows"""
    h, m, rows = state(wf)
    assert len(rows) == len(h)
    for j in range(len(h)):
        flags, floor, level, marks = wh.model_row(rows[j], int(h["segments"][j]), FS, **params)
        assert (int(h["flags"][j]), wh.bits_of(h["floor"][j]), wh.bits_of(h["level"][j])) == (flags, wh.bits_of(floor), wh.bits_of(level)), (j, h[j])
        assert np.array_equal(m[j], marks) and int(h["n_marked"][j]) == len(wh.marked(marks)), j


# ---- 1. rows against the Welch model
SW2 = float(np.sum(sh.window().astype(np.float64) ** 2))
ROW_CASES = {
    "one_row_of_16": (16, [N + 15 * HOP], [16]),
    "16_16_3_ends_short": (16, [N + 34 * HOP], [16, 16, 3]),
    "L64_one_full_row": (64, [N + 63 * HOP], [64]),
    "L64_second_row_of_one": (64, [N + 64 * HOP], [64, 1]),
    "4095_between_two_pushes": (16, [N + 15 * HOP + 100, 4095, N + 16 * HOP], [16, 16, 1]),
}


@pytest.mark.parametrize("name", list(ROW_CASES))
def test_rows_against_the_welch_model(eng, name):
    L_seg, sizes, segs = ROW_CASES[name]
    x = noise_and_tone(sum(sizes), seed=len(name))
    pushes = np.split(x, np.cumsum(sizes)[:-1])
    wf = eng.waterfall(slot_segments=L_seg)
    keep, before, want_first, worst = [], 0, [], 0.0
    ref_rows = []
    for q in pushes:
        d = to_dev(q)
        keep.append(d)
        wf.push_device(d.data_ptr(), len(q))
        rows, h = wh.model_rows(q, L_seg, before)
        ref_rows += [(rows[j], int(h["segments"][j]), q[j * L_seg * HOP:]) for j in range(len(rows))]
        want_first += [int(v) for v in h["first_sample"]]
        before += len(q)
    h = wf.headers()
    assert [int(v) for v in h["segments"]] == segs and [int(v) for v in h["first_sample"]] == want_first, h
    assert [bool(f & capi.WF_SHORT) for f in h["flags"]] == [s < 16 for s in segs]
    got = wf.rows(0, len(h), normalised=True)
    for j, (ref, k, tail) in enumerate(ref_rows):
        ppk = float(sh.periodograms(tail[:N + (k - 1) * HOP]).max()) / SW2
        p_ref = ref / (k * SW2)
        bound = 2e-5 * np.sqrt(p_ref * ppk) + 1e-10 * ppk + 66 * 2.0 ** -24 * p_ref
        ex = float(np.max(np.abs(got[j] - p_ref) / bound))
        worst = max(worst, ex)
        assert ex <= 1.0, (name, j, ex)
    print(f"{name}: rows of {segs} segments, largest error over bound {worst:.4f}")
    if name == "4095_between_two_pushes":
        assert want_first == [0, sizes[0] + 4095, sizes[0] + 4095 + 16 * HOP]
    assert int(h["n_marked"][0]) > 0 and wh.marked(wf.marks(0, 1)[0])[0] in range(2048 + 240, 2048 + 255)       # the tone, near bin 2048 + 123456.7 / 500
    check_detector_of_own_rows(wf)
    wf.close()


# ---- 2. the detector on the GPU: every hand-made row, from host and from device memory
@pytest.mark.parametrize("group", range(len(wh.by_params())))
def test_detector_on_hand_made_rows(eng, group):
    import torch
    params, names = wh.by_params()[group]
    rows = np.stack([wh.HAND[n][0] for n in names])
    segs = np.array([wh.HAND[n][1] for n in names], np.uint32)
    a, b = eng.waterfall(**params), eng.waterfall(**params)
    a.push_rows(rows, segs)
    d = torch.from_numpy(rows).cuda()
    b.push_rows(d.data_ptr(), segs)
    if len(names) > 1:
        b.push_rows(d.data_ptr() + N * 4, segs[1:])                  # and again, from the second row on: the sample count goes on
    ha, ma = a.headers(), a.marks()
    assert same(a.rows(0, len(names)), rows)
    at = 0
    for j, n in enumerate(names):
        rc, hdr, marks = wh.c_row(eng.L, rows[j], int(segs[j]), **params)
        assert rc == 0
        hdr["first_sample"] = at
        at += int(segs[j]) * HOP
        assert ha[j].tobytes() == hdr.tobytes(), (n, ha[j], hdr)
        assert np.array_equal(ma[j], marks), (n, wh.marked(ma[j]), wh.marked(marks))
    hb, mb = b.headers(), b.marks()
    assert same(hb[:len(names)], ha) and same(mb[:len(names)], ma)
    if len(names) > 1:
        assert b.rows_total() == 2 * len(names) - 1 and same(mb[len(names):], ma[1:])
        assert np.array_equal(hb["first_sample"][len(names):].astype(np.int64), ha["first_sample"][1:].astype(np.int64) + (at - int(segs[0]) * HOP))
        for f in ("segments", "flags", "floor", "level", "n_marked"):
            assert hb[f][len(names):].tobytes() == ha[f][1:].tobytes(), f
    unflagged = ha["flags"] == 0
    hits, counted = a.hits()
    assert counted == int(unflagged.sum()) and np.array_equal(hits, a.marks_bool()[unflagged].sum(axis=0).astype(np.uint32))
    a.close(); b.close()


# ---- 3. the same bytes from every door
def test_same_bytes_from_every_door(eng, monkeypatch):
    import torch
    sizes = [N + 86 * HOP + 777, 4095, N + 299 * HOP]                # 5 rows and a short one of 7; no row; 300 segments: two staging slabs, 19 rows
    x = noise_and_tone(sum(sizes), seed=31)
    pushes = np.split(x, np.cumsum(sizes)[:-1])
    ref = eng.waterfall()
    keep = [to_dev(q) for q in pushes]
    for d, q in zip(keep, pushes):
        ref.push_device(d.data_ptr(), len(q))
    want = state(ref)
    h = want[0]
    assert [int(s) for s in h["segments"]] == [16] * 5 + [7] + [16] * 18 + [12]
    assert int(h["first_sample"][6]) == sizes[0] + 4095 and int(h["first_sample"][5]) == 5 * 16 * HOP
    again = eng.waterfall()
    for d, q in zip(keep, pushes):
        again.push_device(d.data_ptr(), len(q))
    assert same_state(state(again), want)
    monkeypatch.setenv("HD_SURVEY_RUNS", "2")                        # (the survey's launch shape is not the waterfall's: rows are runs of L, whatever it says)
    host, pinned = eng.waterfall(), eng.waterfall()
    for q in pushes:
        host.push_host(q)
        buf = eng.pinned_array(len(q))
        buf[:] = q
        pinned.push_host(buf)
    assert same_state(state(host), want) and same_state(state(pinned), want)
    monkeypatch.delenv("HD_SURVEY_RUNS")
    for fmt, (code, dt, bps) in FMTS.items():
        packed = [quantise(fmt, q) for q in pushes]
        floats = [convert(fmt, p) for p in packed]
        fref, fhost, fdev, fhost_code = eng.waterfall(), eng.waterfall(), eng.waterfall(), eng.waterfall()
        for p, f in zip(packed, floats):
            fref.push_host(f)
            fhost.push_host(p, fmt=fmt)
            fhost_code.push_host(p, fmt=code)
            d = torch.from_numpy(p).cuda()
            fdev.push_device(d.data_ptr(), len(p), fmt=fmt)
        w = state(fref)
        assert same(w[0]["first_sample"], h["first_sample"]) and same(w[0]["segments"], h["segments"])
        assert same_state(state(fhost), w) and same_state(state(fdev), w) and same_state(state(fhost_code), w), fmt
        # a packed base off 8-byte alignment: one sample further on (4 bytes cs16, 2 bytes cs8 / cu8)
        d = torch.from_numpy(packed[0]).cuda()
        assert (d.data_ptr() + bps) % 8 != 0
        fref.push_host(floats[0][1:]); fdev.push_device(d.data_ptr() + bps, sizes[0] - 1, fmt=fmt); fhost.push_host(packed[0][1:], fmt=fmt)
        w = state(fref)
        assert same_state(state(fdev), w) and same_state(state(fhost), w), fmt
        assert int(w[0]["first_sample"][-6]) == sum(sizes)
        for v in (fref, fhost, fdev, fhost_code):
            v.close()
    for v in (ref, again, host, pinned):
        v.close()


# ---- 4. hits and reset
def test_hits_and_reset(eng):
    wf = eng.waterfall()
    keep = []
    for k, n in enumerate([N + 40 * HOP, CH, N + 15 * HOP]):         # 3 rows (16, 16, 9: the last short), 2 rows (16, 15: short), 1 row
        d = to_dev(noise_and_tone(n, seed=40 + k, f=-300e3 + 250e3 * k))
        keep.append(d)
        wf.push_device(d.data_ptr(), n)
    h = wf.headers()
    assert [int(s) for s in h["segments"]] == [16, 16, 9, 16, 15, 16] and [int(f) for f in h["flags"]] == [0, 0, 1, 0, 1, 0]
    hits, counted = wf.hits()
    mb = wf.marks_bool()
    assert counted == 4 and np.array_equal(hits, mb[h["flags"] == 0].sum(axis=0).astype(np.uint32))
    assert hits.max() == 2 and int(hits.sum()) == int(h["n_marked"].sum()) and not mb[h["flags"] != 0].any()
    first = state(wf)
    wf.reset()
    hits, counted = wf.hits()
    assert wf.rows_total() == 0 and counted == 0 and not hits.any() and len(wf.headers()) == 0 and wf.tracks() == []
    wf.push_device(keep[0].data_ptr(), N + 40 * HOP)                 # and goes on from zero
    assert same_state(state(wf), tuple(v[:3] for v in first)) and int(wf.headers()["first_sample"][0]) == 0
    assert wf.hits()[1] == 2
    wf.close()


# ---- 5. the ring
def test_the_ring(eng):
    n = N + (6 * 16 - 1) * HOP
    d = to_dev(noise_and_tone(n, seed=50))
    small, big = eng.waterfall(rows_cap=4), eng.waterfall()
    small.push_device(d.data_ptr(), n)
    big.push_device(d.data_ptr(), n)
    assert small.rows_total() == big.rows_total() == 6
    out = np.zeros((4, N), np.float32)
    assert eng.L.hd_waterfall_rows(small.h, 0, 2, out.ctypes.data) == -1 and b"ring" in eng.L.hd_last_error()
    assert eng.L.hd_waterfall_rows(small.h, 1, 1, out.ctypes.data) == -1 and eng.L.hd_waterfall_rows(small.h, 3, 4, out.ctypes.data) == -1
    assert same(small.rows(2, 4), big.rows(2, 4)) and same(small.rows(5, 1), big.rows(5, 1)) and small.rows(6, 0).shape == (0, N)
    assert same(small.headers(), big.headers()) and same(small.marks(), big.marks()) and small.hits()[1] == 6
    assert small.tracks() == big.tracks() and len(big.tracks()) == 1
    one = eng.waterfall(rows_cap=1)                                   # every launch is one row
    one.push_device(d.data_ptr(), n)
    assert same(one.headers(), big.headers()) and same(one.marks(), big.marks()) and same(one.rows(5, 1), big.rows(5, 1))
    assert np.array_equal(one.hits()[0], big.hits()[0])
    for v in (small, big, one):
        v.close()


def test_several_launches(eng, monkeypatch):
    """HD_WATERFALL_CHUNK=4: a push of 11 rows (the last short) is three launches of 4, 4 and 3 rows; with rows_cap = 6 the cuts fall at rows 4, 6 (the
    ring wraps), 10 and 11.  Rows, headers, marks and hits are those of the one launch."""
    import torch
    n = N + (10 * 16 + 5 - 1) * HOP
    d = to_dev(noise_and_tone(n, seed=51))
    one = eng.waterfall()
    one.push_device(d.data_ptr(), n)
    assert [int(s) for s in one.headers()["segments"]] == [16] * 10 + [5]
    monkeypatch.setenv("HD_WATERFALL_CHUNK", "4")
    cut, ring = eng.waterfall(), eng.waterfall(rows_cap=6)
    monkeypatch.delenv("HD_WATERFALL_CHUNK")
    cut.push_device(d.data_ptr(), n)
    ring.push_host(noise_and_tone(n, seed=51))
    assert same_state(state(cut), state(one))
    assert same(ring.headers(), one.headers()) and same(ring.marks(), one.marks()) and same(ring.rows(5, 6), one.rows(5, 6))
    assert np.array_equal(cut.hits()[0], one.hits()[0]) and np.array_equal(ring.hits()[0], one.hits()[0]) and one.hits()[1] == 10
    # push_rows through the same cuts
    rows, segs = one.rows(0, 11), one.headers()["segments"]
    dr = torch.from_numpy(rows).cuda()
    cut.push_rows(dr.data_ptr(), segs)
    ring.push_rows(rows, segs)
    for v in (cut, ring):
        assert v.rows_total() == 22 and same(v.marks(11), one.marks()) and v.hits()[1] == 20
        for f in ("segments", "flags", "floor", "level", "n_marked"):
            assert v.headers(11)[f].tobytes() == one.headers()[f].tobytes(), f
    assert same(cut.rows(11, 11), rows) and same(ring.rows(16, 6), rows[5:])
    for v in (one, cut, ring):
        v.close()


# ---- 6. the engine is left alone
def test_the_engine_is_left_alone(hd):
    """tests/test_gpu_survey.py's test of this name with a waterfall push between every two calls: a pipeline = 1 engine, 64 streams; launch paths, folded
    discriminator checksums and characters of every stream are those of the run without a waterfall."""
    import torch
    S, n_calls = 64, 6
    base = np.stack([synth.fsk_iq(synth.rtty_bits(synth.make_sentence(f"WF{s}", f"{s},1.5,2.5") * 3, 8, 2, 6 + 3 * s, 10), FS, 300, sigma=0.05, seed=80 + s,
                                  n_samples=n_calls * CH, f0=100.0 * s) for s in range(4)])
    dev = [to_dev(base[:, k * CH:(k + 1) * CH]).reshape(4, 2 * CH).repeat(S // 4, 1).contiguous() for k in range(n_calls)]
    torch.cuda.synchronize()
    results = []
    for with_waterfall in (False, True):
        e = hd.Engine(n_streams=S, sampling_rate=FS, decimation=64, pipeline=1)
        wf = e.waterfall() if with_waterfall else None
        paths = []
        for k in range(n_calls):
            e.process_device(dev[k].data_ptr(), CH, CH)
            paths.append(e.timing()["path"])
            if wf and k + 1 < n_calls:
                wf.push_device(dev[k].data_ptr(), S * CH)
        e.flush()
        if wf:
            rows_per_push = -(-sh.segments_of(S * CH) // 16)
            assert wf.rows_total() == (n_calls - 1) * rows_per_push and wf.hits()[1] == (n_calls - 1) * (rows_per_push - 1)       # (each push ends in a short row)
        results.append((paths, [e.demod_checksum_total(s) for s in range(S)], [e.take_chars(s) for s in range(S)]))
        e.close()
    assert results[0][0] == results[1][0], (results[0][0], results[1][0])
    assert results[0][1] == results[1][1] and all(c[0] == n_calls for c in results[0][1])
    assert results[0][2] == results[1][2]


# ---- 7. what it is for
FAN = dict(fs=2.048e6, n_calls=56, offsets=[-600e3, 250e3, 5e3], calls=["WIDEA", "WIDEB", "WIDEC"], noise=0.05, gated=1)
T_ON = 11 * CH + 10000                                                # inside the gated payload's first sentence
BIT = FAN["fs"] / 300.0


def sentence_spans(j, texts):
    """[(first sample, one past the last sample, 'CALL,fields*CRC')] of payload j's sentences: 11 bit times per character behind 6 + 3 j idle bits"""
    at, out = 6 + 3 * j, []
    for line in texts[j].split("\n")[:-1]:
        bits = 11 * (len(line) + 1)
        out.append((int(at * BIT), int(np.ceil((at + bits) * BIT)), line.lstrip("$")))
        at += bits
    return out


def fan_recording():
    fs, n = FAN["fs"], FAN["n_calls"] * CH
    texts = ["".join(synth.make_sentence(c, str(i)) for i in range(3)) for c in FAN["calls"]]
    rec = np.zeros(n, np.complex128)
    for j, (f, t) in enumerate(zip(FAN["offsets"], texts)):
        sig = synth.fsk_iq(synth.rtty_bits(t, 8, 2, 6 + 3 * j, 10), fs, 300, sigma=0.0, seed=j, n_samples=n, f0=f)
        if j == FAN["gated"]:
            sig = sig * (np.arange(n) >= T_ON)
        rec += sig
    nz = synth._noise(n, 7)
    return (rec + FAN["noise"] * (nz[0::2] + 1j * nz[1::2])).astype(np.complex64), texts


def rotated(L, x, f, fs):
    step = C.c_uint32(0)
    assert L.hd_host_tune_step(f, fs, C.byref(step)) == 0
    out = np.zeros(2 * len(x), np.float32)
    L.hd_host_tune_rotate(np.ascontiguousarray(x).view(np.float32), len(x), 0, step.value, out)
    return out.view(np.complex64)


def oracle_sentences(L, x, f, fs):
    from oracle import pyoracle
    dec = pyoracle.Decoder("oracle", factor=64)
    y = rotated(L, x, f, fs)
    for k in range(0, len(y), CH):
        dec(y[k:k + CH], fs)
    return dec.sentences()


def test_tracks_then_front_tune_decode_what_lies_inside_them(hd):
    fs, n_calls, g = FAN["fs"], FAN["n_calls"], FAN["gated"]
    rec, texts = fan_recording()
    spans = [sentence_spans(j, texts) for j in range(3)]
    assert T_ON > spans[g][0][0] and spans[g][1][0] > T_ON and spans[g][2][1] <= len(rec)          # the second and third sentences lie wholly inside the on-time
    L = hd.lib()
    from_t_on = oracle_sentences(L, rec[T_ON:], FAN["offsets"][g], fs)
    whole = oracle_sentences(L, rec, FAN["offsets"][g], fs)
    assert spans[g][1][2] in from_t_on and spans[g][0][2] not in whole                              # (gated off, the first sentence is not there to decode)
    assert from_t_on == whole == [s[2] for s in spans[g][1:] if s[2] in whole], (from_t_on, whole)
    dev = to_dev(rec)
    eng = hd.Engine(n_streams=4, sampling_rate=fs, decimation=64)
    wf = eng.waterfall()
    wf.push_device(dev.data_ptr(), len(rec))
    h = wf.headers()
    unflagged = np.flatnonzero(h["flags"] == 0)
    assert len(h) == 112 and len(unflagged) == 111 and int(h["flags"][-1]) == capi.WF_SHORT
    tracks = wf.tracks()
    for t in tracks:
        print(f"track at {t['offset_hz']:10.1f} Hz: samples {t['first_sample']}-{t['end_sample']}, rows {t['first_row']}-{t['last_row']}, {t['rows_hit']} hit, open {t['open']}")
    assert len(tracks) == 3, tracks
    by_payload = [min(tracks, key=lambda t: abs(t["offset_hz"] - f)) for f in FAN["offsets"]]
    for j, (t, f) in enumerate(zip(by_payload, FAN["offsets"])):
        assert abs(t["offset_hz"] - f) <= 250 + 500, (t, f)
        if j == g:
            assert abs(t["first_sample"] - T_ON) <= 17 * HOP and t["open"] == 1 and t["last_row"] == unflagged[-1], t
        else:
            assert (t["first_row"], t["last_row"], t["rows_hit"], t["open"]) == (0, unflagged[-1], len(unflagged), 1), t
    sv = eng.survey()
    sv.push_device(dev.data_ptr(), len(rec))
    cands = sv.detect()
    near = [c for c in cands if abs(c["offset_hz"] - FAN["offsets"][g]) <= 750]
    print(f"hd_survey_detect over the whole capture: {len(cands)} candidates; the gated payload: " + (f"snr {near[0]['snr_db']:.1f} dB" if near else "not found"))
    for s, t in enumerate(by_payload):
        eng.set_front_tune(s, t["offset_hz"])
    for k in range(n_calls):
        eng.process_device(dev.data_ptr() + k * CH * 8, 0, CH)
    got = [eng.take_sentences(s) for s in range(4)]
    for j, t in enumerate(by_payload):
        inside = [s[2] for s in spans[j] if s[0] >= t["first_sample"] and s[1] <= t["end_sample"]]
        delivered = oracle_sentences(L, rec, FAN["offsets"][j], fs) if j != g else whole
        assert inside == ([s[2] for s in spans[j]] if j != g else [s[2] for s in spans[j][1:]]), (j, inside)
        assert got[j] == [s for s in inside if s in delivered] and len(got[j]) >= 1, (j, got[j], inside, delivered)
    assert got[3] == []
    eng.close()


# ---- 8. errors: all host-side checks, nothing reaches a kernel
def test_errors(hd, eng):
    import torch
    L = eng.L
    d = to_dev(noise_and_tone(CH, 8))
    h = C.c_void_p()
    par = capi.hd_waterfall_params()
    L.hd_waterfall_params_default(C.byref(par))
    assert L.hd_waterfall_create(None, C.byref(par), C.byref(h)) == -1 and L.hd_waterfall_create(eng.h, C.byref(par), None) == -1
    for k, v in (("slot_segments", 15), ("slot_segments", 65), ("rows_cap", 0), ("threshold_db", -1.0), ("threshold_db", float("nan")),
                 ("dc_guard_hz", -1.0), ("dc_guard_hz", float("nan")), ("dc_guard_hz", 2e6)):
        bad = capi.hd_waterfall_params()
        L.hd_waterfall_params_default(C.byref(bad))
        setattr(bad, k, v)
        assert L.hd_waterfall_create(eng.h, C.byref(bad), C.byref(h)) == -1 and not h.value, (k, v)
    assert L.hd_waterfall_create(eng.h, None, C.byref(h)) == 0 and h.value                        # null parameters: the defaults
    L.hd_waterfall_destroy(h)
    wf = eng.waterfall()
    assert L.hd_waterfall_push_device(None, d.data_ptr(), CH) == -1 and L.hd_waterfall_push_host(None, d.data_ptr(), CH) == -1
    assert L.hd_waterfall_push_device(wf.h, None, CH) == -1 and L.hd_waterfall_push_host(wf.h, None, CH) == -1
    assert L.hd_waterfall_push_device(wf.h, d.data_ptr() + 4, CH - 1) == -1 and b"8-byte" in L.hd_last_error()
    pageable = noise_and_tone(CH, 9)
    assert L.hd_waterfall_push_device(wf.h, pageable.ctypes.data, CH) == -1                      # host memory HIP does not know: refused, not launched
    packed = quantise("cs16", pageable)
    dp = torch.from_numpy(packed).cuda()
    assert L.hd_waterfall_push_host_fmt(wf.h, 9, packed.ctypes.data, CH) == -1 and L.hd_waterfall_push_device_fmt(wf.h, 1, None, CH) == -1
    assert L.hd_waterfall_push_device_fmt(wf.h, 1, dp.data_ptr() + 2, CH - 1) == -1 and L.hd_waterfall_push_host_fmt(wf.h, 1, packed.ctypes.data + 2, CH - 1) == -1
    assert L.hd_waterfall_push_device_fmt(wf.h, 1, packed.ctypes.data, CH) == -1 and L.hd_waterfall_push_device_fmt(None, 1, dp.data_ptr(), CH) == -1
    rows, seg = np.ones((2, N), np.float32), np.array([16, 16], np.uint32)
    assert L.hd_waterfall_push_rows(None, rows.ctypes.data, seg.ctypes.data, 2, 0) == -1
    assert L.hd_waterfall_push_rows(wf.h, None, seg.ctypes.data, 2, 0) == -1 and L.hd_waterfall_push_rows(wf.h, rows.ctypes.data, None, 2, 0) == -1
    assert L.hd_waterfall_push_rows(wf.h, rows.ctypes.data, seg.ctypes.data, 2, 1) == -1          # host memory offered as device memory
    for bad in (0, 65):
        assert L.hd_waterfall_push_rows(wf.h, rows.ctypes.data, np.array([16, bad], np.uint32).ctypes.data, 2, 0) == -1
    assert L.hd_waterfall_reset(None) == -1 and L.hd_waterfall_rows_total(None) == 0
    assert wf.rows_total() == 0 and int(wf.hits()[1]) == 0                                        # nothing above was counted
    out_h, out_m, out_r = np.zeros(2, capi.WATERFALL_ROW_DTYPE), np.zeros((2, 128), np.uint32), np.zeros((2, N), np.float32)
    assert L.hd_waterfall_headers(wf.h, 0, 1, out_h.ctypes.data) == -1 and L.hd_waterfall_marks(wf.h, 0, 1, out_m.ctypes.data) == -1
    assert L.hd_waterfall_rows(wf.h, 0, 1, out_r.ctypes.data) == -1
    wf.push_device(d.data_ptr() + 8, N + 15 * HOP)                                                # 8-byte aligned is enough; one row
    assert wf.rows_total() == 1
    assert L.hd_waterfall_headers(wf.h, 0, 1, None) == -1 and L.hd_waterfall_marks(wf.h, 0, 1, None) == -1 and L.hd_waterfall_rows(wf.h, 0, 1, None) == -1
    assert L.hd_waterfall_headers(None, 0, 1, out_h.ctypes.data) == -1 and L.hd_waterfall_headers(wf.h, 1, 1, out_h.ctypes.data) == -1
    assert L.hd_waterfall_headers(wf.h, 0, 2, out_h.ctypes.data) == -1 and L.hd_waterfall_headers(wf.h, 1, 0, out_h.ctypes.data) == 0
    hits, k = np.zeros(N, np.uint32), C.c_uint64(0)
    assert L.hd_waterfall_hits(None, hits.ctypes.data, C.byref(k)) == -1 and L.hd_waterfall_hits(wf.h, None, C.byref(k)) == -1
    assert L.hd_waterfall_hits(wf.h, hits.ctypes.data, None) == 0 and hits.sum() == wf.headers()["n_marked"][0] > 0
    tp = capi.hd_waterfall_track_params()
    L.hd_waterfall_track_params_default(C.byref(tp))
    out, found = (capi.hd_waterfall_track * 4)(), C.c_uint32(9)
    assert L.hd_waterfall_tracks(None, C.byref(tp), out, 4, C.byref(found)) == -1 and found.value == 0
    assert L.hd_waterfall_tracks(wf.h, C.byref(tp), out, 4, None) == -1 and L.hd_waterfall_tracks(wf.h, C.byref(tp), None, 4, C.byref(found)) == -1
    assert L.hd_waterfall_tracks(wf.h, None, out, 4, C.byref(found)) == 0 and found.value == 0   # null parameters: the defaults (min_rows = 3: nothing yet)
    tp.min_rows = 1
    assert L.hd_waterfall_tracks(wf.h, C.byref(tp), out, 4, C.byref(found)) == 0 and found.value == 1 and abs(out[0].offset_hz - 123456.7) <= 500
    tp.merge_hz = -1.0
    assert L.hd_waterfall_tracks(wf.h, C.byref(tp), out, 4, C.byref(found)) == -1
    want = state(wf)
    wf.close()
    L.hd_waterfall_destroy(None)
    # an engine that computes no spectra holds no twiddles: the waterfall brings its own, and makes the same rows
    bare = hd.Engine(n_streams=1, sampling_rate=FS, decimation=64, enable_spectrum=False)
    wb = bare.waterfall()
    wb.push_device(d.data_ptr() + 8, N + 15 * HOP)
    assert same_state(state(wb), want)
    bare.close()
