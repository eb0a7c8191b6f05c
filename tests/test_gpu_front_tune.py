"""Per-stream tuning at the INPUT rate, in front of the first decimation stage (hd_stream_set_front_tune, include/habdec_amd.h).

Defining property: a front-tuned stream fed x is, in every float and every decoded character, a stream without front tuning fed the rotated x, call by
call.  The model is therefore the unmodified oracle at the engine's factor fed the numpy-rotated input, with the phase accumulated here; where back
tuning or the automatic AFC is on as well, the model of tests/test_gpu_tune.py (oracle decimation -> numpy rotation -> oracle back half) is fed the
rotated input instead.  Exact mode: bit-identical floats.  Fast mode: the project's 1e-5 norm-wise bound on the decimated samples, identical decisions."""
import math

import numpy as np
import pytest

import test_gpu_tune as back
from habdec_amd import synth

pytestmark = pytest.mark.gpu

CH = 65536


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def pyoracle():
    from oracle import pyoracle
    return pyoracle


def _tables():
    c = np.array([[math.cos(2 * math.pi * a / 256), math.sin(2 * math.pi * a / 256)] for a in range(256)], np.float32)
    f = np.array([[math.cos(2 * math.pi * b / 65536), math.sin(2 * math.pi * b / 65536)] for b in range(256)], np.float32)
    return c, f


TAB_C, TAB_F = _tables()


def rotate(x, phase, step):
    theta = (np.uint64(phase) + np.arange(len(x), dtype=np.uint64) * np.uint64(step)) & np.uint64(0xFFFFFFFF)
    a, b = (theta >> np.uint64(24)).astype(np.int64), ((theta >> np.uint64(16)) & np.uint64(255)).astype(np.int64)
    cr, ci, fr, fi = TAB_C[a, 0], TAB_C[a, 1], TAB_F[b, 0], TAB_F[b, 1]
    pr, pi = cr * fr - ci * fi, cr * fi + ci * fr
    xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
    out = np.empty(len(x), np.complex64)
    out.real, out.imag = xr * pr - xi * pi, xr * pi + xi * pr
    return out


def step_of(f, rate):
    return int(np.int64(np.round(-(f / rate) * 4294967296.0))) & 0xFFFFFFFF


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def normwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return np.inf
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


class Front:
    """One stream: the front rotation in numpy (phase accumulated here) in front of `dec` -- an oracle Decoder at the engine's factor, or a
    test_gpu_tune.Model where the stream is tuned at the decimated rate as well."""

    def __init__(self, dec, fs):
        self.dec, self.fs, self.step, self.phase, self.fed = dec, fs, 0, 0, False

    def set_front(self, f):
        self.step = step_of(f, self.fs)
        if f == 0:
            self.phase = 0

    def call(self, k, x, lag=1):
        self.fed = len(x) > 0
        if not self.fed:
            if isinstance(self.dec, back.Model):
                self.dec.call(k, x, lag)
            return
        xr = rotate(x, self.phase, self.step) if (self.step or self.phase) else x
        self.phase = (self.phase + len(x) * self.step) & 0xFFFFFFFF
        if isinstance(self.dec, back.Model):
            self.dec.call(k, xr, lag)
        else:
            self.dec(xr, self.fs)

    # what the engine's getters are compared with
    @property
    def chain(self):
        return self.dec.B if isinstance(self.dec, back.Model) else self.dec

    def decimated(self):
        return self.dec.rotated if isinstance(self.dec, back.Model) else self.dec.array("last_decimated")


def process(eng, slab, n_per_stream):
    n = np.ascontiguousarray(n_per_stream, np.uint32)
    slab = np.ascontiguousarray(slab, np.complex64)
    from habdec_amd.capi import check
    check(eng.L.hd_process_host(eng.h, slab.ctypes.data, slab.shape[1], n.ctypes.data, 0))


def run_front(hd, pyoracle, iq, fs, factor, pushes, front, *, tune=None, dc=False, pipeline=0, arith=0, per_call=True, ungated=False, auto=None,
              path=None, lag=1):
    """iq [S, N]; pushes: per-call sample counts (a number or one per stream); front / tune: {call: {stream: Hz}} set before that call (input rate /
    decimated rate); auto: {stream: (hold_s, min_hz)}; path: {call: expected hd_timing.path}.  Returns (engine, models)."""
    S = iq.shape[0]
    tune = tune or {}
    eng = hd.Engine(n_streams=S, max_chunk=max(int(np.max(p)) for p in pushes), sampling_rate=fs, decimation=factor, dc_remove=dc, keep_filtered=True,
                    pipeline=pipeline, arith=arith, ungated=ungated)
    with_back = bool(tune) or bool(auto)
    models = []
    for s in range(S):
        dec = back.Model(pyoracle, fs, factor, dc=dc, ungated=ungated) if with_back else \
            pyoracle.Decoder("oracle", factor=factor, dc_remove=dc, mathh_context=1, ungated=ungated)
        models.append(Front(dec, fs))
    for s, (hold, mn) in (auto or {}).items():
        eng.set_auto_afc(s, True, hold, mn)
        models[s].dec.auto, models[s].dec.hold, models[s].dec.min_hz = True, hold, mn
    pos = np.zeros(S, np.int64)
    for k, n in enumerate(pushes):
        n = np.broadcast_to(np.asarray(n, np.int64), (S,))
        for s, f in front.get(k, {}).items():
            eng.set_front_tune(s, f)
            models[s].set_front(f)
        for s, f in tune.get(k, {}).items():
            eng.set_tune(s, f)
            models[s].dec.set_tune(f)
        slab = np.zeros((S, max(int(n.max()), 1)), np.complex64)
        for s in range(S):
            slab[s, :n[s]] = iq[s, pos[s]:pos[s] + n[s]]
        process(eng, slab, n)
        for s in range(S):
            models[s].call(k, slab[s, :n[s]], lag)
            pos[s] += n[s]
        if path is not None and k in path:
            assert eng.timing()["path"] == path[k], (k, eng.timing()["path"], path[k])
        if any(m.step or m.phase for m in models):
            assert eng.timing()["path"] in (0, 2) and eng.timing()["step_variant"] == 0, (k, eng.timing())
        for s in range(S):
            ft = eng.front_tune(s)
            assert (ft["phase"], ft["step"]) == (models[s].phase, models[s].step), ("front phase / step", k, s, ft, models[s].phase, models[s].step)
        if not per_call:
            continue
        for s in range(S):
            m = models[s]
            if not n[s]:
                continue
            if arith == 0:
                assert same_bits(eng.decimated(s), m.decimated()), ("decimated", k, s)
                assert same_bits(eng.filtered(s), m.chain.array("last_filtered")), ("filtered", k, s)
                assert same_bits(eng.demodulated(s), m.chain.array("last_demod")), ("demod", k, s)
            else:
                err = normwise(eng.decimated(s), m.decimated())
                assert err <= 1e-5, ("decimated", k, s, err)
            assert np.array_equal(eng.bits(s), m.chain.bits()), ("bits", k, s)
    eng.flush()
    for s in range(S):
        m = models[s]
        assert eng.take_chars(s) == m.chain.text("chars_log"), ("chars", s)
        assert eng.take_sentences(s) == m.chain.sentences(), ("sentences", s)
    return eng, models


def signals(S, fs, f0s, *, n, sigma=0.06, seed0=0, texts=None):
    texts = texts or [synth.make_sentence(f"FRONT{s}", f"{s + 1},52.{100 + s},21.{400 + s}") for s in range(S)]
    out = np.zeros((S, n), np.complex64)
    for s in range(S):
        out[s] = synth.fsk_iq(synth.rtty_bits(texts[s], 8, 2, 6 + 3 * s, 10), fs, 300, sigma=sigma, seed=seed0 + s, n_samples=n, f0=f0s[s])
    return out


# ---- 1. every first-stage shape: total factor -> (input rate, push); the rates of the tuning tests' PARITY table, 32 kHz decimated elsewhere
SHAPES = {2: (64e3, 8192), 4: (128e3, 8192), 8: (256e3, 8192), 16: (2.5e6, 8192), 32: (1.024e6, 8192), 64: (2.048e6, CH), 128: (2.048e6, CH),
          256: (2.048e6, CH)}


@pytest.mark.parametrize("factor", list(SHAPES))
def test_parity_per_first_stage_shape(hd, pyoracle, factor):
    """Stream 0 untuned (= the oracle on the raw input), stream 1 at +fs/8 + 0.37 Hz and -fs/5 from the middle call, stream 2 at -0.31 fs and back to 0
    at the middle call (from then on the oracle on raw input, continued from the rotated history)."""
    fs, push = SHAPES[factor]
    n_calls = 10
    f1 = fs / 8 + 0.37
    iq = signals(3, fs, [300.0, f1 + 200.0, -0.31 * fs - 100.0], n=n_calls * push, seed0=factor)
    front = {0: {1: f1, 2: -0.31 * fs}, n_calls // 2: {1: -fs / 5, 2: 0.0}}
    eng, models = run_front(hd, pyoracle, iq, fs, factor, [push] * n_calls, front, ungated=fs / factor > 160e3)
    assert models[0].step == 0 and models[0].phase == 0 and models[2].phase == 0 and models[1].phase != 0
    assert eng.front_tune(1)["from_call"] == n_calls // 2 and eng.front_tune(1)["offset_hz"] == -fs / 5


# ---- 2. ragged pushes and idle streams (the D64_ragged table of the tuning tests)
def test_ragged_pushes_and_idle_streams(hd, pyoracle):
    fs = 2.048e6
    pushes = back.PARITY["D64_ragged"]["pushes"]
    total = sum(int(np.max(p)) for p in pushes)
    iq = signals(4, fs, [300.0, fs / 8 + 300.0, -0.31 * fs, 250e3 - 500.0], n=total, seed0=21)
    front = {0: {1: fs / 8 + 0.37, 2: -0.31 * fs, 3: 250e3}, len(pushes) // 2: {1: -fs / 5, 2: 0.0}}
    run_front(hd, pyoracle, iq, fs, 64, pushes, front)


# ---- 3. pushes so short that the stage-1 history carry holds outputs
def test_short_pushes(hd, pyoracle):
    fs = 2.048e6
    pushes = [[2176, 4288, 3200]] * 40 + [[4288, 2176, 2176]] * 40
    total = sum(int(np.max(p)) for p in pushes)
    iq = signals(3, fs, [fs / 8 + 300.0, -0.31 * fs, 250e3], n=total, seed0=31)
    front = {0: {0: fs / 8 + 0.37, 1: -0.31 * fs, 2: 250e3}, 40: {1: 417e3}}
    run_front(hd, pyoracle, iq, fs, 64, pushes, front)


# ---- 4. front and back tuning together; with the DC blocker on
@pytest.mark.parametrize("dc,path", [(False, 2), (True, 0)], ids=["tail", "dc"])
def test_front_and_back_tuning_together(hd, pyoracle, dc, path):
    fs, n_calls = 2.048e6, 10
    iq = signals(3, fs, [300.0, 250e3 + 2500.0, -600e3 - 4000.0], n=n_calls * CH, seed0=41)
    front = {0: {1: 250e3, 2: -600e3}, 5: {2: -601e3}}
    tune = {0: {0: 300.0, 1: 2500.5, 2: -4000.0}, 5: {1: -300.0, 2: -3000.0}}
    eng, models = run_front(hd, pyoracle, iq, fs, 64, [CH] * n_calls, front, tune=tune, dc=dc, path={k: path for k in range(n_calls)})
    for s in range(3):
        t = eng.tune(s)
        assert (t["phase"], t["step"]) == (models[s].dec.phase, models[s].dec.step), (s, t)


# ---- 5. the automatic AFC behind a front offset
def test_auto_afc_behind_a_front_offset(hd, pyoracle):
    """Payload at +250 kHz + 2 kHz, front tune +250 kHz, auto AFC with hold_s = 1: retuned by about +2 kHz exactly when the model is (the decimated-rate
    offset only), and what is sent after the retune decodes.  Stream 1: the same payload at +2 kHz without a front offset."""
    fs, n_calls = 2.048e6, 62
    texts = ["".join(synth.make_sentence(f"A{s}", str(i)) for i in range(8)) for s in range(2)]
    iq = signals(2, fs, [252e3, 2000.0], n=n_calls * CH, texts=texts, sigma=0.03, seed0=51)
    eng, models = run_front(hd, pyoracle, iq, fs, 64, [CH] * n_calls, {0: {0: 250e3}}, per_call=False, auto={0: (1.0, 100.0), 1: (1.0, 100.0)})
    for s in range(2):
        t, m = eng.tune(s), models[s].dec
        assert len(m.retunes) >= 1 and t["retunes"] == len(m.retunes), (s, t, m.retunes)
        assert t["from_call"] == m.retunes[-1][1] and t["offset_hz"] == pytest.approx(m.retunes[-1][2], abs=1e-9), (s, t, m.retunes)
        assert m.retunes[0][2] == pytest.approx(2000.0, abs=40), m.retunes
        assert all(first - d == 1 for d, first, _ in m.retunes)
        first = m.retunes[0][1]
        bits_per = 11 * len(synth.make_sentence(f"A{s}", "0"))
        want = [i for i in range(8) if (6 + 3 * s + bits_per * i) / 300 * fs / CH >= first and (6 + 3 * s + bits_per * (i + 1)) / 300 * fs / CH <= n_calls - 3]
        assert want and [x.split(",")[1].split("*")[0] for x in m.B.sentences()] == [str(i) for i in want], (s, want, m.B.sentences())
    assert eng.front_tune(0)["offset_hz"] == 250e3 and eng.front_tune(0)["step"] == step_of(250e3, fs) and eng.front_tune(1)["step"] == 0


# ---- 6. fast mode
@pytest.mark.parametrize("factor", [64, 16])
def test_fast_mode(hd, pyoracle, factor):
    fs, push = SHAPES[factor]
    n_calls = 10
    iq = signals(3, fs, [300.0, fs / 8 + 300.0, -0.31 * fs - 100.0], n=n_calls * push, seed0=60 + factor)
    front = {0: {1: fs / 8 + 0.37, 2: -0.31 * fs}, n_calls // 2: {1: -fs / 5, 2: 0.0}}
    run_front(hd, pyoracle, iq, fs, factor, [push] * n_calls, front, arith=1)


# ---- 7. batch mode: leaving and re-entering the step route
def test_batch_mode_leaves_and_reenters_the_step_route(hd, pyoracle):
    fs, n_calls, S = 2.048e6, 40, 4
    texts = [synth.make_sentence(f"B{s}", "0") + synth.make_sentence(f"B{s}", "1") for s in range(S)]
    iq = signals(S, fs, [0.0, 250e3, -600e3 + 200.0, 0.0], n=n_calls * CH, texts=texts, seed0=71)
    # (stream 1 is front-tuned for calls 6-11 only, stream 2 from call 6 to the end of its tuning at call 12: their payloads do not decode; 0 and 3 do)
    front = {6: {1: 250e3, 2: -600e3}, 12: {1: 0.0, 2: 0.0}}
    path = {k: 3 for k in list(range(6)) + list(range(12, n_calls))}
    eng, models = run_front(hd, pyoracle, iq, fs, 64, [CH] * n_calls, front, pipeline=2, per_call=False, path=path)
    # (run_front asserted path in (0, 2) and step_variant 0 for calls 6-11)
    for s in range(S):
        o = pyoracle.Decoder("oracle", factor=64, mathh_context=1)
        m = Front(o, fs)
        want = 0xCBF29CE484222325
        for k in range(n_calls):
            for s2, f in front.get(k, {}).items():
                if s2 == s:
                    m.set_front(f)
            m.call(k, iq[s, k * CH:(k + 1) * CH])
            d = o.array("last_demod").view(np.uint32).astype(np.uint64)
            for x in (len(d), int(d.sum() & 0xFFFFFFFF), int((d * np.arange(1, len(d) + 1, dtype=np.uint64)).sum() & 0xFFFFFFFF)):
                want = ((want ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        ncalls, unknown, h = eng.demod_checksum_total(s)
        assert (ncalls, unknown) == (n_calls, 0), ("every call delivered once", s, ncalls, unknown)
        assert h == want, ("discriminator output of some call differs", s)
    assert len(models[0].chain.sentences()) >= 1 and len(models[3].chain.sentences()) >= 1


# ---- 8. inert
@pytest.mark.parametrize("pipeline", [0, 2])
def test_inert_front_tuning_is_bit_identical_and_keeps_the_path(hd, pipeline):
    fs, n_calls = 2.048e6, 40
    iq = signals(1, fs, [200.0], n=n_calls * CH, texts=[synth.make_sentence("T", "1") * 2])
    iq = np.repeat(iq, 2, axis=0)
    ref = hd.Engine(n_streams=2, sampling_rate=fs, decimation=64, keep_filtered=True, pipeline=pipeline)
    eng = hd.Engine(n_streams=2, sampling_rate=fs, decimation=64, keep_filtered=True, pipeline=pipeline)
    eng.set_front_tune(1, 0.0)
    for k in range(n_calls):
        chunk = np.ascontiguousarray(iq[:, k * CH:(k + 1) * CH])
        ref.process_host(chunk)
        eng.process_host(chunk)
        assert (eng.timing()["path"], eng.timing()["step_variant"]) == (ref.timing()["path"], ref.timing()["step_variant"]), k
        assert eng.front_tune(1)["step"] == 0 and eng.front_tune(1)["phase"] == 0
        if pipeline and k != n_calls - 1:
            continue
        for get in ("decimated", "filtered", "demodulated", "bits"):
            assert same_bits(getattr(eng, get)(1), getattr(eng, get)(0)), (get, k)
            assert same_bits(getattr(eng, get)(1), getattr(ref, get)(1)), (get, k)
    assert eng.timing()["path"] == (3 if pipeline else 2)
    for s in range(2):
        assert eng.demod_checksum_total(s) == ref.demod_checksum_total(s) and eng.demod_checksum_total(s)[0] == n_calls
    got = [eng.take_sentences(0), eng.take_sentences(1), ref.take_sentences(0), ref.take_sentences(1)]
    assert got[0] == got[1] == got[2] == got[3] and len(got[0]) == 2, got


# ---- 9. what it is for
FAN = dict(fs=2.048e6, n_calls=56, offsets=[-600e3, 250e3, 5e3], calls=["WIDEA", "WIDEB", "WIDEC"], noise=0.05)


def fan_recording():
    fs, n = FAN["fs"], FAN["n_calls"] * CH
    texts = ["".join(synth.make_sentence(c, str(i)) for i in range(3)) for c in FAN["calls"]]
    rec = np.zeros(n, np.complex128)
    for j, (f, t) in enumerate(zip(FAN["offsets"], texts)):
        rec += synth.fsk_iq(synth.rtty_bits(t, 8, 2, 6 + 3 * j, 10), fs, 300, sigma=0.0, seed=j, n_samples=n, f0=f)
    nz = synth._noise(n, 7)
    return (rec + FAN["noise"] * (nz[0::2] + 1j * nz[1::2])).astype(np.complex64), texts


def test_one_wideband_recording_feeds_three_payloads(hd):
    """One 2.048 MS/s recording with payloads at -600 kHz, +250 kHz and +5 kHz, read by four streams from device memory with stream_stride = 0: each
    front-tuned stream decodes its own callsign's sentences and nothing else, the untuned one nothing -- and the decimated-rate tuning cannot reach them.
    (The oracle alone, on the rotated recording, decodes the first two of each payload's three sentences at this noise level; the third stays in the text
    stage until more text follows.)"""
    import torch
    fs, n_calls = FAN["fs"], FAN["n_calls"]
    rec, texts = fan_recording()
    dev = torch.from_numpy(rec.view(np.float32).copy()).cuda()
    eng = hd.Engine(n_streams=4, sampling_rate=fs, decimation=64)
    with pytest.raises(hd.HabdecError, match="error -1"):
        eng.set_tune(1, 250e3)
    for s, f in enumerate(FAN["offsets"]):
        eng.set_front_tune(s, f)
    for k in range(n_calls):
        eng.process_device(dev.data_ptr() + k * CH * 8, 0, CH)
    assert eng.timing()["path"] == 2 and eng.timing()["step_variant"] == 0
    got = [eng.take_sentences(s) for s in range(4)]
    for s in range(3):
        want = [t.strip().lstrip("$") for t in texts[s].split("\n") if t][:2]
        assert got[s] == want, (s, got[s], want)
    assert got[3] == []
    assert eng.front_tune(3)["step"] == 0 and eng.front_tune(0)["step"] == step_of(-600e3, fs)


# ---- 10. errors
def test_errors(hd):
    from habdec_amd.capi import lib
    fs = 2.048e6
    eng = hd.Engine(n_streams=2, sampling_rate=fs, decimation=64)
    for f in (fs / 2, -fs / 2, 1.5e6, float("nan")):
        assert eng.L.hd_stream_set_front_tune(eng.h, 0, f) == -1, f          # HD_ERR_INVALID
    assert b"fs/2" in lib().hd_last_error()
    assert eng.L.hd_stream_set_front_tune(eng.h, 2, 1000.0) == -1           # bad stream index
    import ctypes as C
    from habdec_amd import capi
    info = capi.hd_front_tune_info()
    assert eng.L.hd_stream_front_tune(eng.h, 2, C.byref(info)) == -1
    assert eng.L.hd_stream_front_tune(eng.h, 0, None) == -1
    eng.set_front_tune(0, fs / 2 - 1.0)
    assert eng.front_tune(0) == {"offset_hz": fs / 2 - 1.0, "step": step_of(fs / 2 - 1.0, fs), "phase": 0, "from_call": 0}
    one = hd.Engine(n_streams=1, max_chunk=2048, sampling_rate=32e3, decimation=1)
    assert one.L.hd_stream_set_front_tune(one.h, 0, 100.0) == -3            # HD_ERR_UNSUPPORTED
    assert one.L.hd_stream_set_front_tune(one.h, 0, 0.0) == -3
