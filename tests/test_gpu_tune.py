"""Per-stream digital tuning and closed-loop AFC on the GPU (hd_stream_set_tune / hd_stream_set_auto_afc, include/habdec_amd.h).

The model of a tuned stream is built from the unmodified oracle: A decimates (and removes DC) at the engine's factor, the chunk A leaves is rotated in
numpy float32 with the engine's tables, and B -- the oracle at factor 1, fed at the decimated rate with the same chunk sizes -- runs the back half.
In exact mode every float of a tuned stream is then bit-identical to the model's, as untuned streams are to the oracle."""
import ctypes as C
import math

import numpy as np
import pytest

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


def step_of(f, fsd):
    return int(np.int64(np.round(-(f / fsd) * 4294967296.0))) & 0xFFFFFFFF


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


class Model:
    """One tuned stream: oracle decimation (+DC) -> numpy rotation -> oracle back half at factor 1; the auto-AFC rule on B's AFC state."""

    def __init__(self, pyoracle, fs, factor, dc=False, baud=300, bits=8, stops=2, lowpass_bw=None, ungated=False):
        self.fs, self.fsd = fs, fs / factor
        kw = dict(baud=baud, bits=bits, stops=stops, lowpass_bw=lowpass_bw, mathh_context=1, ungated=ungated)
        self.A = pyoracle.Decoder("oracle", factor=factor, dc_remove=dc, with_fft=False, **kw)
        self.B = pyoracle.Decoder("oracle", factor=1, dc_remove=False, **kw)
        self.f, self.step, self.phase = 0.0, 0, 0
        self.pending = []                          # (first call, offset) of retunes not in effect yet
        self.auto, self.hold, self.min_hz, self.elapsed, self.retunes = False, 6.0, 100.0, 0, []
        self.rotated = np.zeros(0, np.complex64)

    def set_tune(self, f):
        self.f, self.step = f, step_of(f, self.fsd)
        if f == 0:
            self.phase = 0

    def call(self, k, x, lag=1):
        """Call k with input x; returns True when the call delivered something (n > 0).  `lag`: calls between a delivery and the call its retune reaches."""
        for first, f in list(self.pending):
            if first <= k:
                self.f, self.step = f, step_of(f, self.fsd)
                self.pending.remove((first, f))
        if len(x) == 0:
            self.rotated = np.zeros(0, np.complex64)
            return
        self.A(x, self.fs)
        d = self.A.array("last_decimated")
        r = rotate(d, self.phase, self.step) if self.step else d
        self.phase = (self.phase + len(d) * self.step) & 0xFFFFFFFF
        self.rotated = r
        self.B(r, self.fsd)
        self.elapsed += len(x)
        corr = self.B.afc()["correction"]
        if self.auto and self.elapsed >= self.hold * self.fs and abs(corr) > self.min_hz:
            target = (self.pending[-1][1] if self.pending else self.f) + corr
            if abs(target) < self.fsd / 2:
                self.pending.append((k + lag, target))
                self.B.reset_correction(corr)
                self.elapsed = 0
                self.retunes.append((k, k + lag, target))


def process(eng, slab, n_per_stream, stride=None):
    n = np.ascontiguousarray(n_per_stream, np.uint32)
    slab = np.ascontiguousarray(slab, np.complex64)
    stride = slab.shape[1] if stride is None else stride
    from habdec_amd.capi import check
    check(eng.L.hd_process_host(eng.h, slab.ctypes.data, stride, n.ctypes.data, 0))


def run_tuned(hd, pyoracle, iq, fs, factor, pushes, offsets, *, dc=False, pipeline=0, arith=0, per_call=True, path=None, lowpass_bw=None,
              ungated=False, auto=None):
    """iq [S, N]; pushes: list of per-stream sample counts per call; offsets: {call: {stream: Hz}} applied before that call;
    auto: {stream: (hold_s, min_hz)}.  Returns (engine, models)."""
    S = iq.shape[0]
    eng = hd.Engine(n_streams=S, max_chunk=max(int(np.max(p)) for p in pushes), sampling_rate=fs, decimation=factor, dc_remove=dc,
                    keep_filtered=True, pipeline=pipeline, arith=arith, ungated=ungated,
                    lowpass_bw_hz=lowpass_bw if lowpass_bw is not None else 1500.0)
    models = [Model(pyoracle, fs, factor, dc=dc, lowpass_bw=lowpass_bw, ungated=ungated) for _ in range(S)]
    for s, (hold, mn) in (auto or {}).items():
        eng.set_auto_afc(s, True, hold, mn)
        models[s].auto, models[s].hold, models[s].min_hz = True, hold, mn
    pos = np.zeros(S, np.int64)
    step_path = pipeline >= 1 and path == 3
    lag = 1 if pipeline == 0 else (4 if (step_path and pipeline >= 2) else 3)
    for k, n in enumerate(pushes):
        n = np.broadcast_to(np.asarray(n, np.int64), (S,))
        for s, f in offsets.get(k, {}).items():
            eng.set_tune(s, f)
            models[s].set_tune(f)
        slab = np.zeros((S, max(int(n.max()), 1)), np.complex64)
        for s in range(S):
            slab[s, :n[s]] = iq[s, pos[s]:pos[s] + n[s]]
        process(eng, slab, n)
        for s in range(S):
            models[s].call(k, slab[s, :n[s]], lag)
            pos[s] += n[s]
        if path is not None:
            assert eng.timing()["path"] == path, (k, eng.timing()["path"], path)
        if not per_call:
            continue
        for s in range(S):
            m = models[s]
            assert eng.tune(s)["phase"] == m.phase, ("phase", k, s)
            if not n[s]:
                continue
            if arith == 0:
                assert same_bits(eng.decimated(s), m.rotated), ("decimated", k, s)
                assert same_bits(eng.filtered(s), m.B.array("last_filtered")), ("filtered", k, s)
                assert same_bits(eng.demodulated(s), m.B.array("last_demod")), ("demod", k, s)
                assert np.array_equal(eng.bits(s), m.B.bits()), ("bits", k, s)
                ga, oa = eng.afc(s), m.B.afc()
                assert (ga["peak_l"], ga["peak_r"]) == (oa["peak_l"], oa["peak_r"]), ("peaks", k, s, ga, oa)
                for key in ("correction", "shift_hz"):
                    assert ga[key] == pytest.approx(oa[key], rel=1e-9, abs=1e-9), (key, k, s)
            else:
                assert normwise(eng.decimated(s), m.rotated) <= 1e-5, ("decimated", k, s)
                gf, of = eng.filtered(s), m.B.array("last_filtered")     # (relative to the signal's peak: a stream tuned away from its payload filters to almost nothing)
                assert gf.shape == of.shape and (of.size == 0 or np.max(np.abs(gf - of)) <= 1e-5 * np.max(np.abs(m.rotated))), ("filtered", k, s)
    eng.flush()
    for s in range(S):
        m = models[s]
        assert eng.take_chars(s) == m.B.text("chars_log"), ("chars", s)
        assert eng.take_sentences(s) == m.B.sentences(), ("sentences", s)
        assert eng.tune(s)["phase"] == m.phase and eng.tune(s)["step"] == m.step, ("tune", s, eng.tune(s), m.phase, m.step)
        if arith == 0 and not per_call and int(np.asarray(pushes[-1]).max()):
            # (a free-running batch: the last call's floats, after the flush)
            assert same_bits(eng.decimated(s), m.rotated), ("last decimated", s)
            assert same_bits(eng.demodulated(s), m.B.array("last_demod")), ("last demod", s)
    return eng, models


def streams(S, fs, f0s, *, n, sigma=0.06, seed0=0, texts=None, repeat=3):
    texts = texts or [synth.make_sentence(f"TUNE{s}", f"{s + 1},52.{100 + s},21.{400 + s}") * repeat for s in range(S)]
    out = np.zeros((S, n), np.complex64)
    for s in range(S):
        b = synth.rtty_bits(texts[s], 8, 2, 6 + 3 * s, 10)
        out[s] = synth.fsk_iq(b, fs, 300, sigma=sigma, seed=seed0 + s, n_samples=n, f0=f0s[s])
    return out, texts


def test_inert_tuning_is_bit_identical_and_keeps_the_path(hd):
    """set_tune(0) and an auto AFC that never fires leave a stream bit-identical to an untouched one, on the untuned engine's path."""
    fs, n_calls = 2.048e6, 40
    iq, _ = streams(1, fs, [200.0], n=n_calls * CH, texts=[synth.make_sentence("T", "1") * 2])
    iq = np.repeat(iq, 2, axis=0)
    ref = hd.Engine(n_streams=2, sampling_rate=fs, decimation=64, keep_filtered=True)
    eng = hd.Engine(n_streams=2, sampling_rate=fs, decimation=64, keep_filtered=True)
    eng.set_tune(1, 0.0)
    eng.set_auto_afc(1, True, 0.0, 1e9)
    for k in range(n_calls):
        chunk = np.ascontiguousarray(iq[:, k * CH:(k + 1) * CH])
        ref.process_host(chunk)
        eng.process_host(chunk)
        assert eng.timing()["path"] == ref.timing()["path"]
        for get in ("decimated", "filtered", "demodulated", "bits"):
            assert same_bits(getattr(eng, get)(1), getattr(eng, get)(0)), (get, k)
            assert same_bits(getattr(eng, get)(1), getattr(ref, get)(1)), (get, k)
        assert eng.tune(1)["step"] == 0 and eng.tune(1)["phase"] == 0 and eng.tune(1)["retunes"] == 0
    got = [eng.take_sentences(0), eng.take_sentences(1), ref.take_sentences(0), ref.take_sentences(1)]
    assert got[0] == got[1] == got[2] == got[3] and len(got[0]) == 2, got


# offsets per stream across 0, +-300, +-2500.5, -4000 and fs_dec/2 - 1, some changed between calls
def _offsets(S, fsd, k_change):
    base = [0.0, 300.0, -2500.5, fsd / 2 - 1][:S]
    later = [-4000.0, -300.0, 2500.5, 0.0][:S]
    return {0: dict(enumerate(base)), k_change: dict(enumerate(later))}


PARITY = {
    # /64 at 2.048 MS/s, synchronous: the stream tail (path 2)
    "D64_tail": dict(fs=2.048e6, factor=64, S=4, pushes=[CH] * 10, pipeline=0, path=2),
    # /64, equal pushes, batch mode two deep: the step kernel (path 3), no flush in between
    "D64_step": dict(fs=2.048e6, factor=64, S=4, pushes=[CH] * 12, pipeline=2, path=3, per_call=False),
    # /16 at 2.5 MS/s: the fused back end declines tuned calls -> separate kernels (path 0)
    "D16_sep": dict(fs=2.5e6, factor=16, S=3, pushes=[CH] * 6, pipeline=0, path=0),
    # DC blocker on: separate kernels, blocker first, then the rotation
    "D64_dc": dict(fs=2.048e6, factor=64, S=3, pushes=[CH] * 8, pipeline=0, path=0, dc=True),
    # /8 at 256 kHz: a single-stage plan
    "D8_single": dict(fs=256e3, factor=8, S=3, pushes=[8192] * 12, pipeline=0, path=0),
    # factor 1
    "F1": dict(fs=32e3, factor=1, S=3, pushes=[2048] * 16, pipeline=0, path=0),
    # ragged pushes, idle streams
    "D64_ragged": dict(fs=2.048e6, factor=64, S=4, pushes=[[CH, 0, 32768, 4352], [0, CH, 4352, 32768], [32768, 4352, 0, CH], [CH, CH, CH, 0],
                                                           [4352, 0, CH, CH], [CH, 32768, 32768, 4352]] * 2, pipeline=0, path=None),
    # pushes of 2176..4288 samples at /64: n2 < T2 - 1, the stage-2 history carry holds outputs (Q4)
    "D64_short": dict(fs=2.048e6, factor=64, S=3, pushes=[[2176, 4288, 3200]] * 40 + [[4288, 2176, 2176]] * 40, pipeline=0, path=None),
}


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_model_on_every_call(hd, pyoracle, name):
    cfg = PARITY[name]
    fs, factor, S = cfg["fs"], cfg["factor"], cfg["S"]
    fsd = fs / factor
    pushes = cfg["pushes"]
    total = sum(int(np.max(p)) for p in pushes)
    f0s = [[300.0, -2500.0, 0.0, 1000.0][s % 4] * min(1.0, fsd / 32000.0) for s in range(S)]
    iq, _ = streams(S, fs, f0s, n=total, seed0=hash(name) % 1000, repeat=1)
    offs = _offsets(S, fsd, len(pushes) // 2)
    run_tuned(hd, pyoracle, iq, fs, factor, pushes, offs, dc=cfg.get("dc", False), pipeline=cfg["pipeline"], path=cfg["path"],
              per_call=cfg.get("per_call", True), ungated=fsd > 160e3)


@pytest.mark.parametrize("name", ["D64_tail", "D16_sep"])
def test_fast_mode_parity(hd, pyoracle, name):
    cfg = PARITY[name]
    fs, factor, S = cfg["fs"], cfg["factor"], cfg["S"]
    fsd = fs / factor
    total = sum(int(np.max(p)) for p in cfg["pushes"])
    iq, _ = streams(S, fs, [300.0, -2500.0, 1000.0, 0.0][:S], n=total, seed0=5, repeat=1)
    run_tuned(hd, pyoracle, iq, fs, factor, cfg["pushes"], _offsets(S, fsd, len(cfg["pushes"]) // 2), pipeline=cfg["pipeline"], path=cfg["path"], arith=1)


def test_off_centre_payload_decodes_only_when_tuned(hd):
    """A payload recorded +4 kHz off centre: the default low-pass (1500 Hz) leaves nothing untuned; tuned to +4000 Hz every sentence decodes."""
    fs, n_calls = 2.048e6, 60
    texts = [synth.make_sentence("OFF", str(i)) for i in range(3)]
    iq, _ = streams(1, fs, [4000.0], n=n_calls * CH, texts=["".join(texts)])
    iq = np.repeat(iq, 2, axis=0)
    eng = hd.Engine(n_streams=2, sampling_rate=fs, decimation=64)
    eng.set_tune(1, 4000.0)
    for k in range(n_calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * CH:(k + 1) * CH]))
    assert eng.timing()["path"] == 2
    assert eng.take_sentences(0) == []
    got = eng.take_sentences(1)
    # (all but the last sentence, which the text stage holds until more text follows)
    assert [g.split("*")[0] for g in got] == [t.strip().lstrip("$").split("*")[0] for t in texts[:-1]], got


@pytest.mark.parametrize("pipeline,path", [(0, 2), (2, 3)])
@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fast"])
def test_closed_loop_matches_the_model(hd, pyoracle, pipeline, path, arith):
    """Auto AFC with hold_s = 1: +2 kHz and -3.5 kHz payloads are retuned, +60 Hz (below min_hz) and noise are not; the retunes, offsets and the calls
    they reach equal the model's, and what is sent after the retune decodes."""
    fs, n_calls = 2.048e6, 62          # (one hold time past the first retune: no second one)
    texts = ["".join(synth.make_sentence(f"L{s}", str(i)) for i in range(8)) for s in range(3)] + ["$$X*"]
    iq, _ = streams(4, fs, [2000.0, -3500.0, 60.0, 0.0], n=n_calls * CH, texts=texts, sigma=0.03)
    iq[3] = (synth._noise(n_calls * CH, 99)[0::2] * 0.03).astype(np.complex64)
    eng, models = run_tuned(hd, pyoracle, iq, fs, 64, [CH] * n_calls, {}, pipeline=pipeline, path=path, arith=arith,
                            per_call=False, auto={s: (1.0, 100.0) for s in range(4)})
    for s in range(4):
        t, m = eng.tune(s), models[s]
        assert t["retunes"] == len(m.retunes), (s, t, m.retunes)
        if m.retunes:
            assert t["from_call"] == m.retunes[-1][1] and t["offset_hz"] == pytest.approx(m.retunes[-1][2], abs=1e-9), (s, t, m.retunes)
    assert len(models[0].retunes) >= 1 and len(models[1].retunes) >= 1 and models[2].retunes == [] and models[3].retunes == []
    assert models[0].retunes[0][2] == pytest.approx(2000.0, abs=40) and models[1].retunes[0][2] == pytest.approx(-3500.0, abs=40)
    lag = 1 if pipeline == 0 else 4
    assert all(first - d == lag for d, first, _ in models[0].retunes + models[1].retunes)
    for s in (0, 1):
        # every sentence sent wholly after the retune, and followed by a few calls for the framer, is decoded
        first = models[s].retunes[0][1]
        bits_per = 11 * len(synth.make_sentence(f"L{s}", "0"))
        want = [i for i in range(8) if (6 + 3 * s + bits_per * i) / 300 * fs / CH >= first and (6 + 3 * s + bits_per * (i + 1)) / 300 * fs / CH <= n_calls - 3]
        assert want and [x.split(",")[1].split("*")[0] for x in models[s].B.sentences()] == [str(i) for i in want], (s, want, models[s].B.sentences())
    assert len(models[2].B.sentences()) >= 3


def test_fan_out_of_one_recording_with_stride_zero(hd):
    """One recording, payloads at -6 kHz (A) and +5 kHz (B), read by four streams with stream_stride = 0 from device memory."""
    import torch
    fs, n_calls = 2.048e6, 56
    ta = "".join(synth.make_sentence("FANA", str(i)) for i in range(3))
    tb = "".join(synth.make_sentence("FANB", str(i)) for i in range(3))
    a, _ = streams(1, fs, [-6000.0], n=n_calls * CH, texts=[ta], sigma=0.0)
    b, _ = streams(1, fs, [5000.0], n=n_calls * CH, texts=[tb], sigma=0.0, seed0=3)
    rec = (a[0] + b[0] + 0.05 * (synth._noise(n_calls * CH, 7)[0::2] + 1j * synth._noise(n_calls * CH, 7)[1::2])).astype(np.complex64)
    dev = torch.from_numpy(rec.view(np.float32).copy()).cuda()
    eng = hd.Engine(n_streams=4, sampling_rate=fs, decimation=64, keep_filtered=True)
    for s, f in enumerate([-6000.0, 5000.0, 0.0, 5000.0]):
        eng.set_tune(s, f)
    for k in range(n_calls):
        eng.process_device(dev.data_ptr() + k * CH * 8, 0, CH)
        assert same_bits(eng.decimated(1), eng.decimated(3)) and same_bits(eng.demodulated(1), eng.demodulated(3)), k
    assert eng.timing()["path"] == 2
    got = [eng.take_sentences(s) for s in range(4)]
    assert len(got[0]) == 2 and all(x.startswith("FANA") for x in got[0]), got[0]
    assert len(got[1]) == 2 and all(x.startswith("FANB") for x in got[1]) and got[1] == got[3], got
    assert got[2] == []


def test_ingest_with_auto_afc(hd, pyoracle, tmp_path):
    """Two cf32 recordings with off-tune payloads through hd_ingest_run, auto AFC on: they are retuned and their sentences decode, as in the model."""
    fs, n_calls = 2.048e6, 80
    n = n_calls * CH
    texts = ["".join(synth.make_sentence(f"ING{s}", str(i)) for i in range(8)) for s in range(2)]
    iq, _ = streams(2, fs, [2500.0, -3000.0], n=n, texts=texts, sigma=0.03)
    paths = []
    for s in range(2):
        p = tmp_path / f"rec{s}.cf32"
        p.write_bytes(synth.to_iqfile_bytes(iq[s]))
        paths.append(p)
    eng = hd.Engine(n_streams=2, sampling_rate=fs, decimation=64, pipeline=1)
    for s in range(2):
        eng.set_auto_afc(s, True, 1.0, 100.0)
    files = hd.IqFiles(paths, chunk=CH, granule=64)
    assert eng.ingest(files) == 2 * n
    for s in range(2):
        m = Model(pyoracle, fs, 64)
        m.auto, m.hold, m.min_hz = True, 1.0, 100.0
        for k in range(n_calls):
            m.call(k, iq[s, k * CH:(k + 1) * CH], 3)      # (equal pushes, one call in flight: the step path delivers a call two calls later)
        t = eng.tune(s)
        assert m.retunes and abs(m.retunes[0][2] - [2500.0, -3000.0][s]) < 60, m.retunes
        assert t["retunes"] == len(m.retunes) and t["from_call"] == m.retunes[-1][1] and t["offset_hz"] == pytest.approx(m.retunes[-1][2], abs=1e-9), (t, m.retunes)
        got = eng.take_sentences(s)
        assert got == m.B.sentences() and len(got) >= 1 and all(x.startswith(f"ING{s}") for x in got), (got, m.B.sentences())
