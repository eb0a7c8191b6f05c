"""Packed IQ (cs16 / cs8 / cu8) through hd_process_*_fmt, hd_survey_push_*_fmt and hd_ingest_run on the GPU.

Defining property: a packed push is, float for float, the cf32 push of hd_host_iq_convert's output.  Every comparison here is therefore BYTE equality
against a second engine fed the converted floats through the existing cf32 call -- no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from habdec_amd import capi, synth
from iq_formats_util import FMTS, all_codes, convert, quantise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def u32p(n):
    return None if n is None else n.ctypes.data_as(C.POINTER(C.c_uint32))


class Feeder:
    """Hands a packed buffer (flat [N, 2] codes, first sample of stream 0 at `off`) to hd_process_*_fmt from pageable memory, from hd_pinned_alloc
    memory or from device memory; keeps what the pointer refers to alive."""

    def __init__(self, eng, source, torch):
        self.eng, self.source, self.torch, self.keep = eng, source, torch, []

    def push(self, fmt, buf, off, stride, n_per_stream, n_uniform):
        code, dt, bps = FMTS[fmt]
        buf = np.ascontiguousarray(buf, dtype=dt)
        n = None if n_per_stream is None else np.ascontiguousarray(n_per_stream, np.uint32)
        L, h = self.eng.L, self.eng.h
        if self.source == "pageable":
            return L.hd_process_host_fmt(h, code, buf.ctypes.data + off * bps, stride, u32p(n), n_uniform)
        if self.source == "pinned":
            pin = self.eng.pinned_array(buf.shape, dt)
            pin[...] = buf
            return L.hd_process_host_fmt(h, code, pin.ctypes.data + off * bps, stride, u32p(n), n_uniform)
        dev = self.torch.from_numpy(buf.copy()).cuda()
        self.keep.append(dev)
        return L.hd_process_device_fmt(h, code, dev.data_ptr() + off * bps, stride, u32p(n), n_uniform)


def push_cf32(eng, slab, stride, n_per_stream, n_uniform):
    slab = np.ascontiguousarray(slab, np.complex64)
    n = None if n_per_stream is None else np.ascontiguousarray(n_per_stream, np.uint32)
    return eng.L.hd_process_host(eng.h, slab.ctypes.data, stride, u32p(n), n_uniform)


def random_codes(fmt, n, seed):
    info = np.iinfo(FMTS[fmt][1])
    return np.random.default_rng(seed).integers(info.min, info.max + 1, size=(n, 2)).astype(FMTS[fmt][1])


# ---- 1. codes and alignment
@pytest.mark.parametrize("source", ["pageable", "pinned", "device"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_every_code_and_every_alignment(hd, torch, fmt, source):
    """decimation = 1: hd_stream_decimated IS the converted push.  One push with every code of the format in I and in Q; then five streams with the odd
    source stride 1031, the base one and three samples into the buffer, n_per_stream = [1031, 0, 1030, 257, the smallest count the engine accepts] --
    behind two full pushes that left every sample of both staging slabs non-zero, so that a stream reading what a longer push left behind, or a row
    written past its count into its neighbour, shows in `decimated`."""
    codes = all_codes(fmt)
    N = len(codes)
    one, ref = (hd.Engine(n_streams=1, max_chunk=N, sampling_rate=32e3, decimation=1) for _ in range(2))
    assert Feeder(one, source, torch).push(fmt, codes, 0, N, None, N) == 0, capi.lib().hd_last_error()
    want = convert(fmt, codes)
    assert push_cf32(ref, want, N, None, N) == 0
    assert same(one.decimated(0), want) and same(one.decimated(0), ref.decimated(0))
    if source == "pinned":
        assert one.timing()["host_calls_in_place"] == 1
    one.close(); ref.close()

    S, stride, M = 5, 1031, 1032
    n_min = capi.lib().hd_min_chunk(1)
    assert n_min >= 1
    eng, ref = (hd.Engine(n_streams=S, max_chunk=M, sampling_rate=32e3, decimation=1) for _ in range(2))
    feed = Feeder(eng, source, torch)
    ragged = [1031, 0, 1030, 257, n_min]
    for k, (off, n) in enumerate([(0, [1031] * S), (0, [1031] * S), (1, ragged), (3, ragged), (1, [8, 1031, 0, n_min, 1030]), (3, [1031] * S)]):
        buf = random_codes(fmt, off + S * stride + 1, 100 + k)
        assert feed.push(fmt, buf, off, stride, np.array(n, np.uint32), 0) == 0, (k, capi.lib().hd_last_error())
        floats = convert(fmt, buf[off:off + S * stride]).reshape(S, stride)
        slab = np.zeros((S, M), np.complex64)
        slab[:, :stride] = floats
        assert push_cf32(ref, slab, M, np.array(n, np.uint32), 0) == 0
        for s in range(S):
            got = eng.decimated(s)
            assert same(got, ref.decimated(s)), (k, s)
            if n[s]:
                assert same(got, floats[s, :n[s]]), (k, s)
    if source == "pinned":
        assert eng.timing()["host_calls_in_place"] == 6
    eng.close(); ref.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_unpack_reads_and_writes_nothing_outside_its_rows(hd, torch, fmt):
    """The kernel alone, into a buffer of sentinels: source rows at every offset a row may have against a 16-byte boundary (0 .. 8 samples), destination
    rows 16-byte aligned and 8 bytes off, odd strides, counts that end in the head, in a vector and in the tail -- every sample in front of a row's
    count is the converted one, and every other float of the destination still holds the sentinel."""
    code, dt, bps = FMTS[fmt]
    eng = hd.Engine(n_streams=1, max_chunk=2048, sampling_rate=32e3, decimation=1)
    fn = eng.L.hd_debug_iq_unpack_timed
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                        C.POINTER(C.c_float)]
    counts = [1031, 0, 1030, 257, 1, 7, 8, 9, 15, 16, 17, 2, 3, 300, 513]
    rows, sstride, dstride = len(counts), 1031, 1037
    ms = C.c_float(0)
    sentinel = np.uint32(0x7FC12345)
    for off in range(0, 9):
        for doff in (0, 1):
            buf = random_codes(fmt, off + rows * sstride, 7 * off + doff)
            src = torch.from_numpy(buf).cuda()
            d_n = torch.from_numpy(np.array(counts, np.int32)).cuda()
            dst = torch.from_numpy(np.full((doff + rows * dstride + 8) * 2, sentinel, np.uint32).view(np.int32)).cuda()
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
            rc = fn(eng.h, code, src.data_ptr() + off * bps, sstride, d_n.data_ptr(), 0, max(counts), rows, dst.data_ptr() + doff * 8, dstride, C.byref(ms))
            assert rc == 0, capi.lib().hd_last_error()
            out = dst.cpu().numpy().view(np.uint32).reshape(-1, 2)
            want = np.full_like(out, sentinel)
            for r, n in enumerate(counts):
                want[doff + r * dstride: doff + r * dstride + n] = convert(fmt, buf[off + r * sstride: off + r * sstride + n]).view(np.uint32).reshape(-1, 2)
            bad = np.argwhere(out != want)
            assert not len(bad), (off, doff, bad[:4])
    # the uniform count and the shared row (stride 0 on both sides is one row)
    buf = random_codes(fmt, 4099, 1)
    src = torch.from_numpy(buf).cuda()
    dst = torch.from_numpy(np.full(4200 * 2, sentinel, np.uint32).view(np.int32)).cuda()
    assert fn(eng.h, code, src.data_ptr() + bps, 0, None, 4097, 4097, 1, dst.data_ptr(), 0, C.byref(ms)) == 0
    out = dst.cpu().numpy().view(np.uint32).reshape(-1, 2)
    assert same(out[:4097], convert(fmt, buf[1:4098]).view(np.uint32).reshape(-1, 2)) and np.all(out[4097:] == sentinel)
    eng.close()


# ---- 2. routes
# /64, 50 baud 7N2, 64 streams, 4096-sample pushes.  The input rate is the lowest at which the chain still has 8 samples per bit behind the /64
# (25.6 kS/s: 400 S/s decimated, shift 100 Hz, low-pass 150 Hz), so that a push carries 8 bits: two sentences per stream, which the oracle must decode
# before anything is compared, need 48 pushes, and the first spectrum (4096 decimated samples) completes in the 64th -- 66 pushes, not six (six pushes of
# 4096 samples hold 48 bits at this rate: not one sentence, and no spectrum).  The signal is the synthetic generator's at half of full scale (amplitude 0.5).
R = dict(S=64, fs=25600.0, n=4096, calls=66, baud=50, bits=7, stops=2, shift=100.0, bw=150.0)


@pytest.fixture(scope="module")
def route_floats():
    S, n = R["S"], R["n"] * R["calls"]
    out = np.zeros((S, n), np.complex64)
    for s in range(S):
        text = synth.make_sentence(f"P{s}", str(s % 10)) * 3
        out[s] = synth.fsk_iq(synth.rtty_bits(text, R["bits"], R["stops"], 2 + s % 5, 4), R["fs"], R["baud"], shift=R["shift"], sigma=0.04, seed=300 + s,
                              n_samples=n)
    return out


@pytest.fixture(scope="module")
def route_inputs(route_floats):
    """fmt -> (packed [S, N, 2], converted floats [S, N]); the oracle, fed the converted floats, decodes at least two sentences of every stream."""
    from oracle import pyoracle
    cache = {}

    def get(fmt):
        if fmt not in cache:
            packed = quantise(fmt, route_floats)
            floats = convert(fmt, packed)
            for s in range(R["S"]):
                o = pyoracle.Decoder("oracle", factor=64, baud=R["baud"], bits=R["bits"], stops=R["stops"], lowpass_bw=R["bw"])
                for k in range(R["calls"]):
                    o(floats[s, k * R["n"]:(k + 1) * R["n"]], R["fs"])
                assert len(o.sentences()) >= 2, (fmt, s, o.sentences(), o.text("chars_log"))
            cache[fmt] = (packed, floats)
        return cache[fmt]
    return get


ROUTES = {
    "sync": dict(cfg=dict(), path=(2, None)),
    "pipeline1": dict(cfg=dict(pipeline=1), path=(3, 1)),
    "pipeline2": dict(cfg=dict(pipeline=2), path=(3, 1)),
    # (/16 with pushes this short takes the stream tail like /64: the DC blocker is what sends a call through the separate kernels, path 0)
    "div16": dict(cfg=dict(decimation=16, dc_remove=True), path=(0, None)),
    "front_tuned": dict(cfg=dict(), path=(2, None), front={3: 1000.0, 7: -2500.0}),
    "fast": dict(cfg=dict(arith=1), path=(2, None)),
}
ROUTE_CASES = [(r, f) for r in ROUTES if r != "fast" for f in FMTS] + [("fast", "cs16")]


def snapshot(eng, S, full):
    out = []
    for s in range(S):
        a = eng.afc(s)
        row = [eng.bits(s).tobytes(), eng.demod_checksum_total(s), eng.demod_checksum(s), eng.take_chars(s), tuple(eng.take_sentences(s)),
               tuple(sorted(a.items())), eng.bits_total(s)]
        if full:
            row += [eng.decimated(s).tobytes(), eng.demodulated(s).tobytes(), eng.spectrum(s).tobytes(), eng.power(s).tobytes()]
        out.append(row)
    return out


@pytest.mark.parametrize("route,fmt", ROUTE_CASES)
def test_every_route_runs_a_packed_push_like_the_cf32_push(hd, route_inputs, route, fmt):
    packed, floats = route_inputs(fmt)
    S, n, calls = R["S"], R["n"], R["calls"]
    spec = ROUTES[route]
    cfg = dict(n_streams=S, max_chunk=n, sampling_rate=R["fs"], decimation=64, baud=R["baud"], rtty_bits=R["bits"], rtty_stops=R["stops"],
               lowpass_bw_hz=R["bw"])
    cfg.update(spec["cfg"])
    eng, ref = hd.Engine(**cfg), hd.Engine(**cfg)
    for s, f in spec.get("front", {}).items():
        eng.set_front_tune(s, f); ref.set_front_tune(s, f)
    pipelined = bool(cfg.get("pipeline"))
    sentences = [0] * S
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(packed[:, k * n:(k + 1) * n]))
        ref.process_host(np.ascontiguousarray(floats[:, k * n:(k + 1) * n]))
        t, tr = eng.timing(), ref.timing()
        assert (t["path"], t["step_variant"]) == (tr["path"], tr["step_variant"]), (k, t, tr)
        assert t["path"] == spec["path"][0], (k, t)
        if spec["path"][1] is not None and k >= 1:
            assert t["step_variant"] == spec["path"][1], (k, t)
        # batch mode: the getters that read device buffers drain the pipeline -- the delivered calls are compared through the ones that do not, and
        # everything at the end; the other routes: everything, every call
        full = not pipelined or k == calls - 1
        if full and pipelined:
            eng.flush(); ref.flush()
        a, b = snapshot(eng, S, full), snapshot(ref, S, full)
        for s in range(S):
            assert a[s] == b[s], (route, fmt, k, s, [i for i, (x, y) in enumerate(zip(a[s], b[s])) if x != y])
            sentences[s] += len(a[s][4])
    tuned = set(spec.get("front", {}))
    assert all(sentences[s] >= 2 for s in range(S) if s not in tuned), sentences
    assert eng.afc(0)["spectra"] >= 1 and len(eng.spectrum(0)) == 4096
    eng.close(); ref.close()


# ---- 3. fan-out
def test_one_cu8_capture_fans_out_to_four_front_tuned_streams(hd, torch):
    """The FAN recording of test_gpu_front_tune.py (payloads at -600 kHz, +250 kHz and +5 kHz in one 2.048 MS/s capture) as rtl_sdr would have written
    it, read from device memory with stream_stride = 0 by four front-tuned streams: converted ONCE into a shared row, and every stream's results are those
    of the cf32 engine on the converted capture."""
    import test_gpu_front_tune as ft
    fs, n_calls, CH = ft.FAN["fs"], ft.FAN["n_calls"], ft.CH
    rec, texts = ft.fan_recording()
    packed = quantise("cu8", rec * np.float32(0.25))                 # three carriers of amplitude 0.5 and the noise: a quarter keeps them inside full scale
    floats = convert("cu8", packed)
    dev_p, dev_f = torch.from_numpy(packed).cuda(), torch.from_numpy(floats.view(np.float32).copy()).cuda()
    eng, ref = hd.Engine(n_streams=4, sampling_rate=fs, decimation=64), hd.Engine(n_streams=4, sampling_rate=fs, decimation=64)
    for s, f in enumerate(ft.FAN["offsets"] + [100e3]):
        eng.set_front_tune(s, f); ref.set_front_tune(s, f)
    for k in range(n_calls):
        eng.process_device(dev_p.data_ptr() + k * CH * 2, 0, CH, fmt="cu8")
        ref.process_device(dev_f.data_ptr() + k * CH * 8, 0, CH)
        if k % 8 == 7 or k == n_calls - 1:
            for s in range(4):
                assert same(eng.decimated(s), ref.decimated(s)) and same(eng.demodulated(s), ref.demodulated(s)), (k, s)
    got = [eng.take_sentences(s) for s in range(4)]
    assert got == [ref.take_sentences(s) for s in range(4)]
    for s in range(3):
        assert len(got[s]) >= 1 and all(x.startswith(ft.FAN["calls"][s]) for x in got[s]), (s, got[s])
    assert got[3] == []
    for s in range(4):
        assert eng.demod_checksum_total(s) == ref.demod_checksum_total(s) and eng.demod_checksum_total(s)[0] == n_calls
    eng.close(); ref.close()


# ---- 4. ingest
def test_ingest_of_cs16_files_decodes_like_the_same_files_as_cf32(hd, tmp_path):
    fs, D, Ck, S = 256e3, 64, 8192, 8
    packed_paths, plain_paths = [], []
    for s in range(S):
        text = synth.make_sentence(f"ING{s}", f"{s},52.{s},21.{s}") * 2
        x = synth.fsk_iq(synth.rtty_bits(text, 8, 2, 4 + s, 6), fs, 300, seed=40 + s, sigma=0.05)
        x = x[:(len(x) // Ck) * Ck + (100 if s == 1 else 0 if s == 2 else 777 * s + 3000)]          # ragged, a whole number of chunks, a 100-sample tail
        codes = quantise("cs16", x)
        p, q = tmp_path / f"f{s}.cs16", tmp_path / f"f{s}.cf32"
        codes.tofile(p); convert("cs16", codes).tofile(q)
        packed_paths.append(p); plain_paths.append(q)
    eng, ref = (hd.Engine(n_streams=S, max_chunk=Ck, sampling_rate=fs, decimation=D, pipeline=1) for _ in range(2))
    done = eng.ingest(hd.IqFiles(packed_paths, chunk=Ck, granule=D, fmt="cs16"))
    assert done == ref.ingest(hd.IqFiles(plain_paths, chunk=Ck, granule=D)) and done > 0
    for s in range(S):
        want = ref.take_sentences(s)
        assert eng.take_sentences(s) == want and len(want) == 2, (s, want)
        assert eng.bits_total(s) == ref.bits_total(s) and eng.bits_total(s) > 0, s
        assert eng.demod_checksum_total(s) == ref.demod_checksum_total(s), s
        assert eng.take_chars(s) == ref.take_chars(s), s
    eng.close(); ref.close()


# ---- 5. survey
@pytest.mark.parametrize("n,runs", [(6144, None), (260 * 2048, None), (260 * 2048, 2)], ids=["2_segments", "259_segments", "259_segments_RUNS=2"])
def test_survey_of_cs8_pushes_is_the_survey_of_the_converted_floats(hd, torch, monkeypatch, n, runs):
    """(259 segments at the default run count: r = 1; at HD_SURVEY_RUNS=2: r = 64, a slab of four runs and one of one)"""
    if runs:
        monkeypatch.setenv("HD_SURVEY_RUNS", str(runs))        # (read when a survey is created)
    fs = 2.048e6
    k = np.arange(n)
    nz = synth._noise(n, 11)
    x = (0.3 * np.exp(2j * np.pi * 250e3 / fs * k) + 0.2 * np.exp(-2j * np.pi * 600e3 / fs * k) + 0.05 * (nz[0::2] + 1j * nz[1::2])).astype(np.complex64)
    packed = quantise("cs8", x)
    floats = convert("cs8", packed)
    eng = hd.Engine(n_streams=1, sampling_rate=fs, decimation=64)
    ref, host, dev = eng.survey(), eng.survey(), eng.survey()
    ref.push_host(floats)
    host.push_host(packed, fmt="cs8")
    d = torch.from_numpy(packed).cuda()
    dev.push_device(d.data_ptr(), n, fmt="cs8")
    want, segs = ref.power()
    assert segs == n // 2048 - 1 and np.all(want > 0)
    for sv in (host, dev):
        got, got_segs = sv.power()
        assert got_segs == segs and same(got, want)
    if segs >= 16:
        cands = ref.detect()
        assert len(cands) >= 2 and host.detect() == cands and dev.detect() == cands
    # a second push on top (the accumulators go on), from a base that is no multiple of 16 bytes
    ref.push_host(floats[3:]); host.push_host(packed[3:], fmt="cs8"); dev.push_device(d.data_ptr() + 3 * 2, n - 3, fmt="cs8")
    want, _ = ref.power()
    assert same(host.power()[0], want) and same(dev.power()[0], want)
    eng.close()


# ---- 6. errors
def test_refused_calls_return_their_codes_and_leave_the_engine_untouched(hd):
    fs, M = 32e3, 4096
    text = synth.make_sentence("ERR", "1,2,3") * 3            # (the last sentence stays in the text stage until more text follows)
    x = synth.fsk_iq(synth.rtty_bits(text, 8, 2, 4, 6), fs, 300, sigma=0.02, seed=3)
    x = x[:len(x) // M * M]
    packed = quantise("cs16", x)
    eng, ref = (hd.Engine(n_streams=1, max_chunk=M, sampling_rate=fs, decimation=1) for _ in range(2))
    L = eng.L
    inside = []
    buf0 = np.ascontiguousarray(packed[:M])

    def on_chars(user, s, p, n):
        inside.append(L.hd_process_host_fmt(eng.h, 1, buf0.ctypes.data, M, None, M))
    cb = capi.CHARS_CB(on_chars)
    L.hd_set_chars_callback(eng.h, cb, None)
    sv = eng.survey()
    for k in range(len(packed) // M):
        buf = np.ascontiguousarray(packed[k * M:(k + 1) * M])
        assert L.hd_process_host_fmt(eng.h, 7, buf.ctypes.data, M, None, M) == -1                       # unknown fmt: HD_ERR_INVALID
        assert b"format" in capi.lib().hd_last_error()
        assert L.hd_process_device_fmt(eng.h, -1, buf.ctypes.data, M, None, M) == -1
        assert L.hd_process_host_fmt(eng.h, 1, None, M, None, M) == -1                                  # null pointer
        assert L.hd_process_device_fmt(eng.h, 3, None, M, None, M) == -1
        assert L.hd_process_host_fmt(eng.h, 1, buf.ctypes.data + 2, M, None, 8) == -1                   # a cs16 base off its 4-byte boundary
        assert L.hd_process_host_fmt(eng.h, 1, buf.ctypes.data, M, None, M + 1) == -4                   # n > max_chunk: HD_ERR_CAPACITY
        assert L.hd_process_host_fmt(eng.h, 2, buf.ctypes.data, M, np.array([M + 64], np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), 0) == -4
        assert L.hd_survey_push_host_fmt(sv.h, 9, buf.ctypes.data, M) == -1 and L.hd_survey_push_device_fmt(sv.h, 1, None, M) == -1
        eng.process_host(buf)                                                                           # the valid call
        ref.process_host(buf)
        assert same(eng.decimated(0), ref.decimated(0)) and same(eng.demodulated(0), ref.demodulated(0)), k
        assert eng.demod_checksum_total(0) == ref.demod_checksum_total(0) and eng.demod_checksum_total(0)[0] == k + 1
    assert inside and all(rc == -1 for rc in inside)                                                    # from inside a callback: HD_ERR_INVALID
    want = ref.take_sentences(0)
    assert eng.take_sentences(0) == want and len(want) >= 1
    assert eng.take_chars(0) == ref.take_chars(0)
    eng.close(); ref.close()
