"""Signals that stop: samples that are EXACTLY zero (a muted receiver, a file padded with zeros) in the middle of a transmission, in the engine's fast
arithmetic mode (hd_engine_config.arith = HD_ARITH_FAST) and, as the control that shows the scenario sound, in the exact mode -- through the C ABI, one
pyoracle.Decoder per stream fed the same pushes, keep_filtered.

The fast mode promises the reference's decisions (bits, characters, sentences) and floats within 1e-5 norm-wise.  Where the reference's numbers are exactly
zero a norm-wise gate says nothing (bench.demod_excess divides by max(|y|, 1e-30): anything passes), and two places of the fast mode could leave the
reference there without any other test noticing:

  1. the cheap window sums of the symbol extractor (kernels/sym_common.h window_sums_shared: k_symbols and the stream tail): a window of zeros must sum to
     +0 exactly, as std::accumulate does -- sgnf has three values, so a rounding residue of 1e-9 is another flag than 0;
  2. the long low-pass through transforms (engine.cpp lowpass_transforms): a block [history | inputs] that mixes signal and exact zeros comes back from the
     transforms with ~1e-6 of the input's peak where the direct sum is 0, and the discriminator turns that floor into arbitrary phases.

One construction for every case.  Stream s < 16 carries sentence A, a span of exact zeros, sentence B; the span begins inside A's last call at input index
z0 + s D (D = the decimation factor: the onset moves by ONE decimated sample from stream to stream, sixteen consecutive alignments = two periods of the
HD_SYM_POS = 8 positions a lane owns, and whole periods of a build with 4), runs through one whole call and ends inside B's first call.  Stream 16 is zeros
from sample 0 up to the same end, stream 17 has seven zero samples inside A's characters, stream 18 has no zeros at all.

  case  shape                                                  route asserted
  a     /64, 2.048 MS/s, 161-tap low-pass                      the stream tail (timing path 2)
  b     /16, 2.5 MS/s, low-pass 3 kHz                          the separate kernels: k_fir_demod + k_symbols (path 0)
  c     /4 ungated, 2.048 MS/s, a few calls                    k_symbols at the long windows: bits and backlog only (the sentences are cut short)
  d     /1, 48 kS/s, 1025 and 4097 taps, HD_NO_LP_FFT=1        direct sums (lowpass_fft_calls == 0)
  e     as d without the variable, fast mode only              the transforms (lowpass_fft_calls > 0, a block mixing zeros and signal among them)

The step kernel (batch mode) runs its stream tails through kernels/tail_body.h, the code case a runs: it has no case of its own.

Per call and stream, fast mode: bits and symbol backlog the oracle's; decimated and filtered floats within test_gpu_fast.run_fast's 1e-5 norm-wise gates (in
an all-zero call that forces exact zeros); where the oracle's filtered y[i] and y[i-1] are both exactly 0 the engine's filtered sample compares equal to 0
and its discriminator output has the oracle's BYTES (a filtered zero of the other sign is printed, not failed: what must hold is the discriminator);
elsewhere bench.demod_excess <= 1.  At the end the text stream, the characters and the sentences are the oracle's.  Exact mode: decimated, filtered and
discriminator floats bit-identical, bits, backlog and text equal.

The inputs are checked against the oracle alone before the GPU is touched (reference(): every stream with a silent span has a call whose filtered output
is exactly 0 throughout, and decodes the sentence sent after the span).

Beside the silence cases, test_fast_mode_window_sums_at_short_symbols (eight cases) runs the shapes of window_sums_shared that no other fast-mode test
reaches -- windows shorter than the eight positions a lane owns, a core of no sample and of two -- on continuous FSK, with test_gpu_fast.run_fast's gates
(floats within 1e-5, bits, backlog and text the oracle's): no zeros there, so the sharper checks above have nothing to bite on."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from habdec_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-5
C = 65536
N_ONSETS = 16                       # silent streams 0..15: consecutive decimated-sample alignments of the onset
S_FROM_ZERO, S_SEVEN, S_CONTROL = N_ONSETS, N_ONSETS + 1, N_ONSETS + 2
S = N_ONSETS + 3
SILENT = list(range(N_ONSETS + 1))  # the streams with a span of zeros

SHAPES = {
    "D64": dict(fs=2.048e6, factor=64, chunk=C, lp_taps=161),
    "D16_lp3k": dict(fs=2.5e6, factor=16, chunk=C, lowpass_bw=3000.0, lp_taps=161),
    "D4_ungated": dict(fs=2.048e6, factor=4, chunk=C, ungated=True, lp_taps=161, calls_per_text=4),
    "D1_1025": dict(fs=48000.0, factor=1, chunk=8192, lp_taps=1025),
    "D1_4097": dict(fs=48000.0, factor=1, chunk=8192, lp_taps=4097),
}
BAUD, BITS, STOPS = 300, 8, 2


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    yield habdec_amd
    reference.cache_clear()          # the shapes' inputs and oracle outputs (about 1 GB together) are shared by this module's tests and go with it


def lp_trans(shape):
    from test_gpu_long_lowpass import tw_for
    T = SHAPES[shape]["lp_taps"]
    return tw_for(T) if T != 161 else None


def make_inputs(shape):
    """(iq [S, ncalls * chunk], meta): [A | one call of idle or zeros | B] per stream, the zero spans as the module docstring states them."""
    from test_gpu_parity import make_streams
    c = SHAPES[shape]
    fs, D, chunk = c["fs"], c["factor"], c["chunk"]
    spb = fs / BAUD
    # B is followed by seven more characters: the symbol extractor releases a run of equal bits at the next flip, and idle has none; and the text stage
    # looks for a sentence once it holds more than 20 characters (the stream that starts from zeros holds nothing but B's)
    texts = [(synth.make_sentence(f"A{s:02d}", "1"), synth.make_sentence(f"B{s:02d}", "2,5") + ".......") for s in range(S)]
    frame = 1 + BITS + STOPS
    m = chunk // D
    delay = (c["lp_taps"] + 64) * D                                  # what the filters hold back, generously
    in_call = (m // 8) * D + 5                                       # the first onset's place in its call: not on a decimated sample's boundary
    if "calls_per_text" in c:                                        # (case c: the sentences are cut short)
        kz, nB = c["calls_per_text"] - 2, c["calls_per_text"]
    else:
        # make_streams puts 6 idle bits in front of a lone stream's text and 10 behind it
        kz = int(np.ceil(((6 + frame * max(len(a) for a, _ in texts) + 2) * spb + delay - in_call) / chunk))       # the call of the onsets: A is over
        nB = int(np.ceil(((6 + frame * max(len(b) for _, b in texts) + 10) * spb + delay) / chunk))
    nA = kz + 2                                                      # ... and the call the silent streams spend in zeros
    ncalls = nA + nB
    iq = np.zeros((S, ncalls * chunk), np.complex64)

    def render(s):
        for which, (n0, n) in enumerate([(0, nA * chunk), (nA * chunk, nB * chunk)]):
            x, _ = make_streams(1, fs, BAUD, BITS, STOPS, int(np.ceil(n / C)), seed0=1000 + 2 * s + which, texts=[texts[s][which]], repeat=1)
            iq[s, n0:n0 + n] = x[0, :n]

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(render, range(S)))
    z0 = kz * chunk + in_call
    z1 = nA * chunk + min(100 * D + 3, int(1.5 * spb))              # inside B's first call: at least four of B's six idle bits are left
    onsets = [z0 + s * D for s in range(N_ONSETS)]
    for s in range(N_ONSETS):
        iq[s, onsets[s]:z1] = 0
    iq[S_FROM_ZERO, :z1] = 0
    seven = int(20.3 * spb)                                          # inside A's second character
    iq[S_SEVEN, seven:seven + 7] = 0
    assert onsets[0] // chunk == onsets[-1] // chunk == nA - 2 and z1 // chunk == nA and seven + 7 < (6 + 11 * len(texts[0][0])) * spb
    assert np.all(iq[SILENT, (nA - 1) * chunk:nA * chunk] == 0) and not np.any(iq[S_CONTROL] == 0)
    return iq, dict(texts=texts, ncalls=ncalls, nA=nA, onsets=onsets, z1=z1, m=m, truncated="calls_per_text" in c)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """The inputs of a shape and what the oracle makes of them, computed once and left unchanged: per call and stream (decimated, filtered, discriminator
    output, bits, backlog), and the text at the end.  Asserts, on the oracle alone, that the inputs are the scenario the tests are about."""
    from oracle import pyoracle
    c = SHAPES[shape]
    fs, chunk = c["fs"], c["chunk"]
    iq, meta = make_inputs(shape)
    kw = {k: c[k] for k in ("lowpass_bw", "ungated") if k in c}
    if lp_trans(shape) is not None:
        kw["lowpass_trans"] = lp_trans(shape)

    def one_stream(s):          # (the decoders are independent and the oracle runs outside the interpreter's lock: one thread per stream, at most 16)
        o = pyoracle.Decoder("oracle", factor=c["factor"], baud=BAUD, bits=BITS, stops=STOPS, **kw)
        col = []
        for k in range(meta["ncalls"]):
            o(iq[s, k * chunk:(k + 1) * chunk], fs)
            col.append(dict(dec=o.array("last_decimated"), filt=o.array("last_filtered"), demod=o.array("last_demod"), bits=o.bits(), held=o.symex_held()))
        assert len(o.array("fir_taps")) == c["lp_taps"]
        return col, dict(rtty=o.text("rtty_stream"), chars=o.text("chars_log"), sentences=o.sentences())

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        cols = list(pool.map(one_stream, range(S)))
    calls = [[cols[s][0][k] for s in range(S)] for k in range(meta["ncalls"])]
    end = [cols[s][1] for s in range(S)]
    for s in SILENT:
        zero_calls = [k for k in range(meta["ncalls"]) if calls[k][s]["filt"].size == meta["m"] and not np.any(calls[k][s]["filt"])]
        assert zero_calls, ("no call in which the oracle's filtered output is exactly zero throughout", shape, s)
        after = sum(len(calls[k][s]["bits"]) for k in range(meta["nA"], meta["ncalls"]))
        assert after > 0, ("no bits behind the silence", shape, s)
        if not meta["truncated"]:
            body = meta["texts"][s][1][2:].split("*")[0]
            assert any(body in x for x in end[s]["sentences"]), ("the oracle does not decode the sentence sent after the silence", shape, s, end[s])
    assert not any(np.any(calls[k][S_CONTROL]["filt"] == 0) for k in range(meta["ncalls"]))
    if not meta["truncated"]:
        assert len(end[S_CONTROL]["sentences"]) == 2 and len(end[S_SEVEN]["sentences"]) >= 1, end[S_CONTROL]
    return iq, meta, calls, end


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def zero_zero(fo, prev):
    """Indices i with y[i] == 0 and y[i-1] == 0 in the oracle's filtered output, y[-1] carried over from the previous call (None: no such sample yet)."""
    z = fo == 0
    zp = np.concatenate([[prev is not None and prev == 0], z[:-1]])
    return z & zp


def run_case(hd, shape, arith, *, path, floats=True):
    """The engine in the given arithmetic and the recorded oracle over the same pushes, every check of the module docstring on every call and stream.
    Returns (engine, the low-pass transform calls whose block mixed zeros and signal, the indices checked at zero per stream)."""
    import bench
    c = SHAPES[shape]
    fs, chunk, T = c["fs"], c["chunk"], c["lp_taps"]
    iq, meta, calls, end = reference(shape)
    kw = {}
    if lp_trans(shape) is not None:
        kw["lowpass_trans"] = lp_trans(shape)
    eng = hd.Engine(n_streams=S, max_chunk=chunk, sampling_rate=fs, decimation=c["factor"], baud=BAUD, rtty_bits=BITS, rtty_stops=STOPS,
                    lowpass_bw_hz=c.get("lowpass_bw", 1500.0), ungated=c.get("ungated", False), keep_filtered=floats, arith=arith, **kw)
    prev = [None] * S
    hist = [np.zeros(0, np.complex64)] * S       # the oracle's decimated samples so far: the low-pass's history
    at_zero = [0] * S
    sign_only = []
    mixed_fft_calls, fft_before = 0, 0
    for k in range(meta["ncalls"]):
        eng.process_host(np.ascontiguousarray(iq[:, k * chunk:(k + 1) * chunk]))
        fft_now = eng.timing()["lowpass_fft_calls"]
        mixed = False
        for s in range(S):
            o = calls[k][s]
            if floats:
                block = np.concatenate([hist[s][-(T - 1):], o["dec"]])
                mixed |= bool(np.any(block == 0) and np.any(block != 0))
                hist[s] = block
                gdec, gf, gd = eng.decimated(s), eng.filtered(s), eng.demodulated(s)
                fo, od = o["filt"], o["demod"]
                if arith == 0:
                    assert same_bits(gdec, o["dec"]), ("decimated", k, s)
                    assert same_bits(gf, fo), ("filtered", k, s)
                    assert same_bits(gd, od), ("demod", k, s)
                else:
                    nd, nf = bench.normwise(gdec, o["dec"]), bench.fir_normwise(gf, fo, o["dec"])
                    assert nd <= TOL and nf <= TOL, ("floats", k, s, nd, nf)
                    zz = zero_zero(fo, prev[s])
                    at_zero[s] += int(np.count_nonzero(zz))
                    assert np.all(gf[zz] == 0), ("filtered sample not zero where the reference's is", k, s, int(np.count_nonzero(gf[zz] != 0)),
                                                 float(np.max(np.abs(gf[zz]))))
                    flipped = zz & ((gf.view(np.uint32).reshape(-1, 2) != fo.view(np.uint32).reshape(-1, 2)).any(axis=1))
                    if flipped.any():
                        sign_only.append((k, s, int(np.count_nonzero(flipped)), int(np.flatnonzero(flipped)[0])))
                    bad = zz & (gd.view(np.uint32) != od.view(np.uint32))
                    assert not bad.any(), ("discriminator output differs where the reference filtered zeros", k, s, int(np.count_nonzero(bad)),
                                           int(np.flatnonzero(bad)[0]), gd[bad][:4], od[bad][:4])
                    ex, ab = bench.demod_excess(np.where(zz, od, gd), od, fo, prev[s], TOL, scale=float(np.max(np.abs(o["dec"]))) if o["dec"].size else None)
                    assert ex <= 1.0, ("discriminator output beyond the propagated bound", k, s, ex, ab)
                if fo.size:
                    prev[s] = fo[-1]
            assert np.array_equal(eng.bits(s), o["bits"]), ("bits", k, s, eng.bits(s).tolist(), o["bits"].tolist())
            assert eng.symbol_backlog(s) == o["held"], ("backlog", k, s, eng.symbol_backlog(s), o["held"])
        if fft_now > fft_before and mixed:
            mixed_fft_calls += 1
        fft_before = fft_now
    if sign_only:
        print("filtered zeros of the other sign (call, stream, count, first index):", sign_only)
    print(shape, "arith", arith, "indices checked at zero per stream:", at_zero, "timing", eng.timing())
    assert eng.timing()["path"] == path, eng.timing()
    if floats and arith:
        assert all(at_zero[s] >= meta["m"] for s in SILENT), ("fewer zero-after-zero outputs than one call's worth", at_zero)
    for s in range(S):
        assert eng.rtty(s) == end[s]["rtty"], ("rtty", s, eng.rtty(s), end[s]["rtty"])
        assert eng.take_chars(s) == end[s]["chars"], ("chars", s)
        assert eng.take_sentences(s) == end[s]["sentences"], ("sentences", s)
    return eng, mixed_fft_calls, at_zero


@pytest.mark.parametrize("arith", [0, 1])
def test_a_silence_through_the_stream_tail(hd, arith):
    """/64, 161-tap low-pass: stage 2, low-pass, discriminator and the symbol extractor in one wave per stream (tail_body.h; the step kernel runs the same code)."""
    run_case(hd, "D64", arith, path=2)[0].close()


@pytest.mark.parametrize("arith", [0, 1])
def test_b_silence_through_the_separate_kernels(hd, arith):
    """/16 at 2.5 MS/s, 3 kHz low-pass: k_fir_demod and k_symbols."""
    run_case(hd, "D16_lp3k", arith, path=0)[0].close()


@pytest.mark.parametrize("arith", [0, 1])
def test_c_silence_at_the_long_windows(hd, arith):
    """/4 ungated: windows of 427 samples per lane in k_symbols, four calls of each sentence (cut short): bits and backlog."""
    run_case(hd, "D4_ungated", arith, path=0, floats=False)[0].close()


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("shape", ["D1_1025", "D1_4097"])
def test_d_silence_through_long_direct_sums(hd, monkeypatch, shape, arith):
    """/1 at 48 kS/s, a low-pass of 1025 and of 4097 taps as direct sums (HD_NO_LP_FFT=1 keeps the fast mode off the transforms)."""
    monkeypatch.setenv("HD_NO_LP_FFT", "1")
    eng, _, _ = run_case(hd, shape, arith, path=0)
    assert len(eng.fir_taps(0)) == SHAPES[shape]["lp_taps"] and eng.timing()["lowpass_fft_calls"] == 0, eng.timing()
    eng.close()


@pytest.mark.parametrize("shape", ["D1_1025", "D1_4097"])
def test_e_silence_through_the_transform_route(hd, monkeypatch, shape):
    """The same streams with the long low-pass through transforms (fast mode's default from 1024 taps on).  A stream whose block [history | inputs]
    holds a run of samples that are exactly zero is given direct sums for that call (k_lp_gather flags it, k_fir_demod sums it instead of taking the transforms'
    rows), so every check of cases a to d holds here too -- and the launches in question did go through the transforms: the control stream's and
    stream 17's rows of the same calls are theirs."""
    monkeypatch.delenv("HD_NO_LP_FFT", raising=False)
    eng, mixed_fft_calls, _ = run_case(hd, shape, 1, path=0)
    t = eng.timing()
    assert len(eng.fir_taps(0)) == SHAPES[shape]["lp_taps"] and t["lowpass_fft_calls"] > 0, t
    assert mixed_fft_calls >= 2, ("no transform call whose block mixed zeros and signal", mixed_fft_calls, t)      # (the onset's call and the end's)
    eng.close()


@pytest.mark.parametrize("path", ["tail", "separate"])
@pytest.mark.parametrize("baud", [2000, 1200, 900, 750])
def test_fast_mode_window_sums_at_short_symbols(hd, monkeypatch, baud, path):
    """The shapes of window_sums_shared that no other fast-mode test reaches (32 kHz, symbols of 16 .. 43 samples: R = 4, 6, 8, 10): windows shorter than the
    eight positions a lane owns (each summed on its own), a core of no sample (R = 8) and of two (R = 10) -- test_gpu_parity's exact-mode case of the same
    name in fast mode, with test_gpu_fast.run_fast's gates: floats within 1e-5, bits, backlog and text the oracle's."""
    from test_gpu_fast import run_fast
    from test_gpu_parity import make_streams
    if path == "separate":
        monkeypatch.setenv("HD_NO_TAIL", "1")
    fs = 2.048e6
    iq, _ = make_streams(2, fs, baud, 8, 2, seed0=300 + baud, repeat=3)
    eng, orcs, worst = run_fast(hd, iq, fs, factor=64, baud=baud, bits=8, stops=2, lowpass_bw=5000.0, expect_path=2 if path == "tail" else 0)
    assert worst["filtered_n"] > 0 and sum(len(o.text("chars_log")) for o in orcs) > 20
    eng.close()
