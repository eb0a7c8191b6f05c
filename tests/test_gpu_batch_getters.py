"""Batch mode's data getters behind stream tails that no longer store what only a getter reads.

A batch-mode engine (`pipeline >= 1`) on a tail route (paths 2 and 3) leaves the discriminator output of a call in the symbol backlog ring only --
`hd_stream_demodulated` reads the newest `last_m` samples of the ring --, and its tails transform a completed 4096-sample buffer for the AFC
statistics without storing the spectrum and the power: `hd_stream_spectrum` / `hd_stream_power` transform the kept buffer again when asked
(`HD_EAGER_SPECTRA=1` stores them in every tail, as a synchronous engine does).

  1. `demodulated` from the ring equals the CPU oracle's `last_demod` bit for bit, for every stream, at the first calls, across the ring's wrap
     (the ring holds 32768 samples: 1024 per call, so call 33 starts at slot 0 again; with the position counters started elsewhere the wrap falls
     INSIDE a call and the read-out is two pieces), on the per-CU step kernel, on its single-wave fallback (an odd stream count, `HD_NO_CU_STEP`),
     with one and with two more calls in flight, across a switch to the separate kernels and back, and behind a ragged push (path 2).
  2. spectra on demand are the bytes a tail would have stored: a default and an `HD_EAGER_SPECTRA=1` engine and a synchronous one, fed the same
     calls, return identical `spectrum`, `power` and `afc` 0 to 3 calls behind a completed buffer and across the second completion.
  3. both in fast mode: engine against engine bit for bit, `demodulated` within `bench.demod_excess` of the oracle.

/64 plan, 2.048 MS/s, 50 baud, pushes of 65536 samples, synthetic FSK + noise.  The streams are copies of eight signals, so eight oracles serve all 64;
the oracle's arrays are computed once per module and not changed."""
import numpy as np
import pytest

from habdec_amd import synth

pytestmark = pytest.mark.gpu

FS, C, D, BAUD = 2.048e6, 65536, 64, 50
NSIG, S64, NCALLS = 8, 64, 34
KEEP = (1, 2, 3, 5, 33, 34)          # calls (1-based) behind which the reference keeps the oracle's arrays


def ring_cap(max_chunk, factor):
    """The engine's symbol ring for a configuration, as hd_engine_create sizes it: the power of two that holds the symbol extractor's vent limit
    (30000 samples), one low-pass batch capacity (the decimated push rounded up to 256, plus 256) and 1024 of slack."""
    m_cap = (max_chunk // factor + 255) // 256 * 256 + 256
    cap = 1
    while cap < 30000 + 1 + m_cap + 1024:
        cap <<= 1
    return cap


RING_CAP = ring_cap(C, D)
M = C // D                           # discriminator outputs per call and stream


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def oracle(**kw):
    from oracle import pyoracle
    return pyoracle.Decoder("oracle", factor=D, baud=BAUD, with_fft=False, **kw)


def snapshot(o, prev_last):
    """What the comparisons need of an oracle after a call (`prev_last`: the last filtered sample of the call before, for demod_excess)."""
    dec = o.array("last_decimated")
    return {"demod": o.array("last_demod"), "filtered": o.array("last_filtered"), "dec_peak": float(np.max(np.abs(dec))) if dec.size else None, "prev": prev_last}


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def signals():
    """[NSIG][NCALLS * C] complex64: 50-baud 8N2 FSK + noise, a sentence repeating, each signal with its own seed and start phase."""
    text = synth.make_sentence("GETTER", "1,52.0,21.0,100") * 8
    bits = synth.rtty_bits(text, 8, 2, 4, 4)
    out = np.stack([synth.fsk_iq(np.roll(bits, 13 * j), FS, BAUD, sigma=0.07, seed=400 + j, n_samples=NCALLS * C, phase0=0.3 * j) for j in range(NSIG)])
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def ref(signals):
    """ref[j][k]: snapshot of signal j's oracle behind call k (k in KEEP), all pushes of C samples."""
    out = []
    for j in range(NSIG):
        o, prev, snaps = oracle(), None, {}
        for k in range(1, NCALLS + 1):
            o(signals[j, (k - 1) * C:k * C], FS)
            if k in KEEP:
                snaps[k] = snapshot(o, prev)
            f = o.array("last_filtered")
            if f.size:
                prev = f[-1]
        out.append(snaps)
    return out


@pytest.fixture(scope="module")
def slab(signals):
    """[NCALLS][S64][C][2] float32 on the device: stream s is signal s % NSIG (a smaller engine reads the first streams of every call's slab)."""
    torch = pytest.importorskip("torch")
    base = torch.from_numpy(signals.view(np.float32).reshape(NSIG, NCALLS, C, 2).copy()).cuda()
    idx = torch.arange(S64, device="cuda") % NSIG
    out = base[idx].permute(1, 0, 2, 3).contiguous()
    torch.cuda.synchronize()
    return out


def engine(hd, S, pipeline, **kw):
    return hd.Engine(n_streams=S, max_chunk=C, sampling_rate=FS, decimation=D, baud=BAUD, pipeline=pipeline, **kw)


def push(hd, eng, slab, k, n=C):
    """Call k (1-based) of the slab; n: samples per stream, one number or one per stream."""
    if np.isscalar(n):
        eng.process_device(slab[k - 1].data_ptr(), C, int(n))
    else:
        n = np.ascontiguousarray(n, np.uint32)
        hd.capi.check(eng.L.hd_process_device(eng.h, slab[k - 1].data_ptr(), C, n.ctypes.data, 0))


# ---------------------------------------------------------------- 1. demodulated, from the ring

DEMOD_CASES = {
    #              S,  pipeline, environment,                         calls checked,     step_variant
    "per_cu_p2":  (S64, 2, {},                                        (1, 2, 5, 33, 34), 1),
    "per_cu_p1":  (S64, 1, {},                                        (1, 2, 5, 33, 34), 1),
    "k_step_5":   (5,   2, {},                                        (1, 2, 5, 33, 34), 0),      # an odd stream count never divides among the XCDs: the single-wave fallback
    "k_step_5_p1": (5,  1, {},                                        (1, 2, 5, 33, 34), 0),
    "no_cu_step": (S64, 2, {"HD_NO_CU_STEP": "1"},                    (1, 2, 5, 33, 34), 0),
    # position counters from 2^32 - 2501: they wrap 2^32 in call 3, and call 3's output starts at ring slot 32315 -- 453 samples, the ring's end, 571 samples
    "wrap_in_call": (S64, 2, {"HD_SYM_BASE0": hex(2 ** 32 - 2501)},   (1, 2, 3, 5),      1),
}


@pytest.mark.parametrize("case", list(DEMOD_CASES))
def test_demodulated_from_the_ring_equals_the_oracle(hd, slab, ref, monkeypatch, case):
    S, pipeline, env, checked, variant = DEMOD_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if case == "wrap_in_call":
        first = (2 ** 32 - 2501 + 2 * M) % RING_CAP
        assert first < RING_CAP < first + M                        # the third call's samples straddle the ring's end
    else:
        assert 32 * M == RING_CAP and max(checked) == 34           # the ring is full at the end of call 32: calls 33 and 34 are the first of its second turn
    eng = engine(hd, S, pipeline)
    for k in range(1, max(checked) + 1):
        push(hd, eng, slab, k)
        if k in checked:
            for s in range(S):
                assert same_bits(eng.demodulated(s), ref[s % NSIG][k]["demod"]), (case, "call", k, "stream", s)
            t = eng.timing()
            # (a stream's first call starts its stage-1 history from zeros, which the per-CU kernel does not do: the single-wave launch)
            assert t["path"] == 3 and t["step_variant"] == (variant if k > 1 else 0), (case, k, t)
    eng.close()


@pytest.mark.parametrize("pipeline", [2, 1])
def test_demodulated_across_a_switch_to_the_separate_kernels_and_back(hd, slab, signals, pipeline):
    """Call 3 removes DC on every stream: no stream tail takes such a call, so it runs through k_fir_demod / k_symbols (which read `demod`), between
    step calls whose output is in the ring only."""
    eng = engine(hd, S64, pipeline)
    orcs = [oracle() for _ in range(NSIG)]
    for k in range(1, 6):
        for s in range(S64):
            eng.set_dc_remove(s, k == 3)
        push(hd, eng, slab, k)
        for j, o in enumerate(orcs):
            o.set_dc_remove(k == 3)
            o(signals[j, (k - 1) * C:k * C], FS)
        for s in range(S64):
            assert same_bits(eng.demodulated(s), orcs[s % NSIG].array("last_demod")), ("call", k, "stream", s)
        assert eng.timing()["path"] == (0 if k == 3 else 3), (k, eng.timing())
    eng.close()


def ragged(k, S):
    """Samples per stream of call k in the ragged runs: call 4 hands the odd streams half a push."""
    return np.where(np.arange(S) % 2 == 1, C // 2, C).astype(np.uint32) if k == 4 else C


@pytest.mark.parametrize("pipeline", [2, 1])
def test_demodulated_behind_a_ragged_push(hd, slab, signals, pipeline):
    """Pushes of unequal size are no step call: stage 1, then the stream tails as a launch of their own (path 2) -- whose output is in the ring only as
    well --, in front of it the pending tails of call 3, behind it step calls again.  (Stream s is signal s % 8: odd streams, odd signals.)"""
    eng = engine(hd, S64, pipeline)
    orcs = [oracle() for _ in range(NSIG)]
    for k in range(1, 7):
        n = ragged(k, S64)
        push(hd, eng, slab, k, n)
        for j, o in enumerate(orcs):
            nj = int(n) if np.isscalar(n) else int(n[j])
            o(signals[j, (k - 1) * C:(k - 1) * C + nj], FS)       # (the half push's second half is never handed over: the engine reads call 5's slab next, so does the oracle)
        for s in range(S64):
            assert same_bits(eng.demodulated(s), orcs[s % NSIG].array("last_demod")), ("call", k, "stream", s)
        assert eng.timing()["path"] == (2 if k == 4 else 3), (k, eng.timing())
    eng.close()


# ---------------------------------------------------------------- 2. spectra on demand

def spectra_engines(hd, monkeypatch, arith=0):
    """(on demand, stored by every tail, synchronous)"""
    lazy = engine(hd, S64, 2, arith=arith)
    monkeypatch.setenv("HD_EAGER_SPECTRA", "1")
    eager = engine(hd, S64, 2, arith=arith)
    monkeypatch.delenv("HD_EAGER_SPECTRA")
    return lazy, eager, engine(hd, S64, 0, arith=arith)


FIRST_ASK = (5, 6, 7, 9)             # calls behind which an engine that has not been asked for a spectrum before is asked for the first time


def run_spectra(hd, slab, monkeypatch, arith=0, ragged_call=False):
    """`lazy` is asked behind every call: its spectra are transformed on demand 0 calls behind the buffer's completion (and asked twice).  The engines
    in `late` run free -- no getter, no flush -- until call k0 and are asked for the first time there: the buffer they transform then completed up to
    three calls earlier (all pushes equal: in call 4; ragged: in call 4 for the even streams, in call 5 for the odd ones) and the calls since have been
    filling the stream's OTHER buffer.  Each is asked again behind call 9, where the second buffer has completed (ragged: call 8 / call 9)."""
    lazy, eager, sync = spectra_engines(hd, monkeypatch, arith)
    late = {k0: engine(hd, S64, 2, arith=arith) for k0 in FIRST_ASK}
    fed = np.zeros(S64, np.int64)                                  # decimated samples handed to the spectrum collection so far
    for k in range(1, 10):
        n = ragged(k, S64) if ragged_call else C
        fed += np.broadcast_to(n, (S64,)) // D
        for e in (lazy, eager, sync):
            push(hd, e, slab, k, n)
            e.flush()
        for e in late.values():
            push(hd, e, slab, k, n)
        t = lazy.timing()
        assert t["path"] == (2 if ragged_call and k == 4 else 3) and eager.timing()["path"] == t["path"] and sync.timing()["path"] == 2, (k, t)
        assert (fed.max() >= 4096) == (k >= 4)
        for s in range(S64):
            if fed[s] < 4096:
                for e in (lazy, eager, sync):
                    assert e.spectrum(s).size == 0 and e.power(s).size == 0, ("a spectrum before the first buffer is full", k, s)
                continue
            p0 = lazy.power(s)                                     # power first, then the spectrum, then both again
            x0 = lazy.spectrum(s)
            assert same_bits(lazy.power(s), p0) and same_bits(lazy.spectrum(s), x0), ("asked twice", k, s)
            assert x0.size == 4096 and p0.size == 4096, (k, s)
            for name, e in (("stored", eager), ("synchronous", sync)):
                assert same_bits(x0, e.spectrum(s)), ("spectrum", name, k, s)
                assert same_bits(p0, e.power(s)), ("power", name, k, s)
                assert lazy.afc(s) == e.afc(s), ("afc", name, k, s)
        for k0, e in late.items():
            if k != k0 and k != 9:
                continue
            e.flush()      # (a getter answers 0 while the call that completed the stream's first buffer is undelivered, as ever: deliver; a flush transforms nothing)
            for s in range(S64):
                assert fed[s] >= 4096
                # (power of the odd streams first, the spectrum of the even ones: either getter must bring both arrays up to date)
                if s % 2:
                    p1 = e.power(s); x1 = e.spectrum(s)
                else:
                    x1 = e.spectrum(s); p1 = e.power(s)
                assert same_bits(x1, eager.spectrum(s)) and same_bits(p1, eager.power(s)), ("first asked behind call", k0, "asked behind", k, "stream", s)
                assert same_bits(x1, sync.spectrum(s)) and same_bits(p1, sync.power(s)), ("synchronous; first asked behind call", k0, "asked behind", k, "stream", s)
                assert e.afc(s) == eager.afc(s), ("afc; first asked behind call", k0, k, s)
            assert e.timing()["path"] == 3, (k0, k, e.timing())
    assert lazy.afc(0)["spectra"] == 2 and lazy.afc(1)["spectra"] == 2     # calls 4..9 lie 0 to 3 calls behind the first completion and 0 to 1 behind the second
    for e in (lazy, eager, sync, *late.values()):
        e.close()


def test_spectra_on_demand_equal_spectra_stored(hd, slab, monkeypatch):
    run_spectra(hd, slab, monkeypatch)


def test_spectra_on_demand_single_wave_step_kernel(hd, slab, monkeypatch):
    monkeypatch.setenv("HD_NO_CU_STEP", "1")
    run_spectra(hd, slab, monkeypatch)


def test_spectra_on_demand_behind_a_ragged_push(hd, slab, monkeypatch):
    """Call 4 is a tail launch of its own (path 2) in which the even streams complete their first buffer; the odd ones complete it a call later."""
    run_spectra(hd, slab, monkeypatch, ragged_call=True)


# ---------------------------------------------------------------- 3. fast mode

def test_fast_mode_demodulated_from_the_ring(hd, slab, ref):
    """arith=1: the batch engine's read-out from the ring against a synchronous engine's `demod` array bit for bit (same tail, same arithmetic), and
    against the oracle within the bound the fast mode's 1e-5 propagates to."""
    import bench
    batch, sync = engine(hd, S64, 2, arith=1), engine(hd, S64, 0, arith=1)
    worst = 0.0
    for k in range(1, 6):
        push(hd, batch, slab, k)
        push(hd, sync, slab, k)
        if k in (1, 2, 5):
            for s in range(S64):
                g, r = batch.demodulated(s), ref[s % NSIG][k]
                assert same_bits(g, sync.demodulated(s)), ("engine against engine", k, s)
                ex, _ = bench.demod_excess(g, r["demod"], r["filtered"], r["prev"], 1e-5, scale=r["dec_peak"])
                worst = max(worst, ex)
                assert ex <= 1.0, ("discriminator output beyond the propagated bound", k, s, ex)
            assert batch.timing()["path"] == 3 and sync.timing()["path"] == 2
    print("fast mode, demodulated from the ring: worst excess over the propagated bound", worst)
    batch.close(); sync.close()


def test_fast_mode_spectra_on_demand(hd, slab, monkeypatch):
    run_spectra(hd, slab, monkeypatch, arith=1)
