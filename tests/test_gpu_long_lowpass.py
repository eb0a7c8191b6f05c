"""Low-pass filters longer than 4097 taps, up to the longest the engine admits (hd_engine_lowpass_taps_max), against the CPU oracle call by call.

The design gives T = min(size_t(4 / transition), batch) | 1 taps (FirFilter.h:185-188), so a narrow transition makes the tap count follow the batch of the
call.  k_fir_demod keeps a tile's inputs for all taps in LDS: T64 is the longest filter that fits 64 KB (above it launch_fir_demod opts in to more dynamic
LDS), Tmax the longest that fits what the device grants a workgroup, and a design above Tmax is refused while the call is planned.  Covered here:

  1. T64, T64 + 2 and Tmax, exact mode, /1 (passthrough + separate kernels): a run from zeros and runs that carry history, on noise and on FSK;
  2. 161 and Tmax taps in the streams of one launch (the LDS image is sized by the longer one);
  3. the tap count following ragged batches (transition 1e-6: T = m + 1), /1 and /16: decreases, increases served from the previous call's buffer
     and from the side buffer behind an idle call, increases that grow the filter's buffer and restart it from zeros;
  4. an increase of exactly 8192 taps without a restart (the FirHistory head's capacity: bit-identical), and one of more -- the documented divergence
     (include/habdec_amd.h, hd_engine_lowpass_taps_max), pinned bit for bit against a float32 restatement;
  5. a design of Tmax + 2 taps: HD_ERR_CAPACITY, every stream untouched, the engine usable, in both arithmetic modes;
  6. fast mode at Tmax through the transforms and as direct sums, and through the /16 sequence of 3.

Exact mode: taps, decimated, filtered and discriminator floats bit-identical, bits and backlog equal on every call.  Fast mode: the gates of
test_gpu_fast.run_fast (1e-5 norm-wise, the discriminator within the propagated bound; bits, backlog and text identical)."""
import numpy as np
import pytest

from habdec_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-5
HD_ERR_CAPACITY = -4
HEAD = 8192          # samples of a run's input the engine keeps for a later run with more taps (engine.cpp: head_cap)
N1 = 19200           # a push at /1: 75 batches of 256 -- room for Tmax taps and, with max_chunk = 20480 (tap capacity 20738), it is the LDS limit that binds
MC1 = 20480
MC16 = 16 * 10240


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def limits(hd):
    """(T64, Tmax): the longest filter inside 64 KB of LDS (host arithmetic) and the longest the engine on this device admits (its getter)."""
    eng = hd.Engine(n_streams=1, max_chunk=MC1, sampling_rate=48000.0, decimation=1, enable_spectrum=False)
    tmax = eng.lowpass_taps_max()
    eng.close()
    t64 = hd.fir_demod_max_taps(64 * 1024)
    print("T64", t64, "Tmax", tmax)
    assert t64 % 2 == 1 and tmax % 2 == 1 and 4097 < t64
    assert t64 + 2 <= tmax <= min(0xFFFF, 20738), (t64, tmax)        # the device grants a workgroup more than 64 KB; the getter never exceeds the tap capacity
    assert tmax + 2 <= N1                                              # (a design of Tmax + 2 taps is possible on a batch of N1: test 5)
    return t64, tmax


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def tw_for(T):
    """A transition width whose design has exactly T taps on any batch of at least T samples: size_t(4.0f / tw) is T - 1 or T, forced odd."""
    assert T % 2 == 1
    tw = np.float32(4.0 / (T - 0.5))
    assert (int(np.float32(4.0) / tw) | 1) == T, (T, tw)
    return float(tw)


def noise(rng, n):
    return (0.4 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


class Rig:
    """An engine (S streams, keep_filtered) and one oracle per stream, fed the same per-stream pushes and control-plane changes."""

    def __init__(self, hd, *, factor, max_chunk, fs, trans, arith=0, pipeline=0, ungated=True, S=2):
        from oracle import pyoracle
        self.S, self.fs, self.max_chunk, self.exact = S, fs, max_chunk, arith == 0
        self.eng = hd.Engine(n_streams=S, max_chunk=max_chunk, sampling_rate=fs, decimation=factor, baud=300, rtty_bits=8, rtty_stops=2, ungated=ungated,
                             keep_filtered=True, enable_spectrum=False, pipeline=pipeline, arith=arith)
        self.orcs = [pyoracle.Decoder("oracle", factor=factor, baud=300, bits=8, stops=2, ungated=ungated, with_fft=False) for _ in range(S)]
        for s in range(S):
            self.set_trans(s, trans[s])
        self.prev = [None] * S
        self.worst = {"decimated": 0.0, "filtered": 0.0, "demod_over_bound": 0.0}

    def set_trans(self, s, t, oracle=True):
        self.eng.set_lowpass_trans(s, t)
        if oracle:
            self.orcs[s].lowpass_trans(t)

    def push(self, chunks):
        """chunks[s]: the samples stream s hands over (empty: it sits the call out).  Returns the engine's return code; the oracles see accepted pushes only."""
        sizes = np.array([len(c) for c in chunks], np.uint32)
        buf = np.zeros((self.S, self.max_chunk), np.complex64)
        for s, c in enumerate(chunks):
            buf[s, :len(c)] = c
        rc = self.eng.L.hd_process_host(self.eng.h, buf.ctypes.data, self.max_chunk, sizes.ctypes.data, 0)
        if rc == 0:
            for s, c in enumerate(chunks):
                if len(c):
                    self.orcs[s](c, self.fs)
        return rc

    def check(self, k, s):
        """Stream s after call k, in which it ran: exact mode bit for bit, fast mode within test_gpu_fast.run_fast's gates."""
        e, o = self.eng, self.orcs[s]
        assert same_bits(e.fir_taps(s), o.array("fir_taps")), ("taps", k, s, len(e.fir_taps(s)), len(o.array("fir_taps")))
        fo, do = o.array("last_filtered"), o.array("last_decimated")
        if self.exact:
            assert same_bits(e.decimated(s), do), ("decimated", k, s)
            assert same_bits(e.filtered(s), fo), ("filtered", k, s)
            assert same_bits(e.demodulated(s), o.array("last_demod")), ("demod", k, s)
        else:
            import bench
            w = self.worst
            w["decimated"] = max(w["decimated"], bench.normwise(e.decimated(s), do))
            w["filtered"] = max(w["filtered"], bench.fir_normwise(e.filtered(s), fo, do))
            ex, _ = bench.demod_excess(e.demodulated(s), o.array("last_demod"), fo, self.prev[s], TOL, scale=float(np.max(np.abs(do))) if do.size else None)
            w["demod_over_bound"] = max(w["demod_over_bound"], ex)
            print("fast", k, s, len(e.fir_taps(s)), w)
            assert w["decimated"] <= TOL and w["filtered"] <= TOL, ("floats", k, s, w)
            assert w["demod_over_bound"] <= 1.0, ("discriminator output beyond the propagated bound", k, s, w)
            if fo.size:
                self.prev[s] = fo[-1]
        assert np.array_equal(e.bits(s), o.bits()), ("bits", k, s)
        assert e.symbol_backlog(s) == o.symex_held(), ("backlog", k, s)

    def finish(self):
        self.eng.flush()                  # (an engine in its failed state refuses this)
        for s, o in enumerate(self.orcs):
            assert self.eng.rtty(s) == o.text("rtty_stream"), ("rtty", s)
            assert self.eng.take_sentences(s) == o.sentences(), ("sentences", s)
            assert self.eng.take_chars(s) == o.text("chars_log"), ("chars", s)
        self.eng.close()


def fsk_streams(S, fs, n, seed0):
    """S streams of n samples, each one short sentence as 300 baud 8N2 FSK at rate fs."""
    out = np.zeros((S, n), np.complex64)
    for s in range(S):
        b = synth.rtty_bits(synth.make_sentence(f"LP{s}", f"{s + 1},52.1,21.4"), 8, 2, 6 + 3 * s, 10)
        out[s] = synth.fsk_iq(b, fs, 300, sigma=0.08, seed=seed0 + s, n_samples=n)
    return out


# ---- 1. at each boundary, exact mode, /1

@pytest.mark.parametrize("signal", ["noise", "fsk"])
@pytest.mark.parametrize("which", ["T64", "T64+2", "Tmax"])
def test_boundary_tap_counts_are_bit_identical(hd, limits, which, signal):
    """The last filter inside 64 KB of LDS, the first above it (the launch that needs the opt-in) and the longest one admitted: four pushes of 19200
    samples at /1 -- the first run starts from zeros, the others carry T - 1 samples of history."""
    t64, tmax = limits
    T = {"T64": t64, "T64+2": t64 + 2, "Tmax": tmax}[which]
    S, fs, ncalls = 2, 48000.0, 4
    if signal == "noise":
        rng = np.random.default_rng(T)
        iq = np.stack([noise(rng, ncalls * N1) for _ in range(S)])
    else:
        iq = fsk_streams(S, fs, ncalls * N1, seed0=T)
    rig = Rig(hd, factor=1, max_chunk=MC1, fs=fs, trans=[tw_for(T)] * S, ungated=signal == "noise")
    for k in range(ncalls):
        assert rig.push([iq[s, k * N1:(k + 1) * N1] for s in range(S)]) == 0, hd.lib().hd_last_error()
        for s in range(S):
            assert len(rig.eng.fir_taps(s)) == T
            rig.check(k, s)
    assert rig.eng.timing()["path"] == 0
    if signal == "fsk":     # the sentence comes through the filter's delay of T / 2 samples: there is text to compare
        assert all(len(o.sentences()) == 1 for o in rig.orcs), [o.text("chars_log") for o in rig.orcs]
    rig.finish()


# ---- 2. mixed tap counts in one launch

def test_default_and_longest_filter_in_one_launch(hd, limits):
    """Stream 0 keeps the default 161 taps, stream 1 has Tmax: one k_fir_demod launch whose LDS image is sized by the longer filter."""
    _, tmax = limits
    S, fs = 2, 48000.0
    rng = np.random.default_rng(2)
    rig = Rig(hd, factor=1, max_chunk=MC1, fs=fs, trans=[0.025, tw_for(tmax)])
    for k in range(3):
        assert rig.push([noise(rng, N1) for _ in range(S)]) == 0
        assert [len(rig.eng.fir_taps(s)) for s in range(S)] == [161, tmax]
        for s in range(S):
            rig.check(k, s)
    rig.finish()


# ---- 3. the tap count following the batch

# decimated samples per call and stream (every push a whole number of 256-sample batches, so m = n / factor and T = m + 1), in units of `unit` samples
SEQ = [[2, 1, 2, 1, 0, 2, 4, 2, 4],
       [1, 2, 1, 2, 4, 0, 2, 4, 2]]


def run_following_sequence(hd, factor, pipeline, arith):
    """Drives SEQ with transition 1e-6 and returns (rig, kinds per stream, calls whose low-pass could take the transform route)."""
    unit = 4096 if factor == 1 else 2560            # /1: T up to 16385 (tap capacity 20738); /16: T up to 10241 (tap capacity 10498)
    S, fs = 2, (48000.0 if factor == 1 else 2.5e6)
    rng = np.random.default_rng(30 + factor)
    rig = Rig(hd, factor=factor, max_chunk=MC1 if factor == 1 else MC16, fs=fs, trans=[1e-6] * S, pipeline=pipeline, arith=arith)
    # the reference's bookkeeping, restated: the filter's one buffer grows to m + T and restarts from zeros when it does (FirFilter.h:141-147)
    buf, t_prev, m_prev, ran_prev = [0] * S, [None] * S, [0] * S, [False] * S
    kinds = [[] for _ in range(S)]
    fft_calls = 0
    for k in range(len(SEQ[0])):
        ms = [SEQ[s][k] * unit for s in range(S)]
        assert rig.push([noise(rng, m * factor) for m in ms]) == 0, hd.lib().hd_last_error()
        restart = False
        for s, m in enumerate(ms):
            if not m:
                ran_prev[s] = False
                continue
            T = len(rig.eng.fir_taps(s))
            assert T == m + 1 and len(rig.orcs[s].array("last_filtered")) == m, (k, s, T, m)
            if m + T > buf[s]:
                buf[s] = m + T
                kinds[s].append("first" if t_prev[s] is None else "grow_restart")
                restart = True
            elif T < t_prev[s]:
                kinds[s].append("decrease")
            else:
                # (within what the engine keeps of the previous run's input: its first min(8192, m) samples)
                assert 0 < T - t_prev[s] <= min(HEAD, m_prev[s]), (k, s, T, t_prev[s], m_prev[s])
                kinds[s].append("increase_from_previous_call" if ran_prev[s] else "increase_behind_idle_call")
            t_prev[s], m_prev[s], ran_prev[s] = T, m, True
            rig.check(k, s)
        fft_calls += 0 if restart else 1
    print(kinds)
    return rig, kinds, fft_calls


WANTED_KINDS = {"first", "decrease", "increase_from_previous_call", "increase_behind_idle_call", "grow_restart"}


@pytest.mark.parametrize("factor,pipeline", [(1, 0), (16, 0), (16, 1)])
def test_tap_count_following_ragged_batches(hd, limits, factor, pipeline):
    """Transition 1e-6: every run has as many taps as its batch allows, so the count changes from call to call.  /1 through the passthrough, /16 through two
    decimation stages (pipelined: the front half does not wait for the back half of the call before).  Every call bit-identical."""
    rig, kinds, _ = run_following_sequence(hd, factor, pipeline, arith=0)
    assert set(kinds[0]) == WANTED_KINDS and set(kinds[1]) >= WANTED_KINDS - {"increase_behind_idle_call"}, kinds
    assert rig.eng.timing()["path"] == 0
    rig.finish()


# ---- 4. an increase of exactly 8192 taps, and one of more

def restate(x, taps, m):
    """y[i] = sum_t x[i + t] taps[t] for i < m, t ascending from a zero sum, every product and every sum rounded to float32 (FirFilter.h:155-161)."""
    xr = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)
    acc = np.zeros((m, 2), np.float32)
    for t in range(len(taps)):
        acc += xr[t:t + m] * taps[t]
    return acc.reshape(-1).view(np.complex64)


def discriminate(hd, y, prev):
    out = np.zeros(len(y), np.float32)
    hd.lib().hd_host_discriminate(np.ascontiguousarray(y).view(np.float32), len(y), np.float32(prev.real), np.float32(prev.imag), out)
    return out


def test_increase_of_exactly_8192_taps_is_bit_identical(hd, limits):
    """Equal batches of 19200 at /1, the tap count set between them, the filter's buffer sized by the first run (Tmax taps) so that nothing restarts:
    161 -> 8353 taps takes the whole head the engine keeps (8192 samples) and is the oracle's bit for bit; so is the way back."""
    _, tmax = limits
    S, fs = 2, 48000.0
    rng = np.random.default_rng(4)
    plan = [tmax, 161, 161 + HEAD, 161, 161 + HEAD]
    rig = Rig(hd, factor=1, max_chunk=MC1, fs=fs, trans=[tw_for(plan[0])] * S)
    for k, T in enumerate(plan):
        for s in range(S):
            rig.set_trans(s, tw_for(T))
        assert rig.push([noise(rng, N1) for _ in range(S)]) == 0
        for s in range(S):
            assert len(rig.eng.fir_taps(s)) == T
            rig.check(k, s)
    rig.finish()


def test_increase_of_more_than_8192_taps_is_the_documented_image(hd, limits):
    """161 -> Tmax between equal batches, no restart: the engine reads zeros where the reference reads older samples of its buffer (include/habdec_amd.h,
    hd_engine_lowpass_taps_max).  The history of that run is [last 160 inputs | first 8192 inputs of the previous run | zeros]: its outputs are that
    image's sums bit for bit, the first T - 1 of them not the oracle's, from output T - 1 on the oracle's again; the run behind it carries on from the
    real inputs and is the oracle's.  (Bits and backlog are not compared: the symbol extractor has seen the diverging discriminator output.)"""
    _, tmax = limits
    S, fs, T = 2, 48000.0, tmax
    rng = np.random.default_rng(5)
    x = [np.stack([noise(rng, N1) for _ in range(S)]) for _ in range(4)]
    rig = Rig(hd, factor=1, max_chunk=MC1, fs=fs, trans=[tw_for(T)] * S)
    for k, Tk in enumerate([T, 161]):        # the buffer is sized by the first run; then the short filter
        for s in range(S):
            rig.set_trans(s, tw_for(Tk))
        assert rig.push(list(x[k])) == 0
        for s in range(S):
            rig.check(k, s)
    carry = [rig.orcs[s].array("last_filtered")[-1] for s in range(S)]
    for s in range(S):
        rig.set_trans(s, tw_for(T))
    assert rig.push(list(x[2])) == 0          # 161 -> Tmax without a restart
    y2 = []
    for s in range(S):
        taps = rig.eng.fir_taps(s)
        assert len(taps) == T and same_bits(taps, rig.orcs[s].array("fir_taps"))
        hist = np.concatenate([x[1][s][-160:], x[1][s][:HEAD], np.zeros(T - 1 - 160 - HEAD, np.complex64)])
        y = restate(np.concatenate([hist, x[2][s]]), taps, N1)
        fo = rig.orcs[s].array("last_filtered")
        got = rig.eng.filtered(s)
        assert same_bits(got, y), ("the diverging run is not the documented image", s, int(np.count_nonzero(got != y)))
        assert same_bits(y[T - 1:], fo[T - 1:]) and not same_bits(y[:T - 1], fo[:T - 1]), s
        assert same_bits(rig.eng.demodulated(s), discriminate(hd, y, carry[s])), ("demod", s)
        y2.append(y)
    assert rig.push(list(x[3])) == 0          # the run behind it: history = the last T - 1 real inputs
    for s in range(S):
        y = restate(np.concatenate([x[2][s][-(T - 1):], x[3][s]]), rig.eng.fir_taps(s), N1)
        assert same_bits(rig.eng.filtered(s), y) and same_bits(y, rig.orcs[s].array("last_filtered")), s
        assert same_bits(rig.eng.demodulated(s), discriminate(hd, y, y2[s][-1])), ("demod", s)
        assert same_bits(rig.eng.demodulated(s), rig.orcs[s].array("last_demod")), s
    rig.eng.flush()
    rig.eng.close()


# ---- 5. refusal

@pytest.mark.parametrize("arith,pipeline,when", [(0, 0, "running"), (0, 1, "running"), (0, 0, "first_run"), (0, 1, "first_run"), (1, 0, "running"), (1, 1, "first_run")])
def test_design_above_the_limit_is_refused_and_leaves_every_stream_untouched(hd, limits, arith, pipeline, when):
    """Stream 1 asks for Tmax + 2 taps while stream 0 runs -- set on a filter that has run (the design changes at once), or ahead of the stream's first
    run (the design is made while the call is planned).  The call returns HD_ERR_CAPACITY, nothing has been queued: with the transition restored every
    stream goes on call by call like oracles that saw only the accepted pushes, and the engine is not in its failed state."""
    _, tmax = limits
    S, fs = 2, 48000.0
    rng = np.random.default_rng(50 + arith)
    rig = Rig(hd, factor=1, max_chunk=MC1, fs=fs, trans=[0.025, tw_for(tmax)], arith=arith, pipeline=pipeline)
    k = 0
    for _ in range(2):
        chunks = [noise(rng, N1), noise(rng, N1 if when == "running" else 0)]
        assert rig.push(chunks) == 0
        for s in range(S):
            if len(chunks[s]):
                rig.check(k, s)
        k += 1
    rig.set_trans(1, tw_for(tmax + 2), oracle=False)
    refused = [noise(rng, N1) for _ in range(S)]
    assert rig.push(refused) == HD_ERR_CAPACITY
    assert b"hd_engine_lowpass_taps_max" in hd.lib().hd_last_error()
    assert rig.push(refused) == HD_ERR_CAPACITY            # ... and again: refusing changes nothing
    rig.set_trans(1, tw_for(tmax), oracle=False)
    for _ in range(2):
        assert rig.push([noise(rng, N1) for _ in range(S)]) == 0, hd.lib().hd_last_error()
        assert [len(rig.eng.fir_taps(s)) for s in range(S)] == [161, tmax]
        for s in range(S):
            rig.check(k, s)
        k += 1
    rig.finish()


# ---- 6. fast mode

@pytest.mark.parametrize("route", ["transforms", "direct"])
def test_fast_mode_longest_filter(hd, limits, monkeypatch, route):
    """Tmax taps at /1 in fast mode, six pushes of 19200 FSK samples: through 65536-point transforms (every run but the one from zeros), and with
    HD_NO_LP_FFT=1 as fused multiply-add sums of Tmax terms in k_fir_demod's largest launch."""
    from test_gpu_fast import run_fast
    _, tmax = limits
    if route == "direct":
        monkeypatch.setenv("HD_NO_LP_FFT", "1")
    S, fs, ncalls = 2, 48000.0, 6
    iq = fsk_streams(S, fs, ncalls * N1, seed0=600)
    eng, orcs, worst = run_fast(hd, iq, fs, factor=1, baud=300, bits=8, stops=2, lowpass_trans=tw_for(tmax), chunk=N1, expect_path=0)
    print(route, worst)
    assert len(eng.fir_taps(0)) == tmax and worst["filtered_n"] == ncalls * S * N1
    assert eng.timing()["lowpass_fft_calls"] == (ncalls - 1 if route == "transforms" else 0)
    assert all(len(o.sentences()) == 1 for o in orcs), [o.text("chars_log") for o in orcs]
    eng.close()


def test_fast_mode_tap_count_following_ragged_batches(hd, limits):
    """The /16 sequence of test 3 in fast mode: k_lp_gather rebuilds the history across every kind of tap-count change; calls in which a stream restarts
    from zeros are direct sums."""
    rig, kinds, fft_calls = run_following_sequence(hd, 16, 0, arith=1)
    assert set(kinds[0]) == WANTED_KINDS, kinds
    assert rig.eng.timing()["lowpass_fft_calls"] == fft_calls and fft_calls >= 4, (rig.eng.timing(), fft_calls)
    rig.finish()
