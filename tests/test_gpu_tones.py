"""The tone-filter demodulator on the GPU (hd_tones_*, kernels/tones.hip).

Behind the quantisation the demodulator is integer arithmetic: rows are compared byte for byte with the host restatement (hd_host_tones_*), which
tests/test_tones_host.py holds to the numpy model of the definition."""
import numpy as np
import pytest

import tones_model as TM
from habdec_amd import synth
from test_gpu_clocked import ROUTES, RT

pytestmark = pytest.mark.gpu
PUSHES = (1, 63, 64, 65, 4097)
HD_ERR_INVALID, HD_ERR_UNSUPPORTED, HD_ERR_CAPACITY = -1, -3, -4


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


# ---------------------------------------------------------------- kernel parity

# (the stream of tones_model.streams() whose IQ is pushed, baud, f_hi, f_lo) on an engine with fsd = 32 kS/s.  The rows are held to the restatement with the
# same modem, so a modem need not fit the signal: what counts is the modems' spread -- 4 to 2048 samples per bit, tones at 0, at the band's edges, both negative.
MODEMS = [("600_8n2", 600.0, 250.0, -250.0), ("300_8n2_32k", 300.0, 250.0, -250.0), ("50_7n2", 50.0, 250.0, -250.0), ("w1", 8000.0, 1000.0, -1000.0),
          ("w2048", 15.625, 250.0, -250.0), ("specials", 300.0, 250.0, -250.0), ("tone_at_0", 300.0, 0.0, -500.0),
          ("tones_at_the_edges", 1200.0, 15999.99, -15999.99), ("tones_negative", 45.45, -1000.0, -1500.0), ("110_8n2", 110.0, 170.0, -255.0)]
N_PARITY = 40000


@pytest.fixture(scope="module")
def parity_iq():
    by = {s[0]: s[1] for s in TM.streams()}
    return [by[name][:N_PARITY] for name, _, _, _ in MODEMS]


@pytest.mark.parametrize("window_q8", [32, 256], ids=["q32", "q256"])
def test_push_device_and_push_host_equal_the_host_restatement(hd, torch, parity_iq, window_q8):
    """Every stream with its own modem in one launch (window_q8 32: W = 1 at 4 samples per bit; 256: W = 2048 and L = 16384 at 2048); per push the sizes 1,
    63, 64, 65 and 4097 in turn, shifted from stream to stream, one stream empty in every third push, and one push longer than the longest L."""
    S = len(MODEMS)
    eng = hd.Engine(n_streams=S)                                     # fsd = 32 kS/s
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    from_host, from_dev = eng.tones(window_q8=window_q8, max_push=20000), eng.tones(window_q8=window_q8, max_push=20000)
    ref = []
    for s, (name, baud, f_hi, f_lo) in enumerate(MODEMS):
        from_host.set_modem(s, baud, f_hi, f_lo); from_dev.set_modem(s, baud, f_hi, f_lo)
        ref.append(hd.HostTones(fsd, baud, f_hi, f_lo, window_q8=window_q8))
        want = TM.modem(fsd, baud, f_hi, f_lo, window_q8)
        for t in (from_host, from_dev):
            st = t.stats(s)
            assert all(st[k] == v for k, v in want.items()) and st["samples"] == 0, (name, st, want)
    W = [r.stats()["W"] for r in ref]
    assert (1 in W) == (window_q8 == 32) and (2048 in W) == (window_q8 == 256) and max(r.stats()["L"] for r in ref) == 16384
    at, push, stride = [0] * S, 0, 20000
    while any(at[s] < parity_iq[s].size for s in range(S)):
        n = np.array([PUSHES[(push + 2 * s) % len(PUSHES)] for s in range(S)], np.uint32)
        if push == 5:
            n[:] = 20000 - np.arange(S) * 3                          # longer than every L: five launches
        if push % 3 == 0:
            n[push // 3 % S] = 0
        n = np.minimum(n, [parity_iq[s].size - at[s] for s in range(S)]).astype(np.uint32)
        slab = np.full((S, stride), np.nan + 1j * np.nan, np.complex64)
        want = []
        for s in range(S):
            slab[s, :n[s]] = parity_iq[s][at[s]:at[s] + n[s]]
            want.append(ref[s].push(slab[s, :n[s]]))
            at[s] += int(n[s])
        from_host.push_host(slab, n)
        d = torch.from_numpy(slab.view(np.float32)).cuda()
        from_dev.push_device(d.data_ptr(), stride, n)
        del d
        for what, t in (("host memory", from_host), ("device memory", from_dev)):
            assert np.array_equal(t.rows()[2], n), (what, push)
            for s in range(S):
                got = t.output(s)
                assert got.tobytes() == want[s].tobytes(), (what, push, MODEMS[s][0], int(n[s]), np.flatnonzero(got != want[s])[:8] if got.size == want[s].size else got.size)
        push += 1
    for s in range(S):
        for t in (from_host, from_dev):
            assert t.stats(s)["samples"] == parity_iq[s].size == ref[s].stats()["samples"]
            assert eng.L.hd_debug_tones_guards(t.h, s) == 0, s
    # reset of one stream and of all: the sample index starts again, the modem stays
    from_dev.reset(0)
    assert from_dev.stats(0)["samples"] == 0 and from_dev.stats(1)["samples"] == parity_iq[1].size and from_dev.rows()[2][0] == 0
    ref[0].reset()
    first = np.zeros((S, 700), np.complex64)
    first[0] = parity_iq[0][:700]
    from_dev.push_host(first, np.array([700] + [0] * (S - 1), np.uint32))
    assert from_dev.output(0).tobytes() == ref[0].push(first[0]).tobytes() and from_dev.output(1).size == 0
    from_dev.reset()
    assert all(from_dev.stats(s)["samples"] == 0 and from_dev.stats(s)["W"] == W[s] for s in range(S))
    eng.close()


# ---------------------------------------------------------------- every route the decimated IQ can take to the demodulator

TONE_HI, TONE_LO = TM.SHIFT / 2, -TM.SHIFT / 2


@pytest.fixture(scope="module")
def route_iq():
    S, n = RT["S"], RT["n"] * RT["calls"]
    out = np.zeros((S, n), np.complex64)
    for s in range(S):
        text = "".join(synth.make_sentence(f"R{s}", str(k)) for k in range(8))
        out[s] = synth.fsk_iq(synth.rtty_bits(text, RT["bits"], RT["stops"], 2 + s % 5, 4), RT["fs"], RT["baud"], sigma=0.05, seed=700 + s, n_samples=n)
    return out


@pytest.fixture(scope="module")
def route_want(hd, route_iq):
    """Per decimation factor and DC blocker: the restatement over the ORACLE's decimated IQ, call by call -- [stream][call] rows."""
    from oracle import pyoracle
    cache = {}

    def want(factor, dc):
        if (factor, dc) not in cache:
            out = []
            for s in range(RT["S"]):
                dec = pyoracle.Decoder("oracle", factor=factor, baud=RT["baud"], bits=RT["bits"], stops=RT["stops"], lowpass_bw=RT["bw"], with_fft=False)
                dec.set_dc_remove(dc)
                h = hd.HostTones(RT["fs"] / factor, RT["baud"], TONE_HI, TONE_LO)
                rows = []
                for k in range(RT["calls"]):
                    dec(route_iq[s, k * RT["n"]:(k + 1) * RT["n"]], RT["fs"])
                    rows.append(h.push(dec.array("last_decimated")))
                out.append(rows)
            cache[(factor, dc)] = out
        return cache[(factor, dc)]
    return want


@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_push_engine_on_every_route(hd, route_iq, route_want, route, arith):
    """Exact mode: the rows are the restatement's over the oracle's decimated IQ.  Fast mode, and a front-tuned stream in either: over the engine's own."""
    extra, path, variant, front = ROUTES[route]
    S, calls, n = RT["S"], RT["calls"], RT["n"]
    cfg = dict(n_streams=S, max_chunk=n, sampling_rate=RT["fs"], decimation=64, baud=RT["baud"], rtty_bits=RT["bits"], rtty_stops=RT["stops"],
               lowpass_bw_hz=RT["bw"], arith=arith)
    cfg.update(extra)
    eng = hd.Engine(**cfg)
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    for s, f in front.items():
        eng.set_front_tune(s, f)
    tones = eng.tones()
    own = []
    for s in range(S):
        tones.set_modem(s, 0, TONE_HI, TONE_LO)                      # baud 0: the engine stream's
        assert tones.stats(s)["F"] == TM.modem(fsd, RT["baud"], TONE_HI, TONE_LO)["F"]
        own.append(hd.HostTones(fsd, RT["baud"], TONE_HI, TONE_LO))
    want = route_want(cfg["decimation"], bool(cfg.get("dc_remove", False))) if arith == 0 else None
    compared = 0
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(route_iq[:, k * n:(k + 1) * n]))
        tones.push_engine()
        t = eng.timing()
        assert t["path"] == path, (route, k, t)
        if variant is not None and k >= 1:
            assert t["step_variant"] == variant, (route, k, t)
        if k in (0, 5):                                              # a second push without a call in between changes nothing
            tones.push_engine()
        for s in range(S):
            got = tones.output(s)
            mine = own[s].push(eng.decimated(s))
            assert got.size == mine.size == n // cfg["decimation"] and got.tobytes() == mine.tobytes(), (route, k, s, "the engine's own decimated IQ")
            if arith == 0 and s not in front:
                assert got.tobytes() == want[s][k].tobytes(), (route, k, s, "the oracle's decimated IQ")
            compared += got.size
        assert tones.stats(0)["samples"] == (k + 1) * (n // cfg["decimation"])
    assert compared == S * calls * (n // cfg["decimation"])
    assert all(eng.L.hd_debug_tones_guards(tones.h, s) == 0 for s in range(S))
    # the tones from the AFC: both peaks valid, or HD_ERR_INVALID
    for s in range(S):
        a = eng.afc(s)
        rc = eng.L.hd_tones_set_modem_from_afc(tones.h, s, 0.0)
        f_hi, f_lo = (a["peak_r"] - 2048) * fsd / 4096, (a["peak_l"] - 2048) * fsd / 4096
        if a["peak_l"] > 0 and a["peak_r"] > 0 and -fsd / 2 < f_lo < f_hi:
            m = TM.modem(fsd, RT["baud"], f_hi, f_lo)
            st = tones.stats(s)
            assert rc == 0 and (st["step_hi"], st["step_lo"], st["samples"]) == (m["step_hi"], m["step_lo"], 0), (route, s, a, st)
        else:
            assert rc == HD_ERR_INVALID, (route, s, a)
    eng.close()


# ---------------------------------------------------------------- the chain on a weak signal: tones -> clocked

SIGMA = 1.0


@pytest.fixture(scope="module")
def weak(hd):
    """The signal, what was sent, the oracle's sentences, and the CPU chain's: restatement over the oracle's decimated IQ -> host clocked decoder."""
    iq, sent = TM.weak_iq(SIGMA)
    fsd = TM.WEAK["fs"] / TM.WEAK["D"]
    oracle, cpu = [], []
    for o, decim, _ in TM.weak_oracle(iq):
        t = hd.HostTones(fsd, TM.WEAK["baud"], TONE_HI, TONE_LO)
        h = hd.HostClocked(fsd, TM.WEAK["baud"], TM.WEAK["bits"], TM.WEAK["stops"])
        for d in decim:
            h.push(t.push(d))
        oracle.append(o)
        cpu.append(h.take_sentences(256))
    return iq, sent, oracle, cpu


def test_a_signal_below_the_discriminators_threshold_end_to_end(hd, weak):
    iq, sent, oracle, cpu = weak
    S, n, calls = TM.WEAK["S"], TM.WEAK["n"], TM.WEAK["calls"]
    eng = hd.Engine(n_streams=S, max_chunk=n, sampling_rate=TM.WEAK["fs"], decimation=TM.WEAK["D"], baud=TM.WEAK["baud"], rtty_bits=8, rtty_stops=2,
                    lowpass_bw_hz=TM.WEAK["bw"])
    tones, from_tones, from_disc = eng.tones(), eng.clocked(), eng.clocked()
    for s in range(S):
        tones.set_modem(s, TM.WEAK["baud"], TONE_HI, TONE_LO)
    ordinary = [[] for _ in range(S)]
    eng.on_sentence(lambda s, call, data, crc: ordinary[s].append(f"{call},{data}*{crc}"))
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        tones.push_engine()
        from_tones.push_tones(tones)
        from_disc.push_engine()
    eng.flush()
    n_disc = n_plain = n_all = 0
    for s in range(S):
        assert ordinary[s] == oracle[s], (s, ordinary[s], oracle[s])
        got = from_tones.take_sentences(s, 256)
        assert got == cpu[s], (s, got, cpu[s])                       # positions, flip counts and text
        disc = from_disc.take_sentences(s, 256)
        assert all(t in sent[s] for (_, _, t) in got + disc), (s, got, disc)
        assert from_tones.stats(s)["samples"] == n * calls // TM.WEAK["D"]
        n_disc += len(disc); n_plain += len([1 for g in got if g[1] == 0]); n_all += len(got)
    print("signal at sigma", SIGMA, ": ordinary", sum(len(o) for o in ordinary), "discriminator row with repair", n_disc, "tone row plain", n_plain, "with repair", n_all,
          "of", 7 * S)
    assert 2 * n_disc < 7 * S and n_plain >= n_disc + 3 and n_all >= n_plain + 3
    assert eng.L.hd_engine_sentences_ok(eng.h) == sum(len(o) for o in ordinary)
    eng.close()


# ---------------------------------------------------------------- errors

def test_bad_parameters_and_null_arguments(hd):
    eng = hd.Engine(n_streams=2, sampling_rate=25600.0, decimation=64, baud=50, rtty_bits=7, lowpass_bw_hz=150.0)        # fsd = 400
    L = eng.L
    for q8 in (31, 257):
        with pytest.raises(hd.HabdecError):
            eng.tones(window_q8=q8)
    t = eng.tones(max_push=100)
    assert L.hd_tones_set_modem(t.h, 0, 400 / 3.4, 50.0, -50.0) == HD_ERR_UNSUPPORTED
    assert L.hd_tones_set_modem(t.h, 0, 400 / 2049.0, 50.0, -50.0) == HD_ERR_UNSUPPORTED
    assert L.hd_tones_set_modem(t.h, 0, 50.0, 200.0, -50.0) == HD_ERR_INVALID           # |f| >= fsd / 2
    assert L.hd_tones_set_modem(t.h, 0, 50.0, 50.0, -200.0) == HD_ERR_INVALID
    assert L.hd_tones_set_modem(t.h, 0, 50.0, 50.0, 50.0) == HD_ERR_INVALID             # f_hi not above f_lo
    assert L.hd_tones_set_modem(t.h, 2, 50.0, 50.0, -50.0) == HD_ERR_INVALID
    assert L.hd_tones_set_modem(None, 0, 50.0, 50.0, -50.0) == HD_ERR_INVALID
    assert L.hd_tones_set_modem_from_afc(t.h, 0, 50.0) == HD_ERR_INVALID                # no call yet: no peaks
    assert L.hd_tones_reset(t.h, 2) == HD_ERR_INVALID and L.hd_tones_push_engine(None) == HD_ERR_INVALID
    assert L.hd_tones_stats(t.h, 0, None) == HD_ERR_INVALID and L.hd_tones_stats(t.h, 2, None) == HD_ERR_INVALID
    assert L.hd_tones_output(t.h, 2, None, 0) == HD_ERR_INVALID and L.hd_tones_output(t.h, 0, None, 4) == HD_ERR_INVALID
    assert L.hd_tones_rows(t.h, None, None, None) == HD_ERR_INVALID and L.hd_tones_rows(None, None, None, None) == HD_ERR_INVALID
    iq = np.ones((2, 100), np.complex64)
    assert L.hd_tones_push_host(t.h, None, 100, None, 100) == HD_ERR_INVALID
    n = np.array([101, 3], np.uint32)
    assert L.hd_tones_push_host(t.h, iq.ctypes.data, 100, n.ctypes.data, 0) == HD_ERR_INVALID   # a row longer than the stride
    t.push_host(iq)                                                  # no stream has a modem yet: passed by
    assert t.stats(0)["F"] == 0 and t.stats(0)["samples"] == 0 and t.output(0).size == 0
    t.set_modem(0, 0, 50.0, -50.0)                                   # the engine stream's baud
    assert t.stats(0)["F"] == 8 << 16 and t.stats(1)["F"] == 0
    assert L.hd_tones_push_device(t.h, iq.ctypes.data, 100, None, 100) == HD_ERR_INVALID        # host memory is not device memory
    t.push_host(iq)
    assert t.stats(0)["samples"] == 100 and t.output(0).size == 100 and t.output(1).size == 0
    long = np.ones((2, 101), np.complex64)
    assert L.hd_tones_push_host(t.h, long.ctypes.data, 101, None, 101) == HD_ERR_CAPACITY       # longer than max_push
    assert t.stats(0)["samples"] == 100 and t.output(0).size == 100
    t.push_engine()                                                  # no call yet: adds nothing
    assert t.stats(0)["samples"] == 100
    assert L.hd_debug_tones_guards(t.h, 0) == 0 and L.hd_debug_tones_guards(t.h, 1) == 0
    eng.close()


# ---------------------------------------------------------------- the guard hook itself

def damage_the_row_guards(hook, d_rows, stride, max_push):
    """What an hd_debug_*_guards hook says of three streams' output rows while four guard words are overwritten in device memory, and after they are put
    back.  d_rows, stride: as hd_*_rows gives them (the address of row 0's payload, a row's stride in floats); G words guard a row on either side."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int], ctypes.c_int
    to_device, to_host = 1, 2
    G = (stride - max_push) // 2
    assert G >= 1 and stride == max_push + 2 * G
    words = [-G,                                  # the first word of the allocation
             stride - 1,                          # the last word of stream 1's front guard
             stride + max_push,                   # the first word of stream 1's back guard
             2 * stride + max_push + G - 1]       # the last word of the allocation
    saved = []
    for w in words:
        v = ctypes.c_uint32(0)
        assert hip.hipMemcpy(ctypes.byref(v), d_rows + 4 * w, 4, to_host) == 0
        saved.append(v.value)
        bad = ctypes.c_uint32(v.value ^ 0xFFFFFFFF)
        assert hip.hipMemcpy(d_rows + 4 * w, ctypes.byref(bad), 4, to_device) == 0
    assert len(set(saved)) == 1, saved            # all four held the one pattern
    damaged = [hook(s) for s in range(3)]
    for w, v in zip(words, saved):
        assert hip.hipMemcpy(d_rows + 4 * w, ctypes.byref(ctypes.c_uint32(v)), 4, to_device) == 0
    return damaged, [hook(s) for s in range(3)]


def test_the_guard_hook_counts_damaged_words(hd):
    """The hook looks at the words that guard the rows: the outermost words of the array and the two guards between streams 1's neighbours."""
    eng = hd.Engine(n_streams=3, max_chunk=TM.WEAK["n"], sampling_rate=TM.WEAK["fs"], decimation=TM.WEAK["D"])
    t = eng.tones(max_push=64)
    d_rows, stride, _ = t.rows()
    damaged, restored = damage_the_row_guards(lambda s: eng.L.hd_debug_tones_guards(t.h, s), d_rows, stride, 64)
    assert damaged == [1, 2, 1] and restored == [0, 0, 0]
    eng.close()
