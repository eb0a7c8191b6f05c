"""The clocked decoder on the GPU (hd_clocked_*, kernels/clocked.hip).

Behind the quantisation the decoder is integer arithmetic: records are compared byte for byte with the host restatement (hd_host_clocked_*), which
tests/test_clocked_host.py holds to the numpy model of the definition."""
import math

import numpy as np
import pytest

import baud_probe_model as M
import clocked_model as CM
from habdec_amd import capi, synth

pytestmark = pytest.mark.gpu
PUSHES = (1, 63, 64, 65, 4097)
BIG = 1 << 14
HD_ERR_INVALID, HD_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def baud_for(F, fsd):
    """A baud rate that gives the clock step F at the decimated rate fsd (streams designed for other rates run on one engine: only fsd / baud counts)."""
    baud = fsd / (F / 65536.0)
    for _ in range(8):
        got = int(math.floor(fsd / baud * 65536 + 0.5))
        if got == F:
            return baud
        baud = math.nextafter(baud, 0.0 if got < F else math.inf)
    raise AssertionError((F, fsd))


# ---------------------------------------------------------------- kernel parity

NAMES = ("600_8n2", "300_8n2_32k", "150_7n1", "45_7n1", "specials", "zeros", "positive", "square", "spb4", "spb130", "spb2048")


@pytest.fixture(scope="module")
def parity_streams():
    """Eleven of the streams of tests/test_clocked_host.py, at most 100000 samples of each (the sample ring of 32768 wraps three times)."""
    by = {s[0]: s for s in CM.streams()}
    return [(n, by[n][1][:100000]) + by[n][2:] for n in NAMES]


def test_push_device_and_push_host_equal_the_host_decoder(hd, torch, parity_streams):
    """Every stream with its own modem in one launch; per push the sizes 1, 63, 64, 65 and 4097 in turn, shifted from stream to stream, one stream empty in
    every third push, and one push larger than the sample ring."""
    S = len(parity_streams)
    eng = hd.Engine(n_streams=S)                                     # fsd = 32 kS/s
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    from_host, from_dev = eng.clocked(record_cap=BIG), eng.clocked(record_cap=BIG)
    ref, rows = [], []
    for s, (name, row, sfsd, baud, nbits, nstops) in enumerate(parity_streams):
        F = CM.clock(sfsd, baud, nbits, nstops)[0]
        b = baud_for(F, fsd)
        from_host.set_modem(s, b, nbits, nstops); from_dev.set_modem(s, b, nbits, nstops)
        ref.append(hd.HostClocked(sfsd, baud, nbits, nstops, record_cap=BIG))
        rows.append(row)
    at, push, stride = [0] * S, 0, 40000
    while any(at[s] < rows[s].size for s in range(S)):
        n = np.array([PUSHES[(push + 2 * s) % len(PUSHES)] for s in range(S)], np.uint32)
        if push == 5:
            n[:] = 40000 - np.arange(S) * 3                          # larger than the ring: ten launches
        if push % 3 == 0:
            n[push // 3 % S] = 0
        n = np.minimum(n, [rows[s].size - at[s] for s in range(S)]).astype(np.uint32)
        slab = np.full((S, stride), np.nan, np.float32)
        for s in range(S):
            slab[s, :n[s]] = rows[s][at[s]:at[s] + n[s]]
            ref[s].push(slab[s, :n[s]])
            at[s] += int(n[s])
        from_host.push_host(slab, n)
        d = torch.from_numpy(slab).cuda()
        from_dev.push_device(d.data_ptr(), stride, n)
        del d
        push += 1
        if push in (1, 2, 6, 7, 40):
            for s in range(S):
                want = ref[s].stats()
                for c in (from_host, from_dev):
                    got = c.stats(s)
                    assert all(got[k] == want[k] for k in ("samples", "cursor", "characters", "rejects", "dropped")), (push, s, got, want)
    total = 0
    for s in range(S):
        want, st = ref[s].records(), ref[s].stats()
        for what, c in (("host memory", from_host), ("device memory", from_dev)):
            got_st = c.stats(s)
            assert all(got_st[k] == st[k] for k in ("samples", "cursor", "characters", "rejects", "dropped")), (what, s, got_st, st)
            got = c.records(s)
            assert got.tobytes() == want.tobytes(), (what, NAMES[s], got.size, want.size)
            assert c.waiting(s) == 0
        assert st["samples"] == rows[s].size and st["dropped"] == 0
        total += want.size                                           # (the four design signals alone carry 403 characters)
    assert total >= 400 and ref[NAMES.index("600_8n2")].stats()["samples"] > 2 * capi.CLOCKED_RING
    # reset of one stream and of all
    from_dev.reset(0)
    assert from_dev.stats(0)["samples"] == 0 and from_dev.stats(1)["samples"] == rows[1].size
    from_dev.reset()
    assert all(from_dev.stats(s)["samples"] == 0 for s in range(S))
    eng.close()


# ---------------------------------------------------------------- every route the discriminator output can take to the decoder

RT = dict(S=8, fs=153600.0, n=16384, baud=300.0, bits=8, stops=2, bw=800.0, calls=14)      # (the step kernel wants pushes of whole 2048-sample tiles)
ROUTES = {
    # name: engine settings, hd_timing.path, step_variant from the second call on, streams tuned at the input rate
    "sync_tail": (dict(), 2, None, {}),                               # the linear demod row
    "batch_tail_ring": (dict(pipeline=1), 2, None, {3: 1000.0}),      # a front-tuned stream keeps a batch engine's calls off the step kernel: k_tail, ring
    "batch_step_ring": (dict(pipeline=1), 3, 1, {}),                  # k_step_cu
    "separate": (dict(decimation=16, dc_remove=True), 0, None, {}),   # the DC blocker sends a call through the separate kernels
}


@pytest.fixture(scope="module")
def route_iq():
    S, n = RT["S"], RT["n"] * RT["calls"]
    out, sent = np.zeros((S, n), np.complex64), []
    for s in range(S):
        text = "".join(synth.make_sentence(f"R{s}", str(k)) for k in range(8))
        sent.append({t.strip("$\n") for t in text.split("\n") if t})
        out[s] = synth.fsk_iq(synth.rtty_bits(text, RT["bits"], RT["stops"], 2 + s % 5, 4), RT["fs"], RT["baud"], sigma=0.05, seed=700 + s, n_samples=n)
    return out, sent


@pytest.fixture(scope="module")
def route_want(hd, route_iq):
    """Per decimation factor and DC blocker: the host decoder over the ORACLE's discriminator output, call by call -- (records, sentences) per stream."""
    from oracle import pyoracle
    iq, _ = route_iq
    cache = {}

    def want(factor, dc):
        if (factor, dc) not in cache:
            out = []
            for s in range(RT["S"]):
                dec = pyoracle.Decoder("oracle", factor=factor, baud=RT["baud"], bits=RT["bits"], stops=RT["stops"], lowpass_bw=RT["bw"], with_fft=False)
                dec.set_dc_remove(dc)
                h = hd.HostClocked(RT["fs"] / factor, RT["baud"], RT["bits"], RT["stops"], record_cap=BIG)
                for k in range(RT["calls"]):
                    dec(iq[s, k * RT["n"]:(k + 1) * RT["n"]], RT["fs"])
                    h.push(dec.array("last_demod"))
                out.append((h.records(), h.take_sentences()))
            cache[(factor, dc)] = out
        return cache[(factor, dc)]
    return want


@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_push_engine_on_every_route(hd, route_iq, route_want, route, arith):
    extra, path, variant, front = ROUTES[route]
    iq, sent = route_iq
    S, calls, n = RT["S"], RT["calls"], RT["n"]
    cfg = dict(n_streams=S, max_chunk=n, sampling_rate=RT["fs"], decimation=64, baud=RT["baud"], rtty_bits=RT["bits"], rtty_stops=RT["stops"],
               lowpass_bw_hz=RT["bw"], arith=arith)
    cfg.update(extra)
    eng = hd.Engine(**cfg)
    for s, f in front.items():
        eng.set_front_tune(s, f)
    clk = eng.clocked(record_cap=BIG)                                # every stream takes the engine stream's modem
    ordinary = []
    eng.on_sentence(lambda s, call, data, crc: ordinary.append((s, call)))
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        clk.push_engine()
        t = eng.timing()
        assert t["path"] == path, (route, k, t)
        if variant is not None and k >= 1:
            assert t["step_variant"] == variant, (route, k, t)
        if k in (0, 5):                                              # a second push without a call in between changes nothing
            clk.push_engine()
    eng.flush()
    want = route_want(cfg["decimation"], bool(cfg.get("dc_remove", False)))
    got_sentences = 0
    for s in range(S):
        if s in front:
            continue                                                 # (tuned 1 kHz away at the input rate: not the oracle's signal)
        rec, sen = want[s]
        got = clk.take_sentences(s)
        if arith == 0:
            # take_sentences drained the ring through the text stage: the records are compared on a second decoder below; here sentences and counters
            assert clk.stats(s)["characters"] == rec.size, (route, s)
        assert [(f, t) for (_, f, t) in got] == [(f, t) for (_, f, t) in sen], (route, s, got, sen)
        assert all(t in sent[s] for (_, _, t) in got)
        got_sentences += len(got)
    assert got_sentences >= S
    # nothing of the clocked decoder goes through the ordinary callback's count
    assert eng.L.hd_engine_sentences_ok(eng.h) == len(ordinary)
    eng.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_push_engine_records_equal_the_host_decoder_over_the_oracle(hd, route_iq, route_want, route):
    extra, path, variant, front = ROUTES[route]
    iq, _ = route_iq
    S, calls, n = RT["S"], RT["calls"], RT["n"]
    cfg = dict(n_streams=S, max_chunk=n, sampling_rate=RT["fs"], decimation=64, baud=RT["baud"], rtty_bits=RT["bits"], rtty_stops=RT["stops"],
               lowpass_bw_hz=RT["bw"])
    cfg.update(extra)
    eng = hd.Engine(**cfg)
    for s, f in front.items():
        eng.set_front_tune(s, f)
    clk = eng.clocked(record_cap=BIG)
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        clk.push_engine()
    want = route_want(cfg["decimation"], bool(cfg.get("dc_remove", False)))
    for s in range(S):
        if s not in front:
            got = clk.records(s)
            assert got.size > 20 and got.tobytes() == want[s][0].tobytes(), (route, s, got.size, want[s][0].size)
    eng.close()


# ---------------------------------------------------------------- end to end on a weak signal

WEAK = dict(fs=32000.0, D=4, n=16000, calls=24, sigma=0.85, S=8)      # 300 baud 8N2 at fsd 8000: rung (b) of NOTES.md's ladder, through the whole chain


@pytest.fixture(scope="module")
def weak_inputs(hd):
    from oracle import pyoracle
    S, n, calls = WEAK["S"], WEAK["n"], WEAK["calls"]
    iq, sent, oracle = np.zeros((S, n * calls), np.complex64), [], []
    for s in range(S):
        text = "".join(synth.make_sentence(f"W{s}", "%d,12:00:%02d,52.%04d,-0.1234,%d" % (k, k, 1000 + s * 7 + k, 100 * k)) for k in range(12))
        sent.append({t.strip("$\n") for t in text.split("\n") if t})
        iq[s] = synth.fsk_iq(synth.rtty_bits(text, 8, 2, 3, 0), WEAK["fs"], 300.0, sigma=WEAK["sigma"], seed=500 + s, n_samples=n * calls)
        dec = pyoracle.Decoder("oracle", factor=WEAK["D"], baud=300, bits=8, stops=2, lowpass_bw=1500.0, with_fft=False)
        for k in range(calls):
            dec(iq[s, k * n:(k + 1) * n], WEAK["fs"])
        oracle.append(dec.sentences())
    return iq, sent, oracle


def test_a_weak_signal_end_to_end(hd, weak_inputs):
    iq, sent, oracle = weak_inputs
    S, n, calls = WEAK["S"], WEAK["n"], WEAK["calls"]
    eng = hd.Engine(n_streams=S, max_chunk=n, sampling_rate=WEAK["fs"], decimation=WEAK["D"], baud=300, rtty_bits=8, rtty_stops=2, lowpass_bw_hz=1500.0)
    clk = eng.clocked()
    ordinary = [[] for _ in range(S)]
    eng.on_sentence(lambda s, call, data, crc: ordinary[s].append(f"{call},{data}*{crc}"))
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        clk.push_engine()
    eng.flush()
    n_oracle = n_plain = n_all = 0
    for s in range(S):
        assert ordinary[s] == oracle[s], (s, ordinary[s], oracle[s])     # the engine's own chain is the oracle's
        got = clk.take_sentences(s)
        assert all(t in sent[s] for (_, _, t) in got), (s, got)
        assert all(t in sent[s] for t in ordinary[s])
        n_oracle += len(ordinary[s]); n_plain += len([1 for g in got if g[1] == 0]); n_all += len(got)
    n_sent = 7 * S                                                   # whole sentences inside 12 s
    print("weak signal: ordinary", n_oracle, "clocked plain", n_plain, "with repair", n_all, "of", n_sent)
    assert 2 * n_oracle < n_sent and n_plain >= n_oracle + 3 and n_all >= n_plain + 3
    assert eng.L.hd_engine_sentences_ok(eng.h) == n_oracle
    eng.close()


# ---------------------------------------------------------------- record ring overflow, guard words, errors

def test_record_ring_overflow_and_guard_words(hd):
    S = 9
    eng = hd.Engine(n_streams=S)
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    case = next(c for c in M.CASES if c[0] == "600_8n2")
    row = M.case_signal(case)                                        # 96000 samples: the sample ring wraps twice, 163 characters
    clk = eng.clocked(record_cap=16)
    ref = hd.HostClocked(fsd, 600, 8, 2, record_cap=16)
    for s in range(S):
        clk.set_modem(s, 600, 8, 2)
    for at in range(0, row.size, 4097):
        clk.push_host(np.tile(row[at:at + 4097], (S, 1)))
        ref.push(row[at:at + 4097])
    want_st, want = ref.stats(), ref.records()
    assert want_st["dropped"] > 100 and want.size == 16
    for s in range(S):
        st = clk.stats(s)
        assert (st["characters"], st["dropped"]) == (want_st["characters"], want_st["dropped"]), (s, st, want_st)
        assert clk.waiting(s) == 16
        if s in (0, S // 2, S - 1):
            assert eng.L.hd_debug_clocked_guards(clk.h, s) == 0
        assert clk.records(s).tobytes() == want.tobytes(), s
    eng.close()


def test_bad_parameters_and_null_arguments(hd):
    eng = hd.Engine(n_streams=2, sampling_rate=25600.0, decimation=64, baud=50, rtty_bits=7, lowpass_bw_hz=150.0)        # fsd = 400
    L = eng.L
    with pytest.raises(hd.HabdecError):
        eng.clocked(record_cap=8)
    with pytest.raises(hd.HabdecError):
        eng.clocked(repair_bits=17)
    c = eng.clocked()
    assert L.hd_clocked_set_modem(c.h, 0, 400 / 3.4, 8, 2, 0) == HD_ERR_UNSUPPORTED
    assert L.hd_clocked_set_modem(c.h, 0, 50.0, 5, 2, 0) == HD_ERR_UNSUPPORTED
    assert L.hd_clocked_set_modem(c.h, 0, 50.0, 8, 3, 0) == HD_ERR_UNSUPPORTED
    assert L.hd_clocked_set_modem(c.h, 2, 50.0, 8, 2, 0) == HD_ERR_INVALID
    assert L.hd_clocked_reset(c.h, 2) == HD_ERR_INVALID and L.hd_clocked_push_engine(None) == HD_ERR_INVALID
    rows = np.ones((2, 100), np.float32)
    assert L.hd_clocked_push_device(c.h, rows.ctypes.data, 100, None, 100) == HD_ERR_INVALID      # host memory is not device memory
    assert L.hd_clocked_push_host(c.h, None, 100, None, 100) == HD_ERR_INVALID
    n = np.array([101, 3], np.uint32)
    assert L.hd_clocked_push_host(c.h, rows.ctypes.data, 100, n.ctypes.data, 0) == HD_ERR_INVALID  # a row longer than the stride
    assert L.hd_clocked_records(c.h, 2, None, 0) == HD_ERR_INVALID and L.hd_clocked_stats(c.h, 0, None) == HD_ERR_INVALID
    assert L.hd_clocked_take_sentences(c.h, 0, None, 4) == HD_ERR_INVALID
    c.push_host(rows)
    assert c.stats(0)["samples"] == 100 and c.stats(1)["samples"] == 100          # the engine streams' own modem: 50 baud 7N2
    c.push_engine()                                                  # no call yet: adds nothing
    assert c.stats(0)["samples"] == 100 and c.take_sentences(0) == []
    eng.close()
