"""AX.25 AFSK on the GPU (hd_afsk_*, kernels/afsk.hip).

Behind the quantisation the modem is integer arithmetic: slot records, candidate records, frames and counters are compared byte for byte with the host
restatement (hd_host_afsk_*), which tests/test_afsk_host.py holds to the numpy model of the definition."""
import ctypes as C

import numpy as np
import pytest

import afsk_cases as K

pytestmark = pytest.mark.gpu
PUSHES = (1, 63, 64, 65, 4097)
HD_ERR_INVALID, HD_ERR_UNSUPPORTED, HD_ERR_CAPACITY = -1, -3, -4
FSD = 32000.0                                   # the decimated rate of a default engine


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def AF(hd):
    from habdec_amd import afsk
    return afsk


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def cases():
    return K.frame_cases()


def same_records(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------- slot kernel

# (baud, mark, space) at 32 kS/s: 8, 26.67, 106.67 and 2048 samples per bit.  The records are held to the restatement with the same modem, so a modem
# need not fit the signal.  The last stream has no modem.
SLOT_MODEMS = [K.FAST, K.BELL, K.HF, (15.625, 15999.0, 0.5), None]
N_SLOTS_TEST = 30000


@pytest.fixture(scope="module")
def slot_rows():
    rng = np.random.default_rng(43)
    out = []
    for s in range(len(SLOT_MODEMS)):
        row = (0.7 * rng.standard_normal(N_SLOTS_TEST)).astype(np.float32)
        row[5000:11000] = K.specials(row[5000:11000], seed=11 + s)          # NaN, +-Inf, +-4 and beyond
        row[20000:20006] = [np.nan, np.inf, -np.inf, 4.0, -4.0, 1e38]
        out.append(row)
    return out


def test_slot_records_of_push_host_and_push_device_equal_the_host_restatement(hd, AF, torch, slot_rows):
    """Every stream with its own modem in one launch; per push the sizes 1, 63, 64, 65 and 4097 in turn, shifted from stream to stream, one stream
    empty in every third push, one push longer than a chunk, one stream without a modem."""
    S = len(SLOT_MODEMS)
    eng = hd.Engine(n_streams=S)
    assert eng.L.hd_engine_decimated_rate(eng.h) == FSD
    from_host, from_dev = AF.Afsk(eng, max_push=10000), AF.Afsk(eng, max_push=10000)
    ref = []
    for s, m in enumerate(SLOT_MODEMS):
        if m is None:
            ref.append(None)
            continue
        from_host.set_modem(s, *m); from_dev.set_modem(s, *m)
        ref.append(AF.HostAfsk(FSD, *m, max_push=10000))
        for f in (from_host, from_dev):
            assert f.stats(s) == ref[s].stats(), s
    assert [r.stats()["W"] for r in ref if r] == [8, 27, 107, 2048]
    at, push, stride, compared = [0] * S, 0, 10000, 0
    while any(at[s] < N_SLOTS_TEST for s in range(S)):
        n = np.array([PUSHES[(push + 2 * s) % len(PUSHES)] for s in range(S)], np.uint32)
        if push == 4:
            n[:] = 9000 - np.arange(S) * 3                           # longer than a chunk: three launches
        if push % 3 == 0:
            n[push // 3 % S] = 0
        n = np.minimum(n, [N_SLOTS_TEST - at[s] for s in range(S)]).astype(np.uint32)
        slab = np.full((S, stride), np.nan, np.float32)
        before = [r.stats()["slots"] if r else 0 for r in ref]
        for s in range(S):
            slab[s, :n[s]] = slot_rows[s][at[s]:at[s] + n[s]]
            if ref[s]:
                ref[s].push(slab[s, :n[s]])
            at[s] += int(n[s])
        from_host.push_host(slab, n)
        d = torch.from_numpy(slab).cuda()
        from_dev.push_device(d.data_ptr(), stride, n)
        del d
        for what, f in (("host memory", from_host), ("device memory", from_dev)):
            for s in range(S):
                st = f.stats(s)
                if not ref[s]:
                    assert (st["F"], st["samples"], st["slots"]) == (0, 0, 0), (what, push, st)
                    continue
                want = ref[s].stats()
                assert (st["samples"], st["slots"]) == (want["samples"], want["slots"]), (what, push, s, st, want)
                k = want["slots"] - before[s]
                got, mine = f.debug_slots(s, before[s], k), ref[s].slots(before[s], k)
                assert same_records(got, mine), (what, push, s, int(n[s]), np.flatnonzero(got != mine)[:8])
                compared += k
        push += 1
    assert compared > 2 * N_SLOTS_TEST                               # (one stream at a slot per sample, twice)
    for s in range(S):
        want_cands = ref[s].candidates() if ref[s] else None         # (taking them empties the log)
        for f in (from_host, from_dev):
            assert f.debug_guards(s) == 0, s
            if ref[s]:
                assert f.stats(s) == ref[s].stats(), s
                assert same_records(f.debug_candidates(s), want_cands), s
    assert ref[0].stats()["flags"] > 0
    eng.close()


# ---------------------------------------------------------------- gate and frame kernel

def restated(AF, modem, params, row):
    """(frames, candidates, stats) of the restatement, the row in one piece: the cuts cannot matter."""
    h = AF.HostAfsk(FSD, *modem, **params)
    h.push(row)
    return h.take_frames(), h.candidates(), h.stats()


def feed(f, rows, pieces, take, torch=None):
    """Push rows (a list, None: the stream gets nothing) in pieces given by pieces(n) -> (start, stop) pairs over the longest row; take(s) after each."""
    S, longest = len(rows), max(r.size for r in rows if r is not None)
    for a, b in pieces(longest):
        n = np.array([0 if r is None else max(0, min(b, r.size) - a) for r in rows], np.uint32)
        slab = np.zeros((S, max(b - a, 1)), np.float32)
        for s, r in enumerate(rows):
            if n[s]:
                slab[s, :n[s]] = r[a:a + n[s]]
        if torch is None:
            f.push_host(slab, n)
        else:
            d = torch.from_numpy(slab).cuda()
            f.push_device(d.data_ptr(), slab.shape[1], n)
            del d
        for s in range(S):
            take(s)


def test_candidates_frames_and_counters_equal_the_host_restatement(hd, AF, torch, cases):
    """The host test's frame cases, a stream each: pushed through host memory in pieces of max_push and through device memory in pieces of 1, 63, 64, 65
    and 4097 samples in turn, so that opening flag, body and closing flag fall into different pushes; one stream takes its slot ring round."""
    names = [n for n in sorted(cases) if cases[n][1] == K.SMALL]
    assert {"ring_wrap", "shared_flag", "hf_300_baud", "repair_2", "false_closing_flag", "repair_refused_callsign", "abort_inside", "open_walk"} <= set(names)
    others = [n for n in sorted(cases) if n not in names]
    assert others == ["max_332", "plain_bad_callsign_allowed", "repair_off"]
    S = len(names)
    eng = hd.Engine(n_streams=S)
    want = {n: restated(AF, *cases[n][:3]) for n in cases}
    whole = lambda n: [(a, min(a + 8192, n)) for a in range(0, n, 8192)]
    cut = lambda n: list(K.cuts(n, PUSHES))

    def run(params, rows, pieces, dev):
        f = AF.Afsk(eng, **params)
        frames, cands = [[] for _ in range(S)], [[] for _ in range(S)]
        for s, name in enumerate(rows):
            if name:
                f.set_modem(s, *cases[name][0])

        def take(s):
            frames[s] += f.take_frames(s)
            cands[s].append(f.debug_candidates(s))
        feed(f, [cases[n][2] if n else None for n in rows], pieces, take, torch if dev else None)
        for s, name in enumerate(rows):
            if not name:
                assert f.stats(s)["samples"] == 0
                continue
            w_frames, w_cands, w_stats = want[name]
            got = np.concatenate(cands[s])
            assert same_records(got, w_cands), (name, dev, got.size, w_cands.size, [(int(c["slot"]), int(c["result"])) for c in got[:6]], [(int(c["slot"]), int(c["result"])) for c in w_cands[:6]])
            assert frames[s] == w_frames, (name, dev)
            assert f.stats(s) == w_stats, (name, dev, f.stats(s), w_stats)
            assert [(fr["data"], fr["flips"]) for fr in frames[s]] == cases[name][3], (name, dev)
            assert f.waiting(s) == 0 and f.debug_guards(s) == 0
        f.close()

    run(K.SMALL, names, whole, False)
    run(K.SMALL, names, cut, True)
    assert want["ring_wrap"][0][0]["slot"] > 65536 and want["ring_wrap"][2]["slots"] > 65536
    for name in others:                                              # each with parameters of its own, on stream 1 of the same engine
        rows = [None] * S
        rows[1] = name
        run(cases[name][1], rows, cut if name == "max_332" else whole, name != "repair_off")
    eng.close()


def test_a_scan_with_more_candidates_than_a_launch_holds(hd, AF):
    """64 streams of the same row of nothing but flags at 8 samples a bit, frames of at most 17 bytes (L = 172 bits): a push of 8192 samples decides
    about 700 flags a stream, 45000 in the scan, eleven launches of the frame kernel.  Every stream must equal the restatement of the one row."""
    S, params = 64, dict(max_frame_bytes=17, max_push=8192)
    row = K.row_of(K.nrzi(K.FLAG * 340), K.FAST, params, start=40.0)
    assert 22000 < row.size < 24576
    w_frames, w_cands, w_stats = restated(AF, K.FAST, params, row)
    assert 1500 < w_stats["flags"] < 16384 and w_frames == []
    eng = hd.Engine(n_streams=S)
    f = AF.Afsk(eng, **params)
    for s in range(S):
        f.set_modem(s, *K.FAST)
    for a in range(0, row.size, 8192):
        f.push_host(np.ascontiguousarray(np.tile(row[a:a + 8192], (S, 1))))
    assert S * w_stats["flags"] > 3 * 8 * 4096                       # eight times what a launch holds in each of the three pushes
    for s in range(S):
        assert f.stats(s) == w_stats, s
        assert same_records(f.debug_candidates(s), w_cands), s
        assert f.waiting(s) == 0 and f.debug_guards(s) == 0
    eng.close()


# ---------------------------------------------------------------- through an engine

# Chosen on the CPU with the oracle's chain on the same IQ and the numpy model on its discriminator row: a low-pass of 11 kHz (the engine's width is the
# two-sided one: +-(3 kHz deviation + 2.2 kHz)) gives a clean row with a peak of 0.85; at sigma 3.9, seed 3, the model loses one frame and gets the
# other with one flip (below sigma 3.6 both decode plain, above 4.2 both are lost).
E2E_LOWPASS, E2E_SIGMA, E2E_SEED = 11000.0, 3.9, 3


def test_push_engine_end_to_end(hd, AF):
    fs, n, S = 2.048e6, 65536, 3
    f1 = K.ui_frame(b">balloon 1 up")
    f2 = K.ui_frame(b"!4903.50N/07201.75W-", src="W1AW", ssid=7, digis=(("WIDE2", 1, True),))
    lv = K.nrzi(K.on_air([f1, f2], before=12, between=6, after=3))
    params = dict(max_frame_bytes=64)
    calls = int(np.ceil((4000 * 64 + (len(lv) + 623 + 40) * fs / 1200) / n))
    audio = AF.afsk_audio(lv, fs, start=4000 * 64.0, n_samples=calls * n)
    iq = np.stack([AF.fm_iq(audio, fs, 3000.0, 0.5, offset=500.0),
                   AF.fm_iq(audio, fs, 3000.0, 0.5, offset=500.0, sigma=E2E_SIGMA, seed=E2E_SEED),
                   AF.fm_iq(np.zeros_like(audio), fs, amplitude=0.0, sigma=1.0, seed=4)])
    eng = hd.Engine(n_streams=S)
    assert eng.L.hd_engine_decimated_rate(eng.h) == FSD
    a = AF.Afsk(eng, **params)
    ref = [AF.HostAfsk(FSD, *K.BELL, **params) for _ in range(S)]
    for s in range(S):
        eng.set_lowpass_bw(s, E2E_LOWPASS)
        a.set_bell202(s)
    got = [[] for _ in range(S)]
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        a.push_engine()
        if k in (0, 5):
            a.push_engine()                                          # a second push without a call in between changes nothing
        for s in range(S):
            ref[s].push(eng.demodulated(s))
            got[s] += a.take_frames(s)
    assert [fr["data"] for fr in got[0]] == [f1[:-2], f2[:-2]] and [fr["flips"] for fr in got[0]] == [0, 0]
    assert [AF.ax25_format(fr["data"]) for fr in got[0]] == ["N0CALL-11>APRS:>balloon 1 up", "W1AW-7>APRS,WIDE2-1*:!4903.50N/07201.75W-"]
    assert got[2] == []
    for s in range(S):
        assert got[s] == ref[s].take_frames() and a.stats(s) == ref[s].stats(), s
        assert same_records(a.debug_candidates(s), ref[s].candidates()), s
        assert a.stats(s)["samples"] == calls * n // 64 and a.debug_guards(s) == 0
    print("stream 1:", [(fr["flips"], AF.ax25_format(fr["data"])) for fr in got[1]], a.stats(1))
    assert all(fr["data"] in (f1[:-2], f2[:-2]) for fr in got[1])
    eng.close()


# ---------------------------------------------------------------- lifecycle and errors

def test_reset_set_modem_destroy_and_the_error_codes(hd, AF, cases):
    eng, other = hd.Engine(n_streams=3), hd.Engine(n_streams=3)
    L = eng.L
    for bad in (dict(max_frame_bytes=16), dict(max_frame_bytes=333), dict(repair_flips=5), dict(repair_bits=11), dict(max_push=40000)):
        with pytest.raises(hd.HabdecError):
            AF.Afsk(eng, **bad)
    f = AF.Afsk(eng, max_push=5000, max_frame_bytes=64)
    sm = lambda s, baud, mark, space: L.hd_afsk_set_modem(f.h, s, baud, mark, space)
    assert sm(0, FSD / 7.99, 1200.0, 2200.0) == HD_ERR_UNSUPPORTED and sm(0, FSD / 2048.1, 1200.0, 2200.0) == HD_ERR_UNSUPPORTED
    assert sm(0, FSD / 8, 1200.0, 2200.0) == 0 and sm(0, FSD / 2048, 1200.0, 2200.0) == 0
    for mark, space in ((0.0, 2200.0), (1200.0, 16000.0), (1700.0, 1700.0), (-1200.0, 2200.0)):
        assert sm(0, 1200.0, mark, space) == HD_ERR_INVALID
    assert sm(3, 1200.0, 1200.0, 2200.0) == HD_ERR_INVALID and L.hd_afsk_set_bell202(f.h, 3) == HD_ERR_INVALID
    assert L.hd_afsk_take_frames(f.h, 3, None, 0) == HD_ERR_INVALID and L.hd_afsk_stats(f.h, 0, None) == HD_ERR_INVALID
    assert L.hd_afsk_push_engine(None) == HD_ERR_INVALID and L.hd_afsk_reset(f.h, 3) == HD_ERR_INVALID
    # a push above max_push is refused whole; a stream without a modem is passed by in front of that test; rows of another kind of memory are refused
    f.set_bell202(0); f.set_modem(1, *K.HF)
    rows = np.zeros((3, 6000), np.float32)
    assert L.hd_afsk_push_host(f.h, rows.ctypes.data, 6000, np.array([100, 5001, 0], np.uint32).ctypes.data, 0) == HD_ERR_CAPACITY
    assert f.stats(0)["samples"] == 0
    assert L.hd_afsk_push_device(f.h, rows.ctypes.data, 6000, np.array([100, 100, 0], np.uint32).ctypes.data, 0) == HD_ERR_INVALID
    assert L.hd_afsk_push_host(f.h, rows.ctypes.data, 50, None, 100) == HD_ERR_INVALID      # a row longer than the stride
    f.push_host(rows, np.array([100, 5000, 6000], np.uint32))
    assert [f.stats(s)["samples"] for s in range(3)] == [100, 5000, 0]
    # A foreign engine: no door of hd_afsk takes another object (the clocked decoder's push_tones and the tracker's attach do, and refuse one of another
    # engine), so there is no error code to assert here.  What there is to show: push_engine reads the object's own engine -- this one has had no call.
    g = AF.Afsk(other, max_frame_bytes=64)
    g.set_bell202(0)
    g.push_engine()
    assert g.stats(0)["samples"] == 0
    # reset restarts a stream; set_modem resets only its own
    modem, params, row, expect = cases["plain"]
    want = restated(AF, modem, dict(max_frame_bytes=64, max_push=5000), row)
    f.reset(0)
    assert f.stats(0)["samples"] == 0 and f.stats(1)["samples"] == 5000 and f.stats(0)["W"] == 27
    feed(f, [row, None, None], lambda n: [(a, min(a + 5000, n)) for a in range(0, n, 5000)], lambda s: None)
    got = f.take_frames(0)
    assert [(fr["data"], fr["flips"]) for fr in got] == expect and got == want[0] and f.stats(0) == want[2]
    f.set_bell202(1)
    assert f.stats(1)["samples"] == 0 and f.stats(1)["W"] == 27 and f.stats(0)["samples"] == row.size
    feed(f, [None, row, None], lambda n: [(a, min(a + 5000, n)) for a in range(0, n, 5000)], lambda s: None)
    assert f.take_frames(1) == got
    f.reset()
    assert all(f.stats(s)["samples"] == 0 and f.stats(s)["frames_plain"] == 0 for s in range(3)) and f.stats(0)["W"] == 27
    for s in range(3):
        assert f.debug_guards(s) == 0
    # destroyed before the engine, by hand and by the engine's close
    h = AF.Afsk(eng)
    h.close()
    eng.close(); other.close()
    assert f.h is None
