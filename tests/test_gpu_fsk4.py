"""Horus Binary 4FSK on the GPU (hd_fsk4_*, kernels/fsk4.hip).

Behind the quantisation the modem is integer arithmetic: slot records, candidate records, frames and counters are compared byte for byte with the host
restatement (hd_host_fsk4_*), which tests/test_fsk4_host.py holds to the numpy model of the definition."""
import numpy as np
import pytest

import fsk4_model as FM
import tones_model as TM

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
def F4(hd):
    from habdec_amd import fsk4
    return fsk4


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def same_records(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------- slot kernel

# (baud, f0, spacing, preset) at 32 kS/s: 8, 2048 and 704.07 samples per symbol; tones around 0, all negative, at the band's edges, one at 0.  The records
# are held to the restatement with the same modem, so a modem need not fit the signal.  The last stream has no modem.
SLOT_MODEMS = [(4000.0, -6000.0, 4000.0, 1), (15.625, -1500.0, 270.0, 2), (45.45, -15999.99, 10666.66, 1), (4000.0, 0.0, 4000.0, 2), None]
N_SLOTS_TEST = 30000


@pytest.fixture(scope="module")
def slot_iq():
    rng = np.random.default_rng(41)
    out = []
    for s in range(len(SLOT_MODEMS)):
        iq = (0.5 * (rng.standard_normal(N_SLOTS_TEST) + 1j * rng.standard_normal(N_SLOTS_TEST))).astype(np.complex64)
        iq[:TM.specials_iq().size // 4] += TM.specials_iq(seed=11 + s)[:TM.specials_iq().size // 4]        # NaN, Inf, +-8 and beyond
        iq[5000:5000 + 6000] = TM.specials_iq(seed=31 + s)
        out.append(iq)
    return out


def test_slot_records_of_push_host_and_push_device_equal_the_host_restatement(hd, F4, torch, slot_iq):
    """Every stream with its own modem in one launch; per push the sizes 1, 63, 64, 65 and 4097 in turn, shifted from stream to stream, one stream
    empty in every third push, one push longer than a chunk, one stream without a modem."""
    S = len(SLOT_MODEMS)
    eng = hd.Engine(n_streams=S)
    assert eng.L.hd_engine_decimated_rate(eng.h) == FSD
    from_host, from_dev = F4.Fsk4(eng, max_push=10000), F4.Fsk4(eng, max_push=10000)
    ref = []
    for s, m in enumerate(SLOT_MODEMS):
        if m is None:
            ref.append(None)
            continue
        baud, f0, spacing, preset = m
        from_host.set_modem(s, baud, f0, spacing, preset); from_dev.set_modem(s, baud, f0, spacing, preset)
        ref.append(F4.HostFsk4(FSD, baud, f0, spacing, preset, max_push=10000))
        want = FM.modem(FSD, baud, f0, spacing)
        for f in (from_host, from_dev):
            st = f.stats(s)
            assert (st["F"], st["W"], st["step"], st["samples"], st["slots"]) == (want["F"], want["W"], want["step"], 0, 0), (s, st, want)
    assert sorted(r.stats()["W"] for r in ref if r) == [8, 8, 704, 2048]
    at, push, stride, compared = [0] * S, 0, 10000, 0
    while any(at[s] < N_SLOTS_TEST for s in range(S)):
        n = np.array([PUSHES[(push + 2 * s) % len(PUSHES)] for s in range(S)], np.uint32)
        if push == 4:
            n[:] = 9000 - np.arange(S) * 3                           # longer than a chunk: three launches
        if push % 3 == 0:
            n[push // 3 % S] = 0
        n = np.minimum(n, [N_SLOTS_TEST - at[s] for s in range(S)]).astype(np.uint32)
        slab = np.full((S, stride), np.nan + 1j * np.nan, np.complex64)
        before = [r.stats()["slots"] if r else 0 for r in ref]
        for s in range(S):
            slab[s, :n[s]] = slot_iq[s][at[s]:at[s] + n[s]]
            if ref[s]:
                ref[s].push(slab[s, :n[s]])
            at[s] += int(n[s])
        from_host.push_host(slab, n)
        d = torch.from_numpy(slab.view(np.float32)).cuda()
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
                assert same_records(got, mine), (what, push, s, int(n[s]), np.flatnonzero((got != mine).any(axis=1))[:8])
                compared += k
        push += 1
    assert compared > 2 * 2 * N_SLOTS_TEST                           # (two streams at a slot per sample, twice)
    for s in range(S):
        for f in (from_host, from_dev):
            assert f.debug_guards(s) == 0, s
            if ref[s]:
                assert {k: v for k, v in f.stats(s).items()} == ref[s].stats(), s
    eng.close()


# ---------------------------------------------------------------- frame kernel

BAUD8, F0, SPACING = 4000.0, -6000.0, 4000.0    # 8 samples per symbol: a V1 frame is 1440 samples, a V2 frame 2080
CUTS = [4097, 1, 63, 64, 65, 4097, 63, 1, 64, 65, 3420]             # 12000 samples; the V2 frame of stream 1 ends with the fifth push, at 4290
N_FRAMES_TEST = sum(CUTS)


def frame_streams():
    """(iq, preset, the payloads that must be delivered) per stream."""
    def tx(payload, fr, **kw):
        return FM.symbols(FM.encode(payload, fr, **kw))

    out = []
    noise = dict(sigma=0.05)
    # 0: two V1 frames back to back
    p = [FM.make_payload(FM.V1, 1), FM.make_payload(FM.V1, 2)]
    out.append((FM.fsk4_iq(np.concatenate([tx(p[0], FM.V1), tx(p[1], FM.V1)]), FSD, BAUD8, F0, SPACING, seed=1, start=2003.0, n_samples=N_FRAMES_TEST, **noise), 1, p))
    # 1: a V2 frame that ends exactly at a push boundary
    p = [FM.make_payload(FM.V2, 3)]
    out.append((FM.fsk4_iq(tx(p[0], FM.V2), FSD, BAUD8, F0, SPACING, seed=2, start=float(sum(CUTS[:5]) - 2080), n_samples=N_FRAMES_TEST, **noise), 2, p))
    # 2: three wrong bits in every third codeword of a V1 frame: hard corrections
    p = [FM.make_payload(FM.V1, 4)]
    flips = [(k, b) for k in range(0, 15, 3) for b in (1, 9, 17)]
    out.append((FM.fsk4_iq(tx(p[0], FM.V1, flips=flips), FSD, BAUD8, F0, SPACING, seed=3, start=5000.0, n_samples=N_FRAMES_TEST, **noise), 1, p))
    # 3: four wrong bits in one codeword of a V2 frame, two of them on symbols the receiver is unsure of: a soft correction
    p = [FM.make_payload(FM.V2, 5)]
    iq, _ = soft_case(p[0], seed=4, start=7001.0, n_samples=N_FRAMES_TEST, **noise)
    out.append((iq, 2, p))
    # 4: noise alone
    out.append((FM.fsk4_iq([], FSD, BAUD8, F0, SPACING, sigma=0.5, seed=5, n_samples=N_FRAMES_TEST), 1, []))
    return out


def soft_case(payload, **kw):
    """A V2 frame with four wrong bits in codeword 5: bits 2 and 7 plainly, bits 13 and 20 on symbols sent as 65 % the wrong tone and 35 % the right
    one.  Hard decoding finds the codeword three bits away and fails the CRC; with the soft values the true codeword costs two sure bits and two unsure
    ones against three sure ones.  Also the symbols that carry the unsure bits."""
    fr = FM.V2
    right = FM.symbols(FM.encode(payload, fr, flips=[(5, 2), (5, 7)]))
    wrong = FM.symbols(FM.encode(payload, fr, flips=[(5, 2), (5, 7), (5, 13), (5, 20)]))
    at = [int(m) for m in np.flatnonzero(right != wrong)]
    assert len(at) == 2
    return FM.fsk4_iq(wrong, FSD, BAUD8, F0, SPACING, alt={m: (int(right[m]), 0.35) for m in at}, **kw), at


def test_candidates_frames_and_counters_equal_the_host_restatement(hd, F4, torch):
    streams = frame_streams()
    S = len(streams)
    eng = hd.Engine(n_streams=S)
    f = F4.Fsk4(eng, max_push=4097)
    ref = []
    for s, (_, preset, _) in enumerate(streams):
        f.set_modem(s, BAUD8, F0, SPACING, preset)
        ref.append(F4.HostFsk4(FSD, BAUD8, F0, SPACING, preset))
        ref[s].push(streams[s][0])                                   # in one piece: the cuts cannot matter
    at, got_frames, got_cands = 0, [[] for _ in range(S)], [[] for _ in range(S)]
    for n in CUTS:
        slab = np.ascontiguousarray(np.stack([iq[at:at + n] for iq, _, _ in streams]))
        f.push_host(slab)
        at += n
        for s in range(S):
            got_frames[s] += f.take_frames(s)
            got_cands[s].append(f.debug_candidates(s))
    f.scan()                                                         # nothing is left to decide
    launches_needed = S * 4097 > 16384                               # the sixth push decides 4097 candidates of every stream: more than one launch holds
    assert launches_needed
    for s, (_, preset, payloads) in enumerate(streams):
        want_frames, want_cands, want = ref[s].take_frames(), ref[s].candidates(), ref[s].stats()
        cands = np.concatenate(got_cands[s])
        assert same_records(cands, want_cands), (s, cands.size, want_cands.size)
        assert got_frames[s] == want_frames, (s, got_frames[s], want_frames)
        assert f.stats(s) == want, (s, f.stats(s), want)
        assert [fr["payload"] for fr in got_frames[s]] == payloads, (s, got_frames[s])
        assert f.waiting(s) == 0 and f.debug_guards(s) == 0
        print("stream", s, {k: want[k] for k in ("candidates", "gate_passes", "crc_failures", "refused", "overlaps", "frames")},
              [(fr["slot"], fr["corrected"], fr["uw_errors"]) for fr in got_frames[s]])
    assert [fr["corrected"] for fr in got_frames[2]] == [15] and [fr["corrected"] for fr in got_frames[3]] == [4]
    noise = f.stats(4)
    assert noise["gate_passes"] > 0 and noise["frames"] == 0 and noise["candidates"] == N_FRAMES_TEST - 7 - 8 * 179
    # without the soft values four errors are beyond the code: at chase_bits = 0 the candidate at the frame's own slot fails its CRC (a neighbouring
    # timing phase, where a neighbour symbol leaks into an unsure one, may still get through)
    soft_at = [c for c in np.concatenate(got_cands[3]) if c["slot"] == 7001]
    assert len(soft_at) == 1 and soft_at[0]["crc_ok"] == 1 and soft_at[0]["corrected"] == 4
    hard = F4.Fsk4(eng, max_push=4097, chase_bits=0)
    hard.set_modem(3, BAUD8, F0, SPACING, 2)
    for k in range(0, N_FRAMES_TEST, 4000):
        slab = np.zeros((S, 4000), np.complex64)
        slab[3] = streams[3][0][k:k + 4000]
        hard.push_host(slab)
    ref_hard = F4.HostFsk4(FSD, BAUD8, F0, SPACING, 2, chase_bits=0)
    ref_hard.push(streams[3][0])
    hard_cands = hard.debug_candidates(3)
    assert same_records(hard_cands, ref_hard.candidates()) and hard.take_frames(3) == ref_hard.take_frames() and hard.stats(3) == ref_hard.stats()
    hard_at = [c for c in hard_cands if c["slot"] == 7001]
    assert len(hard_at) == 1 and hard_at[0]["crc_ok"] == 0
    eng.close()


# ---------------------------------------------------------------- through an engine

def test_push_engine_delivers_the_payloads_and_equals_the_restatement(hd, F4):
    """1000-baud 4FSK at 2.048 MS/s through an engine at /64: 32 samples per symbol, six calls of 65536 samples."""
    fs, n, calls, S = 2.048e6, 65536, 6, 2
    baud, f0, spacing = 1000.0, -3000.0, 2000.0
    payloads = [FM.make_payload(FM.V1, 10 + s) for s in range(S)]
    iq = np.stack([FM.fsk4_iq(FM.symbols(FM.encode(payloads[s], FM.V1)), fs, baud, f0, spacing, sigma=0.1, seed=20 + s, start=4000.0 + 1500 * s, n_samples=n * calls)
                   for s in range(S)])
    eng = hd.Engine(n_streams=S, max_chunk=n, sampling_rate=fs, decimation=64)
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    assert fsd == 32000.0
    f = F4.Fsk4(eng)
    ref = [F4.HostFsk4(fsd, baud, f0, spacing, 1) for _ in range(S)]
    for s in range(S):
        f.set_modem(s, baud, f0, spacing, 1)
    got = [[] for _ in range(S)]
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        f.push_engine()
        if k in (0, 3):
            f.push_engine()                                          # a second push without a call in between changes nothing
        for s in range(S):
            ref[s].push(eng.decimated(s))
            got[s] += f.take_frames(s)
    for s in range(S):
        assert [fr["payload"] for fr in got[s]] == [payloads[s]], (s, got[s])
        assert got[s] == ref[s].take_frames() and f.stats(s) == ref[s].stats(), s
        assert same_records(f.debug_candidates(s), ref[s].candidates())
        assert f.stats(s)["samples"] == calls * n // 64 and f.debug_guards(s) == 0
    eng.close()


# ---------------------------------------------------------------- lifecycle and errors

def test_reset_set_modem_destroy_and_the_error_codes(hd, F4):
    eng = hd.Engine(n_streams=3)
    L = eng.L
    for bad in (dict(window_q8=31), dict(window_q8=257), dict(uw_max_errors=5), dict(chase_bits=7), dict(max_push=(1 << 22) + 1)):
        with pytest.raises(hd.HabdecError):
            F4.Fsk4(eng, **bad)
    f = F4.Fsk4(eng, max_push=5000)
    v1, v2 = F4.frame(1), F4.frame(2)
    import ctypes as C
    sm = lambda s, baud, f0, sp, fr: L.hd_fsk4_set_modem(f.h, s, baud, f0, sp, C.byref(fr))
    assert sm(0, FSD / 7.99, 0.0, 100.0, v1) == HD_ERR_UNSUPPORTED and sm(0, FSD / 2048.1, 0.0, 100.0, v1) == HD_ERR_UNSUPPORTED
    assert sm(0, FSD / 8, 0.0, 100.0, v1) == 0 and sm(0, FSD / 2048, 0.0, 100.0, v1) == 0
    for field, value in (("payload_bytes", 33), ("payload_bytes", 2), ("interleave_mul", 336), ("interleave_mul", 0), ("scrambler_seed", 0),
                         ("scrambler_seed", 0x8000), ("golay_poly", 0xC76), ("golay_poly", 0x475)):
        assert sm(0, 4000.0, 0.0, 100.0, F4.frame(1, **{field: value})) == HD_ERR_UNSUPPORTED, (field, value)
    assert sm(0, 4000.0, 0.0, 100.0, F4.frame(1, golay_poly=0xAE3)) == 0                # the other generator of the code
    assert sm(0, 4000.0, 4000.0, 4000.0, v1) == HD_ERR_INVALID and sm(0, 4000.0, -16000.0, 100.0, v1) == HD_ERR_INVALID
    assert sm(3, 4000.0, 0.0, 100.0, v1) == HD_ERR_INVALID and L.hd_fsk4_set_modem(f.h, 0, 4000.0, 0.0, 100.0, None) == HD_ERR_INVALID
    assert L.hd_fsk4_take_frames(f.h, 3, None, 0) == HD_ERR_INVALID and L.hd_fsk4_stats(f.h, 0, None) == HD_ERR_INVALID
    assert L.hd_fsk4_push_engine(None) == HD_ERR_INVALID and L.hd_fsk4_scan(None) == HD_ERR_INVALID
    # a push above max_push is refused whole; a stream without a modem is passed by in front of that test
    f.set_modem(0, BAUD8, F0, SPACING, 1); f.set_modem(1, BAUD8, F0, SPACING, 2)
    rows = np.zeros((3, 6000), np.complex64)
    assert L.hd_fsk4_push_host(f.h, rows.ctypes.data, 6000, np.array([100, 5001, 0], np.uint32).ctypes.data, 0) == HD_ERR_CAPACITY
    assert f.stats(0)["samples"] == 0
    f.push_host(rows, np.array([100, 5000, 6000], np.uint32))
    assert [f.stats(s)["samples"] for s in range(3)] == [100, 5000, 0]
    # reset restarts a stream; set_modem resets only its own
    p = FM.make_payload(FM.V1, 7)
    iq = FM.fsk4_iq(FM.symbols(FM.encode(p, FM.V1)), FSD, BAUD8, F0, SPACING, sigma=0.05, seed=9, start=333.0, n_samples=3300)
    rows = np.zeros((3, 3300), np.complex64)
    rows[0] = rows[1] = iq
    f.reset(0)
    assert f.stats(0)["samples"] == 0 and f.stats(1)["samples"] == 5000 and f.stats(0)["F"] == 8 << 16
    f.push_host(rows, np.array([3300, 0, 0], np.uint32))
    ref = F4.HostFsk4(FSD, BAUD8, F0, SPACING, 1)
    ref.push(iq)
    got = f.take_frames(0)
    assert [fr["payload"] for fr in got] == [p] and got == ref.take_frames() and f.stats(0) == ref.stats()
    f.set_modem(1, BAUD8, F0, SPACING, 1)
    assert f.stats(1)["samples"] == 0 and f.stats(1)["symbols"] == 180 and f.stats(0)["samples"] == 3300
    f.push_host(rows, np.array([0, 3300, 0], np.uint32))
    assert f.take_frames(1) == got
    f.reset()
    assert all(f.stats(s)["samples"] == 0 and f.stats(s)["frames"] == 0 for s in range(3)) and f.stats(0)["F"] == 8 << 16
    # destroyed before the engine, by hand and by the engine's close
    g = F4.Fsk4(eng)
    g.close()
    eng.close()
    assert f.h is None
