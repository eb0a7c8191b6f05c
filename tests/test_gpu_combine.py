"""The diversity combiner on the GPU (hd_combine_*, kernels/combine.hip).

Behind the quantisation the combiner is integer arithmetic: rows, scores and results are compared byte for byte with the host restatement
(hd_host_combine_*), which tests/test_combine_host.py holds to the numpy model of the definition."""
import ctypes as C

import numpy as np
import pytest

import combine_model as CM
import tones_model as TM
from habdec_amd import synth

pytestmark = pytest.mark.gpu
HD_OK, HD_ERR_INVALID, HD_ERR_UNSUPPORTED, HD_ERR_CAPACITY = 0, -1, -3, -4
NO_GROUP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    import habdec_amd.combine
    return habdec_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


# ---------------------------------------------------------------- k_combine against the host restatement, through three doors

S = 8
GROUPS = ([0, 1, 2], [3, 4, 5, 6])                           # stream 7 is in no group
# rows of 4095, 4096, 4097 and 8193 samples: the chunk's edges; 40000 samples in all: the rings wrap under a delay of 8192
SIZES = [4095, 4096, 4097, 8193, 1, 63, 64, 65, 8193, 8193, 2940]
FIRST = (([0, 8192, 63], [256, 255, 1]), ([4095, 0, 64, 1], [0, 256, 256, 128]))
SECOND = (([8192, 0, 1], [0, 0, 0]), ([0, 8192, 4095, 63], [256, 1, 255, 256]))        # from push 5 on; the first group's weights sum to 0
CHANGE_AT = 5


@pytest.fixture(scope="module")
def float_rows():
    assert sum(SIZES) == 40000
    return CM.random_rows(S, 40000, 60)


def settle(comb, refs, part):
    for g, ref, (delays, weights) in zip(GROUPS, refs, part):
        for m, s in enumerate(g):
            comb.set_delay(s, delays[m]); comb.set_weight(s, weights[m])
            ref.set_delay(m, delays[m]); ref.set_weight(m, weights[m])


@pytest.mark.parametrize("door", ["device", "host", "tones"])
def test_rows_equal_the_host_restatement(hd, torch, float_rows, door):
    eng = hd.Engine(n_streams=S)                                     # fsd = 32 kS/s
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    comb = hd.combine.Combiner(eng, max_push=8193)
    refs = [hd.combine.HostCombiner(g) for g in GROUPS]
    for g in GROUPS:
        comb.set_group(g)
    if door == "tones":
        tones = eng.tones(max_push=8193)
        host_tones = []
        for s in range(S - 1):                                       # (stream 7: no modem, a row of length 0)
            tones.set_modem(s, 300.0, 250.0, -250.0)
            host_tones.append(hd.HostTones(fsd, 300.0, 250.0, -250.0))
        iq = CM.random_rows(S, 80000, 61).view(np.complex64)
    settle(comb, refs, FIRST)
    at = 0
    for push, n in enumerate(SIZES):
        if push == CHANGE_AT:
            settle(comb, refs, SECOND)
        n_arr = np.full(S, n, np.uint32)
        if door == "tones":
            slab = np.ascontiguousarray(iq[:, at:at + n])
            tones.push_host(slab, n_arr)
            rows = np.zeros((S, n), np.float32)
            for s in range(S - 1):
                rows[s] = host_tones[s].push(slab[s])
            ptr, stride, lens = tones.rows()
            assert lens.tolist() == [n] * (S - 1) + [0]
            comb.push_device(ptr, stride, lens)
        else:
            rows = np.ascontiguousarray(float_rows[:, at:at + n])
            if door == "host":
                comb.push_host(rows, n_arr)
            else:
                d = torch.from_numpy(rows).cuda()
                comb.push_device(d.data_ptr(), n, n_arr)
                del d
        at += n
        assert comb.rows()[2].tolist() == [n, 0, 0, n, 0, 0, 0, 0], (door, push)
        for g, ref in zip(GROUPS, refs):
            want = ref.push(rows[g])
            got = comb.output(g[0])
            assert got.tobytes() == want.tobytes(), (door, push, n, g[0], np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
            assert all(comb.output(s).size == 0 for s in g[1:])
    for g, part in zip(GROUPS, SECOND):
        for m, s in enumerate(g):
            st = comb.stats(s)
            assert (st["samples"], st["group"], st["delay"], st["weight"], st["members"]) == (40000, g[0], part[0][m], part[1][m], len(g)), (door, s, st)
    assert comb.stats(7) == dict(samples=0, group=NO_GROUP, delay=0, weight=0, members=0) and comb.output(7).size == 0
    assert all(comb.debug_guards(s) == 0 for s in range(S))
    # reset of one group: counts start again, delays and weights stay
    comb.reset(3)
    refs[1].reset()
    assert comb.stats(4)["samples"] == 0 and comb.stats(4)["delay"] == SECOND[1][0][1] and comb.stats(0)["samples"] == 40000 and comb.rows()[2][3] == 0
    rows = np.ascontiguousarray(float_rows[:, :700])
    comb.push_host(rows, np.array([0, 0, 0, 700, 700, 700, 700, 9], np.uint32))
    assert comb.output(3).tobytes() == refs[1].push(rows[GROUPS[1]]).tobytes() and comb.output(0).size == 0 and comb.stats(0)["samples"] == 40000
    assert all(comb.debug_guards(s) == 0 for s in range(S))
    eng.close()


def test_groups_and_errors(hd):
    eng = hd.Engine(n_streams=10)
    comb = hd.combine.Combiner(eng, max_push=100)
    L = eng.L
    u = lambda *a: np.array(a, np.uint32)
    assert L.hd_combine_set_group(comb.h, np.arange(9, dtype=np.uint32).ctypes.data, 9) == HD_ERR_INVALID           # a ninth member
    assert L.hd_combine_set_group(comb.h, u(1, 2, 1).ctypes.data, 3) == HD_ERR_INVALID                               # a duplicate stream
    assert L.hd_combine_set_group(comb.h, u(1, 10).ctypes.data, 2) == HD_ERR_INVALID and L.hd_combine_set_group(comb.h, None, 2) == HD_ERR_INVALID
    assert L.hd_combine_set_group(None, u(1).ctypes.data, 1) == HD_ERR_INVALID
    assert L.hd_combine_set_delay(comb.h, 1, 0) == HD_ERR_INVALID                                                     # in no group
    comb.set_group([1, 2, 3]); comb.set_group([4, 5])
    assert L.hd_combine_set_delay(comb.h, 2, 8193) == HD_ERR_INVALID and L.hd_combine_set_delay(comb.h, 2, 8192) == HD_OK
    assert L.hd_combine_set_weight(comb.h, 2, 257) == HD_ERR_INVALID and L.hd_combine_set_weight(comb.h, 2, 255) == HD_OK
    rows = np.ones((10, 100), np.float32)
    before = [comb.stats(s)["samples"] for s in range(10)]
    n = np.full(10, 50, np.uint32); n[5] = 49
    assert L.hd_combine_push_host(comb.h, rows.ctypes.data, 100, n.ctypes.data, 0) == HD_ERR_INVALID                 # unequal lengths within a group
    assert [comb.stats(s)["samples"] for s in range(10)] == before and comb.rows()[2].tolist() == [0] * 10         # nothing launched or counted, in any group
    long = np.ones((10, 101), np.float32)
    assert L.hd_combine_push_host(comb.h, long.ctypes.data, 101, None, 101) == HD_ERR_CAPACITY
    assert L.hd_combine_push_device(comb.h, rows.ctypes.data, 100, None, 100) == HD_ERR_INVALID                      # host memory is not device memory
    n[5] = 50; n[0] = 77                                                                                           # (stream 0 is in no group: any length)
    comb.push_host(rows, n)
    assert comb.stats(2)["samples"] == 50 and comb.stats(5)["samples"] == 50 and comb.stats(0)["samples"] == 0
    want = hd.combine.HostCombiner([1, 2, 3])
    want.set_delay(1, 8192); want.set_weight(1, 255)
    assert comb.output(1).tobytes() == want.push(rows[1:4, :50]).tobytes() and comb.output(0).size == 0
    # a stream that was in another group leaves it; a group that loses its reference is dissolved; count = 0 dissolves
    comb.set_group([6, 3])
    assert comb.stats(3)["group"] == 6 and comb.stats(1)["members"] == 2 and comb.stats(1)["samples"] == 50 and comb.stats(2)["delay"] == 8192
    comb.set_group([7, 4])
    assert comb.stats(4)["group"] == 7 and comb.stats(5)["group"] == NO_GROUP
    assert L.hd_combine_set_group(comb.h, u(2).ctypes.data, 0) == HD_ERR_INVALID                                     # no reference
    comb.dissolve(1)
    assert comb.stats(1)["group"] == NO_GROUP and comb.stats(2)["group"] == NO_GROUP and comb.stats(6)["group"] == 6
    assert L.hd_combine_reset(comb.h, 3) == HD_ERR_INVALID and L.hd_combine_reset(comb.h, 10) == HD_ERR_INVALID and L.hd_combine_reset(comb.h, 6) == HD_OK
    assert L.hd_combine_stats(comb.h, 0, None) == HD_ERR_INVALID and L.hd_combine_output(comb.h, 0, None, 4) == HD_ERR_INVALID
    assert L.hd_combine_rows(comb.h, None, None, None) == HD_ERR_INVALID and L.hd_combine_push_engine(None) == HD_ERR_INVALID
    out = np.zeros(8, hd.capi.COMBINE_LAG_DTYPE)
    p = hd.combine._lag_params(L, 8, dict(window=1024, max_lag=64))
    assert L.hd_combine_lags(comb.h, 3, C.byref(p), out.ctypes.data, 8) == HD_ERR_INVALID                            # no reference
    assert L.hd_combine_lags(comb.h, 6, C.byref(p), out.ctypes.data, 1) == HD_ERR_INVALID                            # no room
    assert L.hd_combine_lags(comb.h, 6, C.byref(p), out.ctypes.data, 8) == HD_ERR_UNSUPPORTED                        # no samples yet
    p.guard = 0
    assert L.hd_combine_lags(comb.h, 6, C.byref(p), out.ctypes.data, 8) == HD_ERR_INVALID
    comb.push_engine()                                                                                             # no call yet: adds nothing
    assert all(comb.debug_guards(s) == 0 for s in range(10))
    eng.close()


# ---------------------------------------------------------------- k_combine_lags against the host

# (N, L): the lags planted, one member each; the samples pushed
SEARCHES = {(1024, 64): ((-64, -1, 0, 63, 64), 1024 + 128 + 777), (8192, 2048): ((-2048, -1, 0, 63, 64, 2047), 40000),
            (16384, 4096): ((-4096, -1, 0, 63, 64, 4096), 16384 + 8192 + 777)}


@pytest.mark.parametrize("N,L", list(SEARCHES), ids=["%d_%d" % k for k in SEARCHES])
def test_lag_search_equals_the_host_restatement(hd, N, L):
    lags, n = SEARCHES[(N, L)]
    group = [1, 0] + list(range(2, 1 + len(lags)))                   # the reference is stream 1
    eng = hd.Engine(n_streams=S)
    comb = hd.combine.Combiner(eng, max_push=8192)
    comb.set_group(group)
    ref_row = CM.random_signs(n, 300 + L)
    rows = np.zeros((S, n), np.float32)
    rows[1] = ref_row
    for m, lag in enumerate(lags):
        rows[group[m + 1]] = CM.shifted(ref_row, lag, 400 + 10 * m + L)
    host = hd.combine.HostCombiner(group)
    p = hd.combine._lag_params(eng.L, 8, dict(window=N, max_lag=L))
    out = np.zeros(8, hd.capi.COMBINE_LAG_DTYPE)
    cuts = list(range(0, N + 2 * L - 1, 8000)) + [N + 2 * L - 1] + list(range(N + 2 * L, n, 8000)) + [n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        comb.push_host(np.ascontiguousarray(rows[:, a:b]), np.full(S, b - a, np.uint32))
        host.push(rows[group, a:b])
        if b == N + 2 * L - 1:
            assert eng.L.hd_combine_lags(comb.h, 1, C.byref(p), out.ctypes.data, 8) == HD_ERR_UNSUPPORTED
        if b == N + 2 * L:
            assert eng.L.hd_combine_lags(comb.h, 1, C.byref(p), out.ctypes.data, 8) == HD_OK
    got, want = comb.lags(1, 8, window=N, max_lag=L), host.lags(8, window=N, max_lag=L)
    assert got == want, (got, want)
    assert got[0] == dict(stream=1, lag=0, peak=N, second=0, valid=True)
    assert [r["lag"] for r in got[1:]] == list(lags) and all(r["valid"] for r in got)
    for m in range(1, len(group)):
        a, b = comb.debug_scores(group[m]), host.scores(m)
        assert a.size == 2 * L + 1 and np.array_equal(a, b), (N, L, m, np.flatnonzero(a != b)[:8])
    assert comb.debug_scores(1).size == 0 and comb.debug_scores(7).size == 0
    if L == 64:                                                      # rows that say nothing: every score N, lag 0 by the tie rule, second = N, not valid
        comb.set_group([5, 6])
        zeros = np.zeros((S, N + 2 * L), np.float32)
        comb.push_host(zeros, np.full(S, N + 2 * L, np.uint32))
        r = comb.lags(5, 8, window=N, max_lag=L)
        assert r[1] == dict(stream=6, lag=0, peak=N, second=N, valid=False) and np.array_equal(comb.debug_scores(6), np.full(2 * L + 1, N))
    assert all(comb.debug_guards(s) == 0 for s in range(S))
    eng.close()


# ---------------------------------------------------------------- the engine's door

@pytest.mark.parametrize("pipeline", [0, 1], ids=["linear_row", "symbol_ring"])
def test_push_engine_equals_push_device_of_the_demodulated_rows(hd, torch, pipeline):
    n_streams, n, calls, fs = 4, 16384, 4, 153600.0
    eng = hd.Engine(n_streams=n_streams, max_chunk=n, sampling_rate=fs, decimation=64, baud=300.0, rtty_bits=8, rtty_stops=2, lowpass_bw_hz=800.0, pipeline=pipeline)
    a, b = hd.combine.Combiner(eng), hd.combine.Combiner(eng)
    host = [hd.combine.HostCombiner([0, 1]), hd.combine.HostCombiner([2, 3])]
    for c in (a, b):
        c.set_group([0, 1]); c.set_group([2, 3])
        c.set_delay(1, 5); c.set_weight(3, 100)
    host[0].set_delay(1, 5); host[1].set_weight(1, 100)
    iq = np.stack([synth.fsk_iq(synth.rtty_bits("$$E%d,1*ABCD\n" % s * 6, 8, 2, 3, 4), fs, 300.0, sigma=0.05, seed=800 + s, n_samples=n * calls) for s in range(n_streams)])
    total = 0
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        a.push_engine()
        rows = np.stack([eng.demodulated(s) for s in range(n_streams)])
        assert rows.shape == (n_streams, n // 64)
        d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        b.push_device(d.data_ptr(), rows.shape[1], np.full(n_streams, rows.shape[1], np.uint32))
        del d
        total += rows.shape[1]
        for g, h in zip(([0, 1], [2, 3]), host):
            want = h.push(rows[g])
            assert a.output(g[0]).tobytes() == b.output(g[0]).tobytes() == want.tobytes() and want.size == n // 64, (pipeline, k, g)
        if k in (0, 2):                                              # a second push without a call in between adds nothing
            before = a.output(0)
            a.push_engine()
            assert a.stats(0)["samples"] == total and a.output(0).tobytes() == before.tobytes()
    assert a.stats(2)["samples"] == b.stats(2)["samples"] == total
    assert all(a.debug_guards(s) == 0 and b.debug_guards(s) == 0 for s in range(n_streams))
    eng.close()


# ---------------------------------------------------------------- end to end: four receivers of each of two payloads, tones -> combine -> clocked

SIGMA = 1.2
LATE = (0, 137, 1000, 2047)                                  # decimated samples; 4 input samples each
ALIGN_AFTER = 4                                              # calls: 16000 decimated samples


@pytest.fixture(scope="module")
def receivers(hd):
    """The eight streams' IQ, what was sent, and the CPU chain: oracle's decimated IQ -> host tones -> host combine (aligned after four calls) -> host
    clocked over the remaining calls; and every single receiver's sentences over the same calls."""
    iq = np.stack([CM.receiver_iq(SIGMA, s, m, 4 * LATE[m]) for s in (0, 1) for m in range(4)])
    sent = [CM.weak_text(0)[1], CM.weak_text(1)[1]]
    cpu, lags, single = [], [], [0] * 4
    for p in (0, 1):
        tone_rows = []
        for m in range(4):
            t = hd.HostTones(CM.FSD, TM.WEAK["baud"], TM.SHIFT / 2, -TM.SHIFT / 2)
            tone_rows.append([t.push(d) for d in CM.oracle_decimated(iq[4 * p + m])])
            got = CM.clocked_sentences(hd, tone_rows[m][ALIGN_AFTER:])
            assert all(text in sent[p] for (_, _, text) in got)
            single[m] += len(got)
        h = hd.combine.HostCombiner([4 * p + m for m in range(4)])
        combined = []
        for k in range(TM.WEAK["calls"]):
            row = h.push(np.stack([tone_rows[m][k] for m in range(4)]))
            if k >= ALIGN_AFTER:
                combined.append(row)
            if k == ALIGN_AFTER - 1:
                lags.append(h.align(CM.GUARD))
        cpu.append(CM.clocked_sentences(hd, combined))
    return iq, sent, cpu, lags, single


def test_four_receivers_of_two_payloads_end_to_end(hd, receivers):
    iq, sent, cpu, cpu_lags, single = receivers
    n, calls = TM.WEAK["n"], TM.WEAK["calls"]
    eng = hd.Engine(n_streams=8, max_chunk=n, sampling_rate=TM.WEAK["fs"], decimation=TM.WEAK["D"], baud=TM.WEAK["baud"], rtty_bits=8, rtty_stops=2,
                    lowpass_bw_hz=TM.WEAK["bw"])
    tones, clk = eng.tones(), eng.clocked()
    comb = hd.combine.Combiner(eng)
    for s in range(8):
        tones.set_modem(s, TM.WEAK["baud"], TM.SHIFT / 2, -TM.SHIFT / 2)
    comb.set_group([0, 1, 2, 3]); comb.set_group([4, 5, 6, 7])
    for k in range(calls):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        tones.push_engine()
        comb.push_tones(tones)
        clk.push_device(*comb.rows())
        if k == ALIGN_AFTER - 1:
            assert comb.stats(0)["samples"] == 16000
            for p, ref in enumerate((0, 4)):
                res = comb.align(ref, CM.GUARD)
                assert all(r["valid"] for r in res) and all(abs(r["lag"] - LATE[m]) <= 2 for m, r in enumerate(res)), res
                assert res == cpu_lags[p], (res, cpu_lags[p])
                top = max(r["lag"] for r in res)
                assert [comb.stats(ref + m)["delay"] for m in range(4)] == [top - r["lag"] for r in res]
            for ref in (0, 4):
                clk.take_sentences(ref, 256)                         # (a reset leaves sentences that were not taken: none from before the align may stay)
            clk.reset()                                              # the output's time axis moved
    n_combined = 0
    for p, ref in enumerate((0, 4)):
        got = clk.take_sentences(ref, 256)
        assert got == cpu[p], (p, got, cpu[p])                       # positions, flip counts and text
        assert all(text in sent[p] for (_, _, text) in got), (p, got)
        assert all(clk.take_sentences(ref + m, 256) == [] for m in range(1, 4))
        n_combined += len(got)
    print("four receivers at sigma", SIGMA, ": combined", n_combined, "single receivers with repair", single, "over calls", ALIGN_AFTER, "..", calls - 1)
    assert n_combined >= max(single) + 3
    assert all(comb.debug_guards(s) == 0 for s in range(8))
    eng.close()


# ---------------------------------------------------------------- the guard hook itself

def test_the_guard_hook_counts_damaged_words(hd):
    from test_gpu_tones import damage_the_row_guards
    eng = hd.Engine(n_streams=3, max_chunk=TM.WEAK["n"], sampling_rate=TM.WEAK["fs"], decimation=TM.WEAK["D"])
    comb = hd.combine.Combiner(eng, max_push=64)
    d_rows, stride, _ = comb.rows()
    damaged, restored = damage_the_row_guards(comb.debug_guards, d_rows, stride, 64)
    assert damaged == [1, 2, 1] and restored == [0, 0, 0]
    eng.close()
