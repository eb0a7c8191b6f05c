"""The diversity combiner's host restatement (hd_host_combine_*) against the numpy model of its definition (tests/combine_model.py), byte for byte, the
ladder of NOTES.md -- what the clocked decoder delivers from two and four receivers where one delivers nothing -- and the lag search on the ladder's
rows.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import combine_model as CM
import tones_model as TM

PUSHES = (1, 63, 64, 65, 4097)
HD_OK, HD_ERR_INVALID, HD_ERR_UNSUPPORTED = 0, -1, -3
N_ROWS = 40000                                              # the ring of 32768 samples wraps


@pytest.fixture(scope="module")
def hd():
    from habdec_amd.build import build
    build()
    import habdec_amd
    habdec_amd.lib()
    import habdec_amd.combine
    return habdec_amd


# (name, members, delays and weights of the first part, of the second part): the second part starts at the first push boundary at or behind sample 20000
CASES = [
    ("one_member", 1, ([0], [256]), ([8192], [1])),
    ("two_members", 2, ([0, 8192], [256, 255]), ([1, 4095], [1, 256])),
    ("eight_members", 8, ([0, 1, 63, 64, 4095, 8192, 17, 5000], [256, 255, 1, 0, 256, 128, 7, 256]), ([64, 63, 0, 8192, 1, 4095, 300, 2], [0] * 8)),
    ("specials_alone", 1, ([0], [256]), ([0], [255])),
]


@pytest.fixture(scope="module")
def rows():
    """Per case the input rows: computed once."""
    out = {}
    for k, (name, M, _, _) in enumerate(CASES):
        out[name] = CM.specials_row(N_ROWS)[None, :].copy() if name == "specials_alone" else CM.random_rows(M, N_ROWS, 40 + k)
    return out


def schedule(case, size):
    _, _, first, second = case
    change = -(-20000 // size) * size
    return [(0, first[0], first[1])] + ([(change, second[0], second[1])] if change < N_ROWS else [])


@pytest.fixture(scope="module")
def raw_push(hd):
    """hd_host_combine_push by address: a push of one sample costs a call and no numpy slice."""
    f = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p)(("hd_host_combine_push", hd.lib()))

    def push(h, rows, size, sched):
        rows = np.ascontiguousarray(rows, np.float32)
        out = np.zeros(rows.shape[1], np.float32)
        src, dst, n = rows.ctypes.data, out.ctypes.data, rows.shape[1]
        changes = {start: (d, w) for start, d, w in sched}
        for at in range(0, n, size):
            if at in changes:
                for m, (d, w) in enumerate(zip(*changes[at])):
                    h.set_delay(m, d); h.set_weight(m, w)
            assert f(h.h, src + 4 * at, n, None, min(size, n - at), dst + 4 * at) == HD_OK
        return out
    return push


def test_the_cases_cover_what_they_are_meant_to():
    delays = {d for c in CASES for part in c[2:] for d in part[0]}
    weights = {w for c in CASES for part in c[2:] for w in part[1]}
    assert {0, 1, 63, 64, 4095, 8192} <= delays and {0, 1, 255, 256} <= weights
    assert {c[1] for c in CASES} >= {1, 2, 8} and any(sum(c[3][1]) == 0 for c in CASES)
    sp = CM.specials_row(N_ROWS)
    assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any() and (sp == 4.0).any() and (sp > 4.0).any() and (sp < -4.0).any()
    assert (np.abs(sp[np.isfinite(sp) & (sp != 0)]) < 1e-38).any() and np.signbit(sp[sp == 0]).any()
    q = CM.quantise(np.array([np.nan, np.inf, -np.inf, 4.000001, -1e30, 1e-45, -0.0, 0.00097, -0.00097, 0.0009765625, 3.9995], np.float32))
    assert q.tolist() == [0, 4096, -4096, 4096, -4096, 0, 0, 0, 0, 1, 4095]


@pytest.mark.parametrize("size", PUSHES + (N_ROWS,), ids=[str(p) for p in PUSHES] + ["whole"])
def test_host_equals_model_however_the_rows_are_cut(hd, rows, raw_push, size):
    for case in CASES:
        name, M = case[0], case[1]
        sched = schedule(case, size)
        want_o = CM.integers(rows[name], sched)
        want = CM.combine(rows[name], sched)
        h = hd.combine.HostCombiner(list(range(10, 10 + M)))
        got = raw_push(h, rows[name], size, sched)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (name, size, bad[:8], got[bad[:8]], want[bad[:8]])
        st = h.stats(M - 1)
        assert (st["samples"], st["members"], st["group"], st["delay"], st["weight"]) == (N_ROWS, M, 10, sched[-1][1][M - 1], sched[-1][2][M - 1])
        # the clocked decoder's quantisation of the float gives the integer back
        assert np.array_equal(CM.quantise(got), want_o), (name, size)


def test_reset_and_errors(hd, rows):
    r = rows["two_members"]
    h = hd.combine.HostCombiner([3, 5])
    h.set_delay(1, 100)
    h.push(r[:, :5000])
    h.reset()
    assert h.stats()["samples"] == 0 and h.stats(1)["delay"] == 100 and h.stats(1)["weight"] == 256     # groups, delays and weights stay
    assert h.push(r[:, 5000:9000]).tobytes() == CM.combine(r[:, 5000:9000], [(0, [0, 100], [256, 256])]).tobytes()
    L = h.L
    out = np.zeros(10, np.float32)
    n = np.array([10, 9], np.uint32)
    before = h.stats()["samples"]
    assert L.hd_host_combine_push(h.h, r.ctypes.data, r.shape[1], n.ctypes.data, 0, out.ctypes.data) == HD_ERR_INVALID        # unequal lengths
    assert h.stats()["samples"] == before
    assert L.hd_host_combine_set_delay(h.h, 1, 8193) == HD_ERR_INVALID and L.hd_host_combine_set_delay(h.h, 1, 8192) == HD_OK
    assert L.hd_host_combine_set_weight(h.h, 1, 257) == HD_ERR_INVALID and L.hd_host_combine_set_weight(h.h, 1, 256) == HD_OK
    assert L.hd_host_combine_set_delay(h.h, 2, 0) == HD_ERR_INVALID
    nine, twice = np.arange(9, dtype=np.uint32), np.array([1, 2, 1], np.uint32)
    assert not L.hd_host_combine_create(nine.ctypes.data, 9) and not L.hd_host_combine_create(twice.ctypes.data, 3)
    assert not L.hd_host_combine_create(nine.ctypes.data, 0)
    with pytest.raises(hd.HabdecError):
        hd.combine.HostCombiner(list(range(9)))
    with pytest.raises(hd.HabdecError):
        hd.combine.HostCombiner([4, 4])
    hd.combine.HostCombiner(list(range(8)))


# ---------------------------------------------------------------- lag search

PLANTED = [(-4096, 4096), (-2048, 2048), (-65, 128), (-64, 64), (-1, 64), (0, 64), (1, 64), (63, 64), (64, 64), (2047, 2048), (4096, 4096)]


def search(hd, ref, mem, N, L, guard=8, **kw):
    h = hd.combine.HostCombiner([0, 1])
    h.push(np.stack([ref, mem]))
    return h, h.lags(guard, window=N, max_lag=L, **kw)


@pytest.mark.parametrize("lag,L", PLANTED, ids=[str(p[0]) for p in PLANTED])
def test_a_planted_lag_is_found_and_every_score_equals_the_models(hd, lag, L):
    for N, n in ((1024, 1024 + 2 * L + 777), (8192 if L == 2048 else 2048, 40000)):             # the second: the rings have wrapped
        ref, mem = CM.planted(n, lag, 9000 + lag)
        h, res = search(hd, ref, mem, N, L)
        want = CM.lag_scores(ref, mem, N, L)
        got = h.scores(1)
        assert got.size == 2 * L + 1 and np.array_equal(got, want), (lag, N, np.flatnonzero(got != want)[:8])
        w = CM.lag_result(want, N, L, 8)
        assert res[0] == dict(stream=0, lag=0, peak=N, second=0, valid=True)
        assert res[1] == dict(stream=1, lag=w[0], peak=w[1], second=w[2], valid=w[3]), (res[1], w)
        assert res[1]["lag"] == lag and res[1]["valid"] and res[1]["peak"] > N // 2, (lag, N, res[1])


def test_rows_that_say_nothing(hd):
    N, L = 1024, 64
    n = N + 2 * L
    zeros = np.zeros(n, np.float32)
    h, res = search(hd, zeros, zeros, N, L)
    assert np.array_equal(h.scores(1), np.full(2 * L + 1, N)) and res[1] == dict(stream=1, lag=0, peak=N, second=N, valid=False)
    const = np.full(n, 0.5, np.float32)
    h, res = search(hd, const, -const, N, L)
    assert res[1]["peak"] == -N and res[1]["peak"] <= 0 and not res[1]["valid"] and res[1]["lag"] == 0
    ref, _ = CM.planted(n, 0, 77)
    h, res = search(hd, ref, -ref, N, L)
    assert h.scores(1)[L] == -N and not res[1]["valid"] and np.array_equal(h.scores(1), CM.lag_scores(ref, -ref, N, L))
    # ties: the smaller |l| first, then the negative l -- a row of period 8 scores N at every multiple of 8
    per = np.tile(np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float32), n // 8)
    h, res = search(hd, per, per, N, L)
    assert res[1]["lag"] == 0 and res[1]["peak"] == N and res[1]["second"] == N and not res[1]["valid"]
    h, res = search(hd, per, np.roll(per, 4), N, L)                                              # N at -4 and at +4: the negative one
    assert res[1]["lag"] == -4 and res[1] == dict(zip(("lag", "peak", "second", "valid"), CM.lag_result(CM.lag_scores(per, np.roll(per, 4), N, L), N, L, 8)), stream=1)


def test_the_search_waits_for_its_samples_and_checks_its_parameters(hd):
    N, L = 1024, 64
    ref, mem = CM.planted(N + 2 * L, 5, 31)
    h = hd.combine.HostCombiner([7, 9])
    h.push(np.stack([ref, mem])[:, :N + 2 * L - 1])
    p = hd.combine._lag_params(h.L, 8, dict(window=N, max_lag=L))
    out = np.zeros(2, hd.capi.COMBINE_LAG_DTYPE)
    assert h.L.hd_host_combine_lags(h.h, C.byref(p), out.ctypes.data, 2) == HD_ERR_UNSUPPORTED and h.scores(1).size == 0
    h.push(np.stack([ref, mem])[:, N + 2 * L - 1:])
    assert h.L.hd_host_combine_lags(h.h, C.byref(p), out.ctypes.data, 2) == HD_OK and out["lag"].tolist() == [0, 5] and out["stream"].tolist() == [7, 9]
    assert h.L.hd_host_combine_lags(h.h, C.byref(p), out.ctypes.data, 1) == HD_ERR_INVALID
    d = hd.capi.hd_combine_lag_params()
    h.L.hd_combine_lag_params_default(C.byref(d))
    assert (d.window, d.max_lag, d.guard, d.min_peak_q8, d.min_margin_q8) == (8192, 2048, 0, 76, 16)
    for bad in (dict(window=1000), dict(window=960), dict(window=16448), dict(max_lag=0), dict(max_lag=100), dict(max_lag=4160), dict(guard=0)):
        kw = dict(window=N, max_lag=L, guard=8)
        kw.update(bad)
        p = hd.combine._lag_params(h.L, kw.pop("guard"), kw)
        assert h.L.hd_host_combine_lags(h.h, C.byref(p), out.ctypes.data, 2) == HD_ERR_INVALID, bad


def test_align_sets_delays_and_drops_what_it_cannot_place(hd):
    N, L, n = 1024, 128, 1024 + 256 + 500
    ref, late = CM.planted(n, 100, 5)
    early = CM.shifted(ref, -30, 55)
    noise = CM.random_rows(1, n, 99)[0]
    h = hd.combine.HostCombiner([2, 4, 6, 8])
    h.set_delay(3, 77)
    rows = np.stack([ref, late, early, noise])
    h.push(rows)
    res = h.align(8, window=N, max_lag=L)
    assert [r["lag"] for r in res[:3]] == [0, 100, -30] and [r["valid"] for r in res] == [True, True, True, False]
    want = CM.align([(r["lag"], r["valid"]) for r in res], [0, 0, 0, 77], [256] * 4)
    assert want[:2] == ([100, 0, 130, 77], [256, 256, 256, 0])
    assert [h.stats(m)["delay"] for m in range(4)] == want[0] and [h.stats(m)["weight"] for m in range(4)] == want[1]
    p = hd.combine._lag_params(h.L, 8, dict(window=N, max_lag=L))
    out = np.zeros(4, hd.capi.COMBINE_LAG_DTYPE)
    assert h.L.hd_host_combine_align(h.h, C.byref(p), out.ctypes.data, 4) == 3                  # the reference's entry counts
    more = CM.random_rows(4, 3000, 100)
    assert h.push(more).tobytes() == CM.combine(np.concatenate([rows, more], axis=1), [(0, [0, 0, 0, 77], [256] * 4), (n, want[0], want[1])])[n:].tobytes()


# ---------------------------------------------------------------- the ladder: four receivers of each of four payloads (NOTES.md, "Diversity combiner")
# CRC-valid sentences, plain / with repair, of the 28 sent over the four payloads -- measured with this code on the CPU:
#   sigma 1.2: one receiver 1 / 3 and 0 / 1, two combined 31 / 31, four combined 32 / 32
#   sigma 1.4: one receiver 0 / 0,           two combined 14 / 18, four combined 29 / 29

def ladder(hd, sigma):
    out = dict(single=[0] * 4, single_repaired=[0] * 4, two=0, two_repaired=0, four=0, four_repaired=0, false=0)
    for s in range(4):
        sent = CM.weak_text(s)[1]
        rows = [CM.receiver_row(sigma, s, m) for m in range(4)]
        both = hd.combine.HostCombiner([0, 1]).push(np.stack(rows[:2]))
        four = hd.combine.HostCombiner([0, 1, 2, 3]).push(np.stack(rows))
        mean = np.trunc(CM.quantise(np.stack(rows)).sum(axis=0) / 4.0)                              # the mean of the quantised rows, truncated toward zero
        assert np.array_equal(CM.quantise(four), mean)
        for key, row in [("two", both), ("four", four)] + [(m, rows[m]) for m in range(4)]:
            for suffix, repair in (("", False), ("_repaired", True)):
                got = [t for (_, _, t) in CM.clocked_sentences(hd, row, repair)]
                assert len(set(got)) == len(got)
                out["false"] += len([t for t in got if t not in sent])
                if isinstance(key, int):
                    out["single" + suffix][key] += len(got)
                else:
                    out[key + suffix] += len(got)
    return out


def test_ladder(hd):
    sent = 28
    c12, c14 = ladder(hd, 1.2), ladder(hd, 1.4)
    for sigma, c in ((1.2, c12), (1.4, c14)):
        print("combine ladder: sigma", sigma, "single receivers plain", c["single"], "with repair", c["single_repaired"], "two combined", c["two"], "/",
              c["two_repaired"], "four combined", c["four"], "/", c["four_repaired"], "not sent", c["false"])
        assert c["false"] == 0, (sigma, c)                           # nothing delivered that was not sent
    assert 2 * max(c12["single_repaired"]) < sent and 4 * c12["two"] >= 3 * sent, c12
    assert max(c14["single_repaired"]) == 0 and c14["four_repaired"] >= c14["two_repaired"] + 3, c14


@pytest.mark.parametrize("sigma", [1.2, 1.7])
def test_alignment_on_the_ladders_rows(hd, sigma):
    """Member 1 is 137 samples late; searches ending at n = 12288, 48000 and 96000."""
    ref, mem = CM.receiver_row(sigma, 0, 0), CM.receiver_row(sigma, 0, 1)
    late = np.concatenate([np.zeros(137, np.float32), mem[:-137]])
    h = hd.combine.HostCombiner([0, 1])
    at = 0
    for n in (12288, 48000, 96000):
        h.push(np.stack([ref[at:n], late[at:n]]))
        at = n
        r = h.lags(CM.GUARD)[1]
        print("combine alignment: sigma", sigma, "n", n, r, "peak / N %.3f margin / N %.3f" % (r["peak"] / 8192, (r["peak"] - r["second"]) / 8192))
        assert r["valid"] and abs(r["lag"] - 137) <= 2, (sigma, n, r)


def test_noise_alone_is_not_valid(hd):
    """Eight pairs of independent noise rows, searches ending at n = 12288, 48000 and 96000 (NOTES.md has the figures the defaults come from)."""
    reach = []
    for k in range(8):
        a, b = CM.noise_row(2 * k + 1), CM.noise_row(2 * k + 2)
        h = hd.combine.HostCombiner([0, 1])
        at = 0
        for n in (12288, 48000, 96000):
            h.push(np.stack([a[at:n], b[at:n]]))
            at = n
            r = h.lags(CM.GUARD)[1]
            reach.append(float(np.abs(h.scores(1)).max()) / 8192)
            assert not r["valid"], (k, n, r)
    print("combine noise alone: largest |score| / N over all lags %.3f .. %.3f" % (min(reach), max(reach)))
