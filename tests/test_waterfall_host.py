"""Host side of the waterfall (include/habdec_amd_host.h: hd_host_waterfall_detect_row, hd_host_waterfall_tracks) -- no GPU.

1. The row detector against a numpy restatement (float32 arithmetic, one rounding per operation), bit for bit, on hand-made rows (HAND: also what
   tests/test_gpu_waterfall.py pushes through the GPU's detector).
2. The tracker against a plain-Python restatement.
3. Noise alone gives no mark: a condition, not a measurement.
4. A capture model: three signals at 256 kS/s, two of them gated in time.

The row model is float64 numpy with the segmentation of tests/test_survey_host.py (periodograms), summed per row.

A symmetric guard |f_i| < dc_guard_hz always takes out an odd number of bins (bin 2048 is f = 0), so the eligible count m is even only without a guard:
the even / odd cases are guard 0 (m = 4096), one bin out (m = 4095) and three bins out (m = 4093)."""
import ctypes as C
import math

import numpy as np
import pytest

import test_survey_host as sh
from habdec_amd import capi, synth

N, HOP = 4096, 2048
FS = 2.048e6
SHORT, BAD, NO_FLOOR = capi.WF_SHORT, capi.WF_BAD, capi.WF_NO_FLOOR
INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def L():
    from habdec_amd.build import build
    build()
    return capi.lib()


# ---- the detector, restated in numpy float32
def factor(threshold_db, segments):
    return np.float32(max(10.0 ** (threshold_db / 10.0), 1.0 + 8.0 / math.sqrt(segments)))


def eligible(fs, dc_guard_hz):
    f = (np.arange(N) - N // 2) * (fs / N)
    return np.abs(f) >= dc_guard_hz if dc_guard_hz > 0 else np.ones(N, bool)


def model_row(row, segments, fs=FS, threshold_db=6.0, dc_guard_hz=0.0):
    """(flags, floor, level, marks uint32[128]) of one row of 4096 float32 sums"""
    row = np.ascontiguousarray(row, np.float32)
    key = row.view(np.uint32)
    flags = SHORT if segments < 16 else 0
    none = np.zeros(128, np.uint32)
    if (key > INF_BITS).any():
        return flags | BAD, np.float32(0), np.float32(0), none
    el = eligible(fs, dc_guard_hz)
    s = np.sort(key[el]).view(np.float32)                       # ascending as unsigned patterns
    m = len(s)
    with np.errstate(over="ignore"):
        floor = s[m // 2] if m % 2 else np.float32(0.5) * (s[m // 2 - 1] + s[m // 2])      # float32 + float32, float32 * float32: one rounding each
        if floor == 0 or np.isinf(floor):
            return flags | NO_FLOOR, np.float32(0), np.float32(0), none
        level = floor * factor(threshold_db, segments)
    assert floor.dtype == np.float32 and level.dtype == np.float32
    if flags:
        return flags, floor, level, none
    return flags, floor, level, np.packbits(el & (row >= level), bitorder="little").view(np.uint32)


def c_row(L, row, segments, fs=FS, **params):
    """(rc, header, marks) of hd_host_waterfall_detect_row"""
    p = capi.hd_waterfall_params()
    L.hd_host_waterfall_params_default(C.byref(p))
    for k, v in params.items():
        setattr(p, k, v)
    row = np.ascontiguousarray(row, np.float32)
    hdr, marks = np.zeros(1, capi.WATERFALL_ROW_DTYPE), np.full(128, 0xDEADBEEF, np.uint32)
    rc = L.hd_host_waterfall_detect_row(row.ctypes.data, segments, fs, C.byref(p), hdr.ctypes.data, marks.ctypes.data)
    return rc, hdr[0], marks


def bits_of(x):
    return int(np.float32(x).view(np.uint32))


def marked(marks):
    return [int(i) for i in np.flatnonzero(np.unpackbits(np.ascontiguousarray(marks, np.uint32).view(np.uint8), bitorder="little"))]


# ---- hand-made rows: name -> (row, segments, params)
def _hand():
    rng = np.random.Generator(np.random.PCG64(11))
    perm = rng.permutation(N)
    ones = np.ones(N, np.float32)
    H = {}

    def put(name, row, segments=16, **params):
        H[name] = (np.ascontiguousarray(row, np.float32), segments, params)

    def with_(bins, base=ones):
        r = base.copy()
        for i, v in bins.items():
            r[i] = v
        return r

    put("all_equal", np.full(N, 3.0))
    put("all_zero", np.zeros(N))
    put("median_inf_both_middles", with_({i: np.inf for i in perm[:2049]}))
    put("median_inf_upper_middle", with_({i: np.inf for i in perm[:2048]}))
    put("middle_sum_overflows", np.full(N, 3e38))
    put("inf_bins_above_a_finite_floor", with_({5: np.inf, 4000: np.inf}))
    put("one_nan", with_({1234: np.nan}))
    put("one_negative_zero", with_({77: -0.0}))
    put("one_negative", with_({4095: -1.0}))
    put("nan_inside_the_guard_still_bad", with_({2048: np.nan}), dc_guard_hz=600.0)
    # ties: 2040 x 1, 16 x 2 (sorted places 2040..2055: both middles inside the run of equals), the rest 3, in scrambled places; two bins far above
    t = np.empty(N, np.float32)
    t[perm[:2040]], t[perm[2040:2056]], t[perm[2056:]] = 1.0, 2.0, 3.0
    put("ties_both_middles_in_a_run", with_({int(perm[0]): 100.0, int(perm[4000]): 100.0}, t))
    t = np.empty(N, np.float32)
    t[perm[:2048]], t[perm[2048:]] = 1.0, 2.0                        # s[2047] = 1, s[2048] = 2: the lower middle is the largest key below the upper
    put("ties_middles_straddle_two_runs", with_({int(perm[4095]): 7.0}, t))
    t = np.empty(N, np.float32)
    t[perm[:2047]], t[perm[2047:2049]], t[perm[2049:]] = 1.0, 2.0, 3.0   # s[2047] = s[2048] = 2, the run starts exactly at the lower middle
    put("ties_run_starts_at_the_lower_middle", t)
    # even and odd eligible counts on noise-like values; a huge value inside the guard is neither floor nor mark
    e = rng.uniform(1.0, 1.5, N).astype(np.float32)
    e[[100, 3000]] = 40.0
    put("m_4096_even", e)
    put("m_4095_odd", with_({2048: 1e9}, e), dc_guard_hz=250.0)
    put("m_4093_odd", with_({2047: 1e9, 2048: 1e9, 2049: 1e9}, e), dc_guard_hz=750.0)
    put("guard_edge_is_eligible", with_({2046: 1e9, 2050: 1e9}, e), dc_guard_hz=1000.0)     # |f| = 1000 Hz is outside the guard
    # every byte of the key decides somewhere: random patterns below +inf
    put("random_patterns", rng.integers(0, INF_BITS, N, dtype=np.uint32).view(np.float32), 64)
    put("random_patterns_narrow", (rng.integers(0, 1 << 9, N, dtype=np.uint32) + np.uint32(0x3F800000)).view(np.float32), 64)
    put("subnormal_floor", (rng.integers(1, 1 << 20, N, dtype=np.uint32)).view(np.float32), 32)
    # the level itself: floor 1, level = F[16]
    F16 = factor(6.0, 16)
    put("at_level_and_one_ulp_below", with_({100: F16, 200: np.nextafter(F16, np.float32(0)), 300: np.nextafter(F16, np.float32(9))}))
    put("word_and_half_boundaries", with_({i: 100.0 for i in (0, 31, 32, 2047, 2048, 4095)}))
    put("all_bins_marked_but_the_floor_half", with_({int(i): 50.0 for i in perm[:2040]}))
    # segments select the table entry; threshold_db = 0 leaves 1 + 8 / sqrt(s): 3 at 16, 2 at 64
    tb = with_({10: 2.5, 20: 3.0, 30: 1.99, 40: 2.0})
    put("segments_15_short", tb, 15, threshold_db=0.0)
    put("segments_1_short", tb, 1, threshold_db=0.0)
    put("segments_16_noise_term", tb, 16, threshold_db=0.0)
    put("segments_64_noise_term", tb, 64, threshold_db=0.0)
    put("segments_64_threshold_rules", tb, 64, threshold_db=4.0)
    put("short_and_bad", with_({9: np.nan}), 3)
    put("short_and_no_floor", np.zeros(N), 15)
    return H


HAND = _hand()


def by_params():
    """HAND grouped by parameter set: [(params, [names])] (one waterfall per group on the GPU)"""
    groups = {}
    for name, (_, _, params) in HAND.items():
        groups.setdefault(tuple(sorted(params.items())), []).append(name)
    return [(dict(k), v) for k, v in groups.items()]


@pytest.mark.parametrize("name", list(HAND))
def test_detector_against_the_numpy_model(L, name):
    row, segments, params = HAND[name]
    flags, floor, level, marks = model_row(row, segments, **params)
    rc, hdr, got = c_row(L, row, segments, **params)
    assert rc == 0
    assert (int(hdr["flags"]), bits_of(hdr["floor"]), bits_of(hdr["level"])) == (flags, bits_of(floor), bits_of(level)), (name, hdr, flags, floor, level)
    assert np.array_equal(got, marks), (name, marked(got), marked(marks))
    assert int(hdr["n_marked"]) == len(marked(marks)) and int(hdr["segments"]) == segments and int(hdr["first_sample"]) == 0 and int(hdr["_pad"]) == 0
    want = {"all_equal": (0, []), "all_zero": (NO_FLOOR, []), "median_inf_both_middles": (NO_FLOOR, []), "median_inf_upper_middle": (NO_FLOOR, []),
            "middle_sum_overflows": (NO_FLOOR, []), "inf_bins_above_a_finite_floor": (0, [5, 4000]), "one_nan": (BAD, []), "one_negative_zero": (BAD, []),
            "one_negative": (BAD, []), "nan_inside_the_guard_still_bad": (BAD, []), "m_4095_odd": (0, [100, 3000]), "m_4093_odd": (0, [100, 3000]),
            "guard_edge_is_eligible": (0, [100, 2046, 2050, 3000]), "at_level_and_one_ulp_below": (0, [100, 300]),
            "word_and_half_boundaries": (0, [0, 31, 32, 2047, 2048, 4095]), "segments_15_short": (SHORT, []), "segments_1_short": (SHORT, []),
            "segments_16_noise_term": (0, [20]), "segments_64_noise_term": (0, [10, 20, 40]), "segments_64_threshold_rules": (0, [20]),
            "short_and_bad": (SHORT | BAD, []), "short_and_no_floor": (SHORT | NO_FLOOR, [])}
    if name in want:
        assert (flags, marked(marks)) == want[name], (name, flags, marked(marks))
    if name == "ties_both_middles_in_a_run" or name == "ties_run_starts_at_the_lower_middle":
        assert floor == 2.0
    if name == "ties_middles_straddle_two_runs":
        assert floor == 1.5 and len(marked(marks)) == 1
    if name == "all_bins_marked_but_the_floor_half":
        assert len(marked(marks)) == 2040
    if name == "segments_15_short":
        assert floor == 1.0 and level == factor(0.0, 15) and level > 3.0            # a short row still carries floor and level


def test_defaults_and_errors(L):
    p = capi.hd_waterfall_params()
    L.hd_host_waterfall_params_default(C.byref(p))
    assert (p.slot_segments, p.rows_cap, p.threshold_db, p.dc_guard_hz) == (16, 1024, 6.0, 0.0)
    q = capi.hd_waterfall_params()
    L.hd_waterfall_params_default(C.byref(q))
    assert bytes(p) == bytes(q)
    t = capi.hd_waterfall_track_params()
    L.hd_waterfall_track_params_default(C.byref(t))
    assert (t.merge_hz, t.max_width_hz, t.gap_rows, t.min_rows) == (1500.0, 0.0, 1, 3)
    assert C.sizeof(capi.hd_waterfall_row) == 32 == capi.WATERFALL_ROW_DTYPE.itemsize and C.sizeof(capi.hd_waterfall_track) == 72
    row = np.ones(N, np.float32)
    for seg in (0, 65):
        assert c_row(L, row, seg)[0] == -1
    for params in (dict(threshold_db=-1.0), dict(threshold_db=float("nan")), dict(dc_guard_hz=-1.0), dict(dc_guard_hz=float("nan")), dict(dc_guard_hz=2e6)):
        assert c_row(L, row, 16, **params)[0] == -1, params
    assert c_row(L, row, 16, fs=0.0)[0] == -1
    hdr, marks = np.zeros(1, capi.WATERFALL_ROW_DTYPE), np.zeros(128, np.uint32)
    assert L.hd_host_waterfall_detect_row(None, 16, FS, C.byref(p), hdr.ctypes.data, marks.ctypes.data) == -1
    assert L.hd_host_waterfall_detect_row(row.ctypes.data, 16, FS, None, hdr.ctypes.data, marks.ctypes.data) == -1
    assert L.hd_host_waterfall_detect_row(row.ctypes.data, 16, FS, C.byref(p), None, marks.ctypes.data) == -1
    assert L.hd_host_waterfall_detect_row(row.ctypes.data, 16, FS, C.byref(p), hdr.ctypes.data, None) == -1


# ---- the tracker, restated
def model_tracks(headers, mbool, fs, merge_hz=1500.0, gap_rows=1, min_rows=3, max_width_hz=0.0):
    binw = fs / N
    g = min(N, math.ceil(merge_hz / binw))
    open_, done = [], []
    for r in range(len(headers)):
        idx = [] if headers["flags"][r] else [int(i) for i in np.flatnonzero(mbool[r])]
        clusters = []
        for i in idx:
            if clusters and i - clusters[-1][-1] - 1 <= g:
                clusters[-1].append(i)
            else:
                clusters.append([i])
        for c in clusters:
            lo, hi = c[0], c[-1]
            for t in open_:
                if lo <= t["bin_hi"] + g and hi + g >= t["bin_lo"]:
                    t["rows"].add(r)
                    t["bin_lo"], t["bin_hi"] = min(t["bin_lo"], lo), max(t["bin_hi"], hi)
                    t["marks"] += len(c); t["sum"] += sum(c)
                    break
            else:
                open_.append(dict(first_row=r, rows={r}, bin_lo=lo, bin_hi=hi, marks=len(c), sum=sum(c), open=0))
        for t in list(open_):
            if r - max(t["rows"]) > gap_rows:
                open_.remove(t); done.append(t)
    for t in open_:
        t["open"] = 1
        done.append(t)
    out = []
    for t in done:
        last = max(t["rows"])
        d = dict(first_sample=int(headers["first_sample"][t["first_row"]]), end_sample=int(headers["first_sample"][last]) + (int(headers["segments"][last]) + 1) * HOP,
                 first_row=t["first_row"], last_row=last, marks=t["marks"], offset_hz=(t["sum"] / t["marks"] - N // 2) * binw,
                 width_hz=(t["bin_hi"] - t["bin_lo"] + 1) * binw, rows_hit=len(t["rows"]), bin_lo=t["bin_lo"], bin_hi=t["bin_hi"], open=t["open"])
        if d["rows_hit"] < min_rows or (max_width_hz > 0 and d["width_hz"] > max_width_hz):
            continue
        out.append(d)
    out.sort(key=lambda d: (d["first_sample"], d["offset_hz"]))
    return out


def sheet(rows, seg=16, flags=None, last_segments=None):
    """headers and marks of a hand-made waterfall: rows = one collection of marked bins per row"""
    h = np.zeros(len(rows), capi.WATERFALL_ROW_DTYPE)
    mb = np.zeros((len(rows), N), bool)
    for r, bins in enumerate(rows):
        mb[r, list(bins)] = True
    h["first_sample"] = np.arange(len(rows)) * seg * HOP
    h["segments"] = seg
    if last_segments:
        h["segments"][-1] = last_segments
    h["n_marked"] = mb.sum(axis=1)
    for r, f in (flags or {}).items():
        h["flags"][r] = f
    return h, mb


def pack(mb):
    return np.packbits(mb, axis=1, bitorder="little").view(np.uint32).reshape(len(mb), 128)


def c_tracks(mb_headers, cap=64, fs=FS, **params):
    h, mb = mb_headers
    import habdec_amd
    return habdec_amd.waterfall_tracks(h, pack(mb), fs, cap, **params)


def same_tracks(got, want):
    assert len(got) == len(want), (got, want)
    for a, b in zip(got, want):
        for k in b:
            if k in ("offset_hz", "width_hz"):
                assert a[k] == pytest.approx(b[k], rel=1e-12, abs=1e-9), (k, a, b)
            else:
                assert a[k] == b[k], (k, a, b)


# g = 3 bins at the default merge_hz and 2.048 MS/s
A = [1000, 1001]
TRACK_CASES = {
    "one_steady_track": (sheet([A] * 5), {}, 1),
    "two_clusters_of_one_row_join_one_track": (sheet([[1000, 1001], [998, 1004], [1000], [1000]]), {}, 1),   # row 1: 998 and 1004 are two clusters (5 > g apart)
    "gap_of_gap_rows_bridges": (sheet([A, A, [], A, A]), {}, 1),
    "gap_of_gap_rows_plus_1_splits": (sheet([A, A, A, [], [], A, A, A]), {}, 2),
    "gap_rows_0": (sheet([A, A, A, [], A, A, A]), dict(gap_rows=0), 2),
    "gap_rows_2": (sheet([A, A, [], [], A]), dict(gap_rows=2), 1),
    "a_flagged_row_is_a_row_without_marks": (sheet([A, A, A, A, A], flags={2: BAD}), {}, 1),
    "min_rows_drops": (sheet([A, A, [2000], A]), {}, 1),
    "min_rows_1_keeps": (sheet([A, A, [2000], A]), dict(min_rows=1), 2),
    "max_width_drops": (sheet([list(range(500, 510)) + [900]] * 3), dict(max_width_hz=3000.0), 1),
    "merge_reach_of_a_track": (sheet([[1000], [1003], [1006], [1010]]), dict(min_rows=1), 2),          # cumulative range 1000-1006 reaches 1009, not 1010
    "a_cluster_joins_the_first_track_by_creation": (sheet([[1000, 1007], [1003, 1004], [1007], [1000]]), dict(min_rows=1), 2),
    "order_by_first_sample_then_offset": (sheet([[3000], [3000, 100, 2000], [3000, 100, 2000], [100, 2000], [100, 2000]]), dict(min_rows=2), 3),
    "edges_do_not_wrap": (sheet([[0, 4095]] * 3), {}, 2),
    "short_last_row_end_sample": (sheet([A] * 4, last_segments=3), {}, 1),
    "nothing": (sheet([[], []]), {}, 0),
}


@pytest.mark.parametrize("name", list(TRACK_CASES))
def test_tracker_against_its_restatement(L, name):
    hm, params, n = TRACK_CASES[name]
    want = model_tracks(hm[0], hm[1], FS, **params)
    got = c_tracks(hm, **params)
    assert len(got) == n == len(want), (got, want)
    same_tracks(got, want)
    if name == "two_clusters_of_one_row_join_one_track":
        assert (got[0]["bin_lo"], got[0]["bin_hi"], got[0]["rows_hit"], got[0]["marks"], got[0]["open"]) == (998, 1004, 4, 6, 1)
    if name == "gap_of_gap_rows_bridges":
        assert (got[0]["first_row"], got[0]["last_row"], got[0]["rows_hit"]) == (0, 4, 4)
    if name == "gap_of_gap_rows_plus_1_splits":
        assert [(t["first_row"], t["last_row"], t["open"]) for t in got] == [(0, 2, 0), (5, 7, 1)]
    if name == "a_flagged_row_is_a_row_without_marks":
        assert got[0]["rows_hit"] == 4
    if name == "merge_reach_of_a_track":
        assert [(t["bin_lo"], t["bin_hi"]) for t in got] == [(1000, 1006), (1010, 1010)]
    if name == "a_cluster_joins_the_first_track_by_creation":
        assert [(t["bin_lo"], t["bin_hi"], t["marks"], t["rows_hit"], t["open"]) for t in got] == [(1000, 1007, 5, 4, 1), (1007, 1007, 1, 1, 0)]
    if name == "max_width_drops":
        assert (got[0]["bin_lo"], got[0]["bin_hi"]) == (900, 900)
    if name == "order_by_first_sample_then_offset":
        assert [t["bin_lo"] for t in got] == [3000, 100, 2000] and [t["open"] for t in got] == [0, 1, 1]
    if name == "short_last_row_end_sample":
        assert got[0]["end_sample"] == 3 * 16 * HOP + 4 * HOP and got[0]["first_sample"] == 0 and got[0]["open"] == 1
    if name == "one_steady_track":
        assert got[0]["offset_hz"] == (1000.5 - 2048) * FS / N and got[0]["width_hz"] == 2 * FS / N and got[0]["end_sample"] == 4 * 16 * HOP + 17 * HOP


def test_cap_smaller_than_found_and_tracker_errors(L):
    h, mb = TRACK_CASES["order_by_first_sample_then_offset"][0]
    m = pack(mb)
    p = capi.hd_waterfall_track_params()
    L.hd_waterfall_track_params_default(C.byref(p))
    p.min_rows = 2
    out, found = (capi.hd_waterfall_track * 4)(), C.c_uint32(9)
    call = lambda hp, mp, n, fs, pp, op, cap, fp: L.hd_host_waterfall_tracks(hp, mp, n, fs, pp, op, cap, fp)
    assert call(h.ctypes.data, m.ctypes.data, len(h), FS, C.byref(p), out, 1, C.byref(found)) == 0 and found.value == 3 and out[0].bin_lo == 3000
    assert out[1].marks == 0                                                        # nothing written past cap
    assert call(h.ctypes.data, m.ctypes.data, len(h), FS, C.byref(p), None, 0, C.byref(found)) == 0 and found.value == 3      # cap 0: count only
    assert call(None, None, 0, FS, C.byref(p), out, 4, C.byref(found)) == 0 and found.value == 0
    assert call(None, m.ctypes.data, len(h), FS, C.byref(p), out, 4, C.byref(found)) == -1 and found.value == 0
    assert call(h.ctypes.data, None, len(h), FS, C.byref(p), out, 4, C.byref(found)) == -1
    assert call(h.ctypes.data, m.ctypes.data, len(h), FS, None, out, 4, C.byref(found)) == -1
    assert call(h.ctypes.data, m.ctypes.data, len(h), FS, C.byref(p), None, 4, C.byref(found)) == -1
    assert call(h.ctypes.data, m.ctypes.data, len(h), FS, C.byref(p), out, 4, None) == -1
    assert call(h.ctypes.data, m.ctypes.data, len(h), 0.0, C.byref(p), out, 4, C.byref(found)) == -1
    for k, v in (("merge_hz", -1.0), ("merge_hz", float("nan")), ("max_width_hz", -1.0)):
        q = capi.hd_waterfall_track_params()
        L.hd_waterfall_track_params_default(C.byref(q))
        setattr(q, k, v)
        assert call(h.ctypes.data, m.ctypes.data, len(h), FS, C.byref(q), out, 4, C.byref(found)) == -1, k


# ---- the row model: float64 sums per row, the survey's segmentation
def model_rows(x, L_seg, before=0):
    """(rows float64 [n, 4096] raw sums, headers without detector fields) of ONE push of x"""
    k = sh.segments_of(len(x))
    n = (k + L_seg - 1) // L_seg
    rows = np.zeros((n, N))
    h = np.zeros(n, capi.WATERFALL_ROW_DTYPE)
    for j in range(n):
        s0, s1 = j * L_seg, min((j + 1) * L_seg, k)
        rows[j] = sh.periodograms(x[s0 * HOP:(s1 - 1) * HOP + N]).sum(axis=0)
        h["first_sample"][j], h["segments"][j] = before + s0 * HOP, s1 - s0
    return rows, h


def detect_rows(L, rows, h, fs, **params):
    """the numpy detector on float32(rows), checked against the C function row by row: (headers, marks bool [n, 4096])"""
    h = h.copy()
    mb = np.zeros((len(rows), N), bool)
    for j, row in enumerate(rows.astype(np.float32)):
        flags, floor, level, marks = model_row(row, int(h["segments"][j]), fs, **params)
        rc, hdr, got = c_row(L, row, int(h["segments"][j]), fs, **params)
        assert rc == 0 and int(hdr["flags"]) == flags and bits_of(hdr["floor"]) == bits_of(floor) and bits_of(hdr["level"]) == bits_of(level)
        assert np.array_equal(got, marks)
        h["flags"][j], h["floor"][j], h["level"][j], h["n_marked"][j] = flags, floor, level, len(marked(marks))
        mb[j, marked(marks)] = True
    return h, mb


@pytest.mark.parametrize("L_seg", [16, 32, 64])
def test_noise_alone_gives_no_mark(L, L_seg):
    """40 rows of noise at sigma = 0.05: not one mark, not one track -- the condition is 0."""
    n = N + (40 * L_seg - 1) * HOP
    nz = synth._noise(n, 100 + L_seg)
    x = 0.05 * (nz[0::2] + 1j * nz[1::2])
    rows, h = model_rows(x, L_seg)
    assert len(rows) == 40 and (h["segments"] == L_seg).all()
    h, mb = detect_rows(L, rows, h, FS)
    assert not h["flags"].any()
    assert int(mb.sum()) == 0, [(j, marked(pack(mb)[j])) for j in range(40) if mb[j].any()]
    assert c_tracks((h, mb), min_rows=1) == []


# ---- a capture model: 256 kS/s, L = 16, 48 rows
CAP = dict(fs=256e3, L=16, rows=48, amp=0.3, noise=0.05, shift=500.0)


def capture():
    fs, Ls = CAP["fs"], CAP["L"]
    R = Ls * HOP
    n = N + (CAP["rows"] * Ls - 1) * HOP
    bits = synth.rtty_bits(synth.make_sentence("WFALL", "1,52.1,21.4,1000") * 10, 8, 2, 10, 10)
    k = np.arange(n)
    x = synth.fsk_iq(bits, fs, 300, shift=CAP["shift"], f0=40e3, amp=CAP["amp"], sigma=0.0, n_samples=n).astype(np.complex128)
    gate = (k >= 16 * R + 5000) & (k < 32 * R + 9000)
    x += gate * synth.fsk_iq(bits, fs, 300, shift=CAP["shift"], f0=-70e3, amp=CAP["amp"], sigma=0.0, n_samples=n)
    blip = (k >= 40 * R + 6000) & (k < 40 * R + 20000)
    x += blip * CAP["amp"] * np.exp(2j * np.pi * 10e3 / fs * k)
    nz = synth._noise(n, 9)
    return (x + CAP["noise"] * (nz[0::2] + 1j * nz[1::2])).astype(np.complex64)


def test_capture_model(L):
    fs = CAP["fs"]
    rows, h = model_rows(capture(), CAP["L"])
    assert len(rows) == CAP["rows"]
    hm = detect_rows(L, rows, h, fs)
    got = c_tracks(hm, fs=fs)
    same_tracks(got, model_tracks(hm[0], hm[1], fs))
    tol = CAP["shift"] / 2 + fs / N
    for t in got:
        print(f"track at {t['offset_hz']:10.1f} Hz, rows {t['first_row']}-{t['last_row']}, {t['rows_hit']} rows hit, {t['marks']} marks, open {t['open']}")
    assert len(got) == 2, got
    steady, gated = got
    assert abs(steady["offset_hz"] - 40e3) <= tol and (steady["first_row"], steady["last_row"], steady["rows_hit"], steady["open"]) == (0, 47, 48, 1)
    assert abs(gated["offset_hz"] + 70e3) <= tol and (gated["first_row"], gated["last_row"], gated["rows_hit"], gated["open"]) == (16, 32, 17, 0)
    assert gated["first_sample"] == 16 * CAP["L"] * HOP and gated["end_sample"] == 32 * CAP["L"] * HOP + 17 * HOP
    three = c_tracks(hm, fs=fs, min_rows=1)
    same_tracks(three, model_tracks(hm[0], hm[1], fs, min_rows=1))
    assert len(three) == 3, three
    blip = three[2]
    assert abs(blip["offset_hz"] - 10e3) <= fs / N and (blip["first_row"], blip["last_row"], blip["open"]) == (40, 40, 0)
