"""The device discriminator over its whole domain, and the flip search beside non-finite samples and on plateaus of equal weights -- against the CPU oracle,
byte for byte, call by call.

Part 1 (discriminator).  The streams of tests/discriminator_domain.py (tests/test_discriminator_domain_inputs.py proves on the CPU what they reach: all twenty
cells of exact_atan2f_plain in the clean streams, where every wave takes the straight-line function, and again in the planted ones, where a run of exact zeros at
least every 192 outputs sends every wave through exact_atan2f, with its special classes) through both inlined copies of the code and every kernel that carries one:

  factor1_separate   decimation 1, two pushes of 16384                      k_fir_demod (6 outputs per lane), the low-pass's input is the stream itself
  d64_tail256        /64, synchronous, 4 streams, pushes of 4096            k_tail, 256 lanes
  d64_tail64         /64, synchronous, 512 streams (the four patterns, repeated)   k_tail, 64 lanes
  d64_step_cu        /64, pipeline = 1, 64 streams                          k_step_cu from the second call on
  d64_step           the same with HD_NO_CU_STEP=1                          k_step
  d16_separate       /16 with HD_NO_TAIL=1                                  k_fir_demod behind two stages

The low-pass has 5 taps (lowpass_trans = 0.8) on every route; hd_timing.path is asserted.  Exact mode: decimated, filtered (where the engine keeps them) and
demodulated are the oracle's bytes; bits and backlog are the oracle's on the streams without NaN or Inf.  No tolerance anywhere.  A NaN stands exactly where the
oracle has one; its sign and payload are not compared (`canonical`, the convention of tests/test_gpu_spectrum_tail.py).  The pipelined routes are compared
through the discriminator checksums and the bits of every delivered call, which do not drain the pipeline, and buffer for buffer behind a flush every fifth call.
Fast mode (fused multiply-add in the FIRs; factor1_separate and d64_tail256): the engine's OWN low-pass output through hd_host_discriminate must be its
discriminator output bit for bit -- the discriminator apart from the FIR arithmetic.

Part 2 (flip search).  RTTY at /64, 300 baud 8N2, with one NaN in the idle carrier, NaN stretches that end R/2 before a bit edge and begin R/2 behind one, and the
same with +Inf, -Inf (window sums hold Inf - Inf); then lookup_mode = 0 with a 7 kHz shift, where every edge zone has its first maximum on a plateau of equal
integer weights.  Bits, backlog, flip points (synchronous routes), characters and sentences against the oracle, through the separate kernels, k_tail and k_step_cu."""
import numpy as np
import pytest

import discriminator_domain as dd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


def canonical(a):
    a = np.ascontiguousarray(a)
    f = a.view(np.float32).copy()
    f[np.isnan(f)] = np.nan
    return f


def same(a, b):
    a, b = canonical(a), canonical(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def checksum(demod):
    d = np.ascontiguousarray(demod).view(np.uint32).astype(np.uint64)
    return len(d), int(d.sum() & 0xFFFFFFFF), int((d * np.arange(1, len(d) + 1, dtype=np.uint64)).sum() & 0xFFFFFFFF)


ROUTES = {
    "factor1_separate": dict(case="factor1", S=4, cfg={}, env={}, path=0, variant=None),
    "d64_tail256": dict(case="d64", S=4, cfg={}, env={}, path=2, variant=None),
    "d64_tail64": dict(case="d64", S=512, cfg={}, env={}, path=2, variant=None),
    "d64_step_cu": dict(case="d64", S=64, cfg=dict(pipeline=1), env={}, path=3, variant=1),
    "d64_step": dict(case="d64", S=64, cfg=dict(pipeline=1), env=dict(HD_NO_CU_STEP="1"), path=3, variant=0),
    "d16_separate": dict(case="d16", S=4, cfg={}, env=dict(HD_NO_TAIL="1"), path=0, variant=None),
}
NP = len(dd.PATTERNS)
FINITE = [i for i, p in enumerate(dd.PATTERNS) if p != "wild"]          # bits and backlog are compared on these


def engine(hd, c, S, **kw):
    return hd.Engine(n_streams=S, max_chunk=c["push"], sampling_rate=c["fs"], decimation=c["factor"], baud=300, rtty_bits=8, rtty_stops=2,
                     lowpass_trans=dd.LOWPASS_TRANS, ungated=c["factor"] == 1, **kw)


def slab_of(case, k, S):
    c = dd.CASES[case]
    four = np.stack([dd.stream(case, p)[k * c["push"]:(k + 1) * c["push"]] for p in dd.PATTERNS])
    return np.ascontiguousarray(np.tile(four, (S // NP, 1)))


def checked_streams(S, k):
    if S <= 8 or k % 16 == 3:                         # (512 streams: all of them every 16th call, in a call whose low-pass runs; 16 of them in every call)
        return range(S)
    return sorted(set(range(4)) | set(range(S // 2 - 4, S // 2 + 4)) | set(range(S - 4, S)))


@pytest.mark.parametrize("route", list(ROUTES))
def test_exact_discriminator_matches_the_cpu_chain_over_the_whole_domain(hd, monkeypatch, route):
    r = ROUTES[route]
    case, S = r["case"], r["S"]
    c = dd.CASES[case]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    want = [dd.oracle_run(case, p) for p in dd.PATTERNS]
    ncalls = len(want[0])
    assert all(call["ntaps"] in (0, dd.T) for w in want for call in w)
    assert sum(len(call["demod"]) for call in want[0]) == c["n"]
    pipelined = bool(r["cfg"].get("pipeline"))
    eng = engine(hd, c, S, keep_filtered=not pipelined, **r["cfg"])
    variants, seen, compared, lag = [], {s: set() for s in range(S)}, 0, set()

    def compare_buffers(k, streams):
        n = 0
        for s in streams:
            w = want[s % NP][k]
            assert same(eng.decimated(s), w["decimated"]), ("decimated", route, k, s)
            if not pipelined:
                assert same(eng.filtered(s), w["filtered"]), ("filtered", route, k, s)
                if len(w["filtered"]):
                    assert len(eng.fir_taps(s)) == dd.T
            got = eng.demodulated(s)
            if not same(got, w["demod"]):
                bad = np.nonzero(canonical(got).view(np.uint32) != canonical(w["demod"]).view(np.uint32))[0] if got.shape == w["demod"].shape else []
                cl = dd.classify(w["filtered"], w["prev"])
                first = int(bad[0]) if len(bad) else -1
                raise AssertionError(("demodulated", route, dd.PATTERNS[s % NP], "call", k, "stream", s, "differing outputs", len(bad), "first", first,
                                      "classes", [n_ for n_ in dd.SPECIALS + dd.OPTIONAL if len(bad) and cl[n_][first]], "cell", int(cl["cell"][first]) if len(bad) else None,
                                      "got", got[bad[:4]] if len(bad) else got.shape, "want", w["demod"][bad[:4]] if len(bad) else w["demod"].shape))
            n += len(got)
            if s % NP in FINITE:
                assert np.array_equal(eng.bits(s), w["bits"]), ("bits", route, k, s)
                assert eng.symbol_backlog(s) == w["held"], ("backlog", route, k, s)
        return n

    def compare_delivered(k):
        for s in range(S):
            if s % NP not in FINITE:
                continue
            ci, n, c0, c1 = eng.demod_checksum(s)                  # ci: the call delivered last; (0, None) is also what the read-out says before any was
            assert ci <= k
            if ci not in seen[s] and not (n is None and (ci == 0 or not len(want[s % NP][ci]["demod"]))):
                assert (n, c0, c1) == checksum(want[s % NP][ci]["demod"]), ("discriminator checksum", route, ci, s)
                assert np.array_equal(eng.bits(s), want[s % NP][ci]["bits"]), ("bits of the delivered call", route, ci, s)
                seen[s].add(ci)
                lag.add(k - ci)

    for k in range(ncalls):
        eng.process_host(slab_of(case, k, S))
        t = eng.timing()
        assert t["path"] == r["path"], (route, k, t)
        variants.append(t["step_variant"])
        if not pipelined:
            compared += compare_buffers(k, checked_streams(S, k))
            continue
        compare_delivered(k)
        if k % 5 == 4 or k == ncalls - 1:
            eng.flush()
            compare_delivered(k)
            compared += compare_buffers(k, range(S))
    if r["variant"] is not None:
        assert all(v == r["variant"] for v in variants[1:]), (route, variants)
    if pipelined:
        # every fourth call carries discriminator output (256 decimated samples make a low-pass run); a flush may deliver two calls at once
        assert min(len(v) for s, v in seen.items() if s % NP in FINITE) >= ncalls // 4 - 2, (sorted(lag), {s: len(v) for s, v in seen.items()})
    assert compared >= c["n"] * (4 if not pipelined else 1)
    eng.close()


@pytest.mark.parametrize("route", ["factor1_separate", "d64_tail256"])
def test_fast_mode_discriminator_is_the_restatement_of_its_own_lowpass_output(hd, route):
    r = ROUTES[route]
    case, S = r["case"], r["S"]
    c = dd.CASES[case]
    L = hd.capi.lib()
    eng = engine(hd, c, S, keep_filtered=True, arith=1)
    prev, total, nans = [None] * S, 0, 0
    for k in range(c["n"] * c["factor"] // c["push"]):
        eng.process_host(slab_of(case, k, S))
        assert eng.timing()["path"] == r["path"]
        for s in range(S):
            f, got = eng.filtered(s).copy(), eng.demodulated(s)
            assert len(f) == len(got)
            if not len(f):
                continue
            if prev[s] is None:
                prev[s] = f[0]
            want = np.zeros(len(f), np.float32)
            L.hd_host_discriminate(np.ascontiguousarray(f).view(np.float32), len(f), float(prev[s].real), float(prev[s].imag), want)
            assert same(got, want), (route, k, s, np.nonzero(canonical(got).view(np.uint32) != canonical(want).view(np.uint32))[0][:8])
            prev[s] = f[-1]
            total += len(f)
            nans += int(np.isnan(want).sum())
    assert total == S * c["n"] and nans > 0
    eng.close()


# ---- flip search
FLIP_ROUTES = {"separate": dict(cfg={}, env=dict(HD_NO_TAIL="1"), path=0), "tail": dict(cfg={}, env={}, path=2), "step_cu": dict(cfg=dict(pipeline=1), env={}, path=3)}


def run_flip_route(hd, monkeypatch, route, streams, results, **cfg):
    """streams: inputs; results: their oracle calls (discriminator_domain.flip_oracle).  Eight engine streams, the given ones in turn."""
    r, F = FLIP_ROUTES[route], dd.FLIP
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    S, n = 8, F["push"]
    pipelined = bool(r["cfg"].get("pipeline"))
    eng = hd.Engine(n_streams=S, max_chunk=n, sampling_rate=F["fs"], decimation=F["factor"], baud=F["baud"], rtty_bits=F["bits"], rtty_stops=F["stops"],
                    keep_filtered=not pipelined, **r["cfg"], **cfg)
    of = lambda s: results[s % len(results)]
    chars, sentences, variants, nflips, delivered = [""] * S, [[] for _ in range(S)], [], 0, [set() for _ in range(S)]
    for k in range(F["calls"]):
        eng.process_host(np.ascontiguousarray(np.stack([streams[s % len(streams)][k * n:(k + 1) * n] for s in range(S)])))
        t = eng.timing()
        assert t["path"] == r["path"], (route, k, t)
        variants.append(t["step_variant"])
        for s in range(S):
            chars[s] += eng.take_chars(s)
            sentences[s] += eng.take_sentences(s)
            d, dn = eng.demod_checksum(s)[:2]                    # the call whose results have been delivered ((0, None): none yet)
            assert d == k or pipelined
            if d == 0 and dn is None:
                continue
            delivered[s].add(d)
            w = of(s)[d]
            assert np.array_equal(eng.bits(s), w["bits"]), ("bits", route, d, s)
            assert chars[s] == w["chars"] and tuple(sentences[s]) == w["sentences"], ("text", route, d, s, chars[s], w["chars"])
            if not pipelined:
                assert same(eng.demodulated(s), w["demod"]), ("demodulated", route, d, s)
                assert eng.symbol_backlog(s) == w["held"], ("backlog", route, d, s)
                assert np.array_equal(eng.flips(s).astype(np.int64), w["flips"]), ("flip points", route, d, s, eng.flips(s), w["flips"])
                nflips += len(w["flips"])
    eng.flush()
    for s in range(S):
        w = of(s)[-1]
        assert chars[s] + eng.take_chars(s) == w["chars"] and tuple(sentences[s] + eng.take_sentences(s)) == w["sentences"], ("text at the end", route, s)
        assert np.array_equal(eng.bits(s), w["bits"]) and eng.symbol_backlog(s) == w["held"], ("bits and backlog at the end", route, s)
        assert same(eng.demodulated(s), w["demod"]), ("demodulated at the end", route, s)
    if pipelined:
        assert all(v == 1 for v in variants[1:]), variants
        assert min(len(d) for d in delivered) >= F["calls"] - 3, [sorted(d) for d in delivered]
    else:
        assert nflips > 100 * S // len(results)
    eng.close()


@pytest.mark.parametrize("route", list(FLIP_ROUTES))
def test_flip_search_beside_nan_and_inf_samples(hd, monkeypatch, route):
    streams = dd.flip_streams()
    results = [dd.flip_results(name) for name in dd.FLIP_STREAMS]
    e1, e2, R, span = dd._cache["flip_edges"]
    assert len(results[0][-1]["sentences"]) == 2 and span > 2 * R
    for name, res in zip(dd.FLIP_STREAMS, results):
        bad = dd.nonfinite_spans(np.concatenate([c["demod"] for c in res]))
        if name == "nan_idle":
            assert bad[1] < 1000
        if name.endswith("_edges"):
            assert abs(bad[0] + span - 1 - (e1 - R // 2)) <= 1 and abs(bad[1] - span + 1 - (e2 + R // 2)) <= 1, (name, bad, e1, e2)
    run_flip_route(hd, monkeypatch, route, [streams[name] for name in dd.FLIP_STREAMS], results)


@pytest.mark.parametrize("route", list(FLIP_ROUTES))
def test_flip_search_on_plateaus_of_equal_integer_weights(hd, monkeypatch, route):
    x, res = dd.integer_weight_stream()
    R = int(round(dd.FLIP["fs"] / dd.FLIP["factor"] / dd.FLIP["baud"])) // 4
    interior = sum(1 for c in res for lo, f in dd.zones(c, R) if f != lo)
    assert interior >= 10 and len(res[-1]["sentences"]) == 2, interior
    run_flip_route(hd, monkeypatch, route, [x], [res], lookup_mode=0, lowpass_bw_hz=dd.INT["lowpass_bw"])
