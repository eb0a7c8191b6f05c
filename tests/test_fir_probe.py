"""The sparse-probe check of the FIR stages (tests/fir_probe.py), as far as it can be settled without a GPU:

  a. the ORACLE stays inside the model's bound, on every case tests/test_gpu_fast_taps.py runs on the kernels -- which is what makes that bound a fair
     demand on them: the reference arithmetic alone passes it;
  b. the probes kill mutants: a float32 emulation of the chain (bit-equal to the oracle; also as two fused multiply-add chains) with one tap scaled by
     1 + 2^-10, zeroed, or swapped with its neighbour exceeds the bound at least fourfold, for every tap of every table -- against the norm-wise 1e-5 gate
     (bench.normwise), which the same mutants pass;
  c. the layout conditions hold, counted from the impulse positions, for the real and the imaginary part each on its own: every tap of both stages exercised, also through the history carry, and -- for the
     worker waves -- among a tile's wrapped rows, in a run's first tile and in the closing tile."""
import numpy as np
import pytest

import fir_probe as fp

NAMES = fp.CASE_NAMES                    # static: the table behind them needs the oracle's tap tables, which collection must not
KILL = 4.0


class _Cases:
    def __getitem__(self, name):
        return fp.cases()[name]


CASES = _Cases()
_runs = {}


@pytest.fixture(scope="module")
def schedule_exe(tmp_path_factory):
    exe = fp.build_schedule_program(tmp_path_factory.mktemp("ring"))
    if exe is None:
        pytest.skip("no host C++ compiler")
    return exe


def rotated(L, x, f, fs):
    """hd_host_tune_rotate over a whole stream (the phase runs on from call to call, as the engine's does)."""
    import ctypes as C
    if f == 0.0:
        return x
    step = C.c_uint32(0)
    assert L.hd_host_tune_step(f, fs, C.byref(step)) == 0
    out = np.zeros(2 * len(x), np.float32)
    L.hd_host_tune_rotate(np.ascontiguousarray(x).view(np.float32), len(x), 0, step.value, out)
    return out.view(np.complex64)


def case_streams(name):
    """(inputs [S, n C] as the first stage sees them, positions, stages) of a case: the probe, rotated by the host's bit model where the case is tuned."""
    c = CASES[name]
    x, pos, st = fp.case_input(c)
    if c.get("tune"):
        from habdec_amd.build import build
        build()
        import habdec_amd
        L = habdec_amd.lib()
        x = np.stack([rotated(L, x[s], f, c["fs"]) for s, f in enumerate(c["tune"])])
    return x, pos, st


def oracle_run(name):
    """Per stream the oracle's read-outs of every call, the model's, and the low-pass taps -- computed once per case."""
    c = CASES[name]
    key = fp.layout_key(c)                      # (cases that differ in the engine's settings only share one run)
    if key not in _runs:
        from oracle import pyoracle
        x, pos, st = case_streams(name)
        out = []
        for s in range(c["S"]):
            o = pyoracle.Decoder("oracle", factor=c["factor"], lowpass_bw=c.get("lowpass_bw"), ungated=c.get("ungated", False))
            calls = x[s].reshape(c["n"], c["C"])
            got = []
            for k in range(c["n"]):
                o(calls[k], c["fs"])
                got.append((o.array("last_decimated"), o.array("last_filtered")))
            taps = o.array("fir_taps")
            lp = c.get("filtered") and len(taps) > 0
            out.append((got, fp.model(calls, st, taps if lp else None), taps))
        _runs[key] = (out, pos, st)
    return _runs[key]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_stays_inside_the_bound(name):
    c = CASES[name]
    out, pos, st = oracle_run(name)
    worst, worst_f, filtered = 0.0, 0.0, 0
    for s, (got, res, taps) in enumerate(out):
        for k, ((dec, filt), r) in enumerate(zip(got, res)):
            worst = max(worst, fp.check(dec, r, "oracle decimated", k, s, pos[s], st, c["C"]))
            if c.get("filtered") and len(taps):
                assert (r["fy"] is None) == (filt.size == 0), ("the model filters in other calls than the oracle", name, s, k)
            if r["fy"] is not None:
                worst_f = max(worst_f, fp.check(filt, r, "oracle filtered", k, s, pos[s], st, c["C"], fy=True))
                filtered += filt.size
    print(name, "oracle excess: decimated", worst, "filtered", worst_f)
    assert worst <= 1.0 and worst_f <= 1.0
    assert filtered > 0 or not c.get("filtered")


@pytest.mark.parametrize("name", NAMES)
def test_layout_conditions(name, request):
    c = CASES[name]
    schedule_exe = request.getfixturevalue("schedule_exe") if c.get("ring") else None       # (only the worker-wave cases need the schedule program)
    out, pos, st = oracle_run(name)
    x = fp.case_input(c)[0]
    C, n, S = c["C"], c["n"], c["S"]
    (R1, k1), F = st[0], fp.total_ratio(st)
    T1 = len(k1)
    lo = fp.min_spacing(st)
    assert lo == T1 + R1 * ((len(st[1][1]) - 1) if len(st) == 2 else 0)
    assert all(np.all(np.diff(p) >= lo) for p in pos)                                  # isolated impulses
    assert np.all(np.abs(x).reshape(S, n, C).max(axis=2) > 0)                          # no stream all zero in any push
    assert set(np.unique(x).tolist()) <= set(fp.AMPS.tolist()) | {0}
    tiles = fp.schedule_tiles(schedule_exe, C // R1, fp.halo_rows(st), c["ring"][0], c["ring"][1]) if c.get("ring") else None
    # Real and imaginary part are two filters on the two halves of a float2: each has to meet every condition with its own impulses, counted from
    # what the first stage is fed (behind the front tuner, where the case has one).
    fed = case_streams(name)[0].view(np.float32).reshape(S, n * C, 2)
    for part in (0, 1):
        own = [p[fed[s, p, part] != 0] for s, p in enumerate(pos)]
        cov = fp.coverage(own, st, C, n, tiles, fp.first_worker_call(c))
        assert cov["res1"] == set(range(R1)) and cov["resF"] == set(range(F)), (part, sorted(set(range(F)) - cov["resF"]))
        assert cov["taps1"] == set(range(T1))
        # the newest sample of a window (tap T - 1) is the output's own row: it cannot lie in the push before
        assert cov["carry1"] >= set(range(T1 - 1)), (part, sorted(set(range(T1 - 1)) - cov["carry1"]))
        if len(st) == 2:
            T2 = len(st[1][1])
            assert cov["taps2"] == set(range(T2))
            assert cov["carry2"] >= set(range(T2 - 1)), (part, sorted(set(range(T2 - 1)) - cov["carry2"]))
        if tiles is not None:
            assert R1 == 32 and fp.halo_rows(st) == tiles[0][2] - tiles[0][1]
            assert cov["first"] == set(range(T1)) and cov["closing"] == set(range(T1)), (part, sorted(set(range(T1)) - cov["first"]), sorted(set(range(T1)) - cov["closing"]))
            if c["ring"][1]:
                assert any(t[4] for t in tiles), "no chained tile in this schedule"
                assert cov["wrapped"] == set(range(T1)), (part, sorted(set(range(T1)) - cov["wrapped"]))
    # no untested stretch: at most 1 % of the checked samples have nothing in their windows (y == 0 and e == 0 in both parts)
    total = sum(len(r["y"]) for _, res, _ in out for r in res)
    empty = sum(int(np.count_nonzero(((r["e"] == 0) & (r["y"] == 0)).all(axis=1))) for _, res, _ in out for r in res)
    print(name, "outputs without a term:", empty, "of", total)
    assert empty <= 0.01 * total, (empty, total)


def mutant_layout(factor, lowpass_ntaps=0):
    """One stream, one push, from zero history: impulses at the least odd spacing, two more than the total ratio (every residue, so every tap)."""
    st = fp.tables(factor)
    F, P = fp.total_ratio(st), fp.spacing_for(st, lowpass_ntaps)
    N = -(-(F + 2) * P // (F * fp.LP_BATCH)) * F * fp.LP_BATCH
    x, _ = fp.probe_input(1, N, 1, st, pos=[np.arange(5, N, P)])
    return x[0], st


@pytest.mark.parametrize("factor", [64, 128, 256, 16, 8])
def test_probes_kill_every_decimator_tap_mutant(factor):
    import bench
    from oracle import pyoracle
    x, st = mutant_layout(factor)
    res = fp.model(x[None, :], st)[0]
    mb = fp.MutantBench(x, st)
    o = pyoracle.Decoder("oracle", factor=factor, ungated=True)
    o(x, 1e6)
    odec = o.array("last_decimated")
    as_c = lambda y: np.ascontiguousarray(y).view(np.complex64).reshape(-1)
    assert np.array_equal(as_c(mb.run()[-1]).view(np.uint32), odec.view(np.uint32)), "the sequential emulation is not the oracle's arithmetic"
    assert fp.excess(odec, res["y"], res["e"]) <= 1.0
    assert fp.excess(as_c(mb.run(mode="fma2")[-1]), res["y"], res["e"]) <= 1.0          # two fused chains: inside the same bound
    for j, (r, k) in enumerate(st):
        kills = mb.kills(j, res["y"], res["e"])
        assert len(kills) >= 3 * len(k) - 1 - int(np.count_nonzero(k[1:] == k[:-1]))
        worst = min(kills, key=kills.get)
        t = [np.asarray(kk, np.float32) for _, kk in st]
        t[j] = dict(fp.mutants(k))[worst]
        print(f"/{factor} table {j} ({len(k)} taps): smallest kill {kills[worst]:.1f} by {worst}; that mutant's norm-wise difference {bench.normwise(as_c(mb.run(t)[-1]), odec):.2e}")
        assert kills[worst] >= KILL, (factor, j, worst, kills[worst])


_lowpass_bench = []


def lowpass_kills(fs):
    """Every mutant of the low-pass table the oracle designs at /64 and sample rate fs, on `filtered`, on a layout so sparse that no window of the low-pass
    sees two impulses: ({mutant: excess}, taps, the model's result).  The emulation is first held bit-equal to the oracle, and both arithmetics inside the bound."""
    from oracle import pyoracle
    o = pyoracle.Decoder("oracle", factor=64)
    o(np.zeros(64 * 256, np.complex64), fs)
    taps = o.array("fir_taps").copy()
    assert len(taps) == 161
    if not _lowpass_bench:                  # the layout and the term structure depend on the number of taps only: one for both rates
        x, st = mutant_layout(64, len(taps))
        _lowpass_bench.append((x, st, fp.MutantBench(x, st, taps)))
    x, st, mb = _lowpass_bench[0]
    mb.tables[2] = np.asarray(taps, np.float32)
    o = pyoracle.Decoder("oracle", factor=64)
    o(x, fs)
    res = fp.model(x[None, :], st, taps)[0]
    as_c = lambda y: np.ascontiguousarray(y).view(np.complex64).reshape(-1)
    assert np.array_equal(as_c(mb.run()[-1]).view(np.uint32), o.array("last_filtered").view(np.uint32))
    assert fp.excess(o.array("last_filtered"), res["fy"], res["fe"]) <= 1.0
    assert fp.excess(as_c(mb.run(mode="fma2")[-1]), res["fy"], res["fe"]) <= 1.0
    return mb.kills(2, res["fy"], res["fe"]), taps, res


def test_probes_kill_every_lowpass_tap_mutant():
    """Every tap of the low-pass at /64, on `filtered`: scaled by 1 + 2^-10, zeroed, swapped with its neighbour -- each at least fourfold outside the bound.

    At 2.4 MS/s, not at the 2.048 MS/s of the GPU cases.  The low-pass is a windowed sinc of 161 taps at every rate; which taps land on the sinc's zero
    crossings depends on 1500 Hz against the decimated rate.  At 2.048 MS/s (32 kHz) taps 13 and 147 land on one: -5.7e-8 beside neighbours of 2.1e-6 and
    -3.5e-6 (centre tap 3.1e-2).  The low-pass is never fed anything sparser than one impulse response of the decimators, about 38 smooth samples, so
    whatever window puts a sample on tap 13 puts samples of like size on taps 12 and 14, and their share of the bound outweighs a 2^-10 change of tap 13
    whatever the spacing of the impulses: no layout settles that, the table has to.  At 2.4 MS/s (37.5 kHz) no tap is less than 0.19 of its larger
    neighbour (0.016 at 2.048 MS/s), and all 482 mutants are killed.  test_lowpass_mutants_of_the_table_the_gpu_cases_use holds the 2.048 MS/s table to the same demand
    wherever the float64 model shows it can be met at all."""
    kills, taps, _ = lowpass_kills(2.4e6)
    assert len(kills) >= 3 * len(taps) - 1 - int(np.count_nonzero(taps[1:] == taps[:-1]))
    worst = min(kills, key=kills.get)
    print(f"low-pass at 2.4 MS/s (161 taps): smallest kill {kills[worst]:.2f} by {worst}")
    short = sorted((v, k) for k, v in kills.items() if v < KILL)
    assert not short, ("mutants that exceed the bound less than fourfold", short)


def test_lowpass_mutants_of_the_table_the_gpu_cases_use():
    """The 2.048 MS/s table (tail_64, the step cases): every mutant at least fourfold outside the bound, but for scaled taps that PROVABLY cannot be.

    A tap t scaled by 1 + 2^-10 moves the exact value of output n by 2^-10 |k[t] d[n - (T - 1) + t]|, d being the low-pass's input.  In units of the bound
    that is `reach[t]`, its largest over the outputs, computed here from the float64 model alone.  The emulation's own rounding stays inside the bound (it
    is a summation tree like any other), so a mutant's excess is at most reach + 1 and at least reach - 1, both up to the 2^-10 by which the mutated
    table's bound is larger.  reach < 2.9 therefore means that no arithmetic shows this mutant fourfold on this layout; those taps are exempt as SCALED
    mutants only -- zeroed and swapped they must be killed like every other, and are.  They are the table's two zero crossings (see above)."""
    kills, taps, res = lowpass_kills(2.048e6)
    T = len(taps)
    d, fe = np.abs(res["y"]), res["fe"]
    n = len(fe)
    dd = np.concatenate([np.zeros((T - 1, 2)), d])[:T - 1 + n]
    with np.errstate(divide="ignore", invalid="ignore"):
        reach = np.array([np.max(np.where(fe > 0, 2.0 ** -10 * abs(float(taps[t])) * dd[t:t + n] / fe, 0.0)) for t in range(T)])
    blind = [t for t in range(T) if reach[t] < 2.9]
    for t in range(T):
        assert reach[t] - 1.01 <= kills[("scaled", t)] <= reach[t] * (1 + 2.0 ** -9) + 1.01, (t, reach[t], kills[("scaled", t)])
    short = sorted((v, k) for k, v in kills.items() if v < KILL and not (k[0] == "scaled" and k[1] in blind))
    rest = min(v for k, v in kills.items() if not (k[0] == "scaled" and k[1] in blind))
    print(f"low-pass at 2.048 MS/s: scaled taps out of reach {[(t, round(float(reach[t]), 2), round(kills[('scaled', t)], 2)) for t in blind]}; smallest kill of the other {len(kills) - len(blind)}: {rest:.1f}")
    assert not short, ("mutants that exceed the bound less than fourfold", short)
    # a zero crossing: the neighbours differ in sign and the tap is smaller than either
    assert all(0 < t < T - 1 and taps[t - 1] * taps[t + 1] < 0 and abs(taps[t]) < min(abs(taps[t - 1]), abs(taps[t + 1])) for t in blind), "out of reach, yet no zero crossing of the table"


def test_the_norm_wise_gate_passes_what_the_probe_kills():
    """What the 1e-5 gate could not see, re-measured: single-tap mutants of the /64 tables against bench.normwise on noise and on the probe."""
    import bench
    st = fp.tables(64)
    r = np.random.default_rng(64)
    noise = (0.4 * (r.standard_normal(16384) + 1j * r.standard_normal(16384))).astype(np.complex64)
    probe, _ = mutant_layout(64)
    as_c = lambda y: np.ascontiguousarray(y).view(np.complex64).reshape(-1)
    benches = {what: fp.MutantBench(x, st) for what, x in (("noise", noise), ("probe", probe))}
    refs = {what: as_c(mb.run()[-1]) for what, mb in benches.items()}
    for j, t, f in ((0, 5, 1.001), (0, 0, 1.001), (0, 211, 1.001), (1, 0, 1.001)):
        taps = [np.asarray(k, np.float32).copy() for _, k in st]
        taps[j][t] *= np.float32(f)
        for what, mb in benches.items():
            nw = bench.normwise(as_c(mb.run(taps)[-1]), refs[what])
            print(f"table {j} tap {t} x {f} on {what}: norm-wise {nw:.2e}")
            assert nw <= 1e-5
    res = fp.model(probe[None, :], st)[0]
    assert fp.excess(as_c(benches["probe"].run(taps)[-1]), res["y"], res["e"]) >= KILL
