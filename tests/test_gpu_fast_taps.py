"""Every tap of every FIR in the FAST arithmetic mode, componentwise: sparse probes and the float64 model of tests/fir_probe.py against the kernels.

The norm-wise 1e-5 gate of tests/test_gpu_fast.py cannot see a wrong edge tap, a wrapped sum that lost one of its two chains at a tile boundary, or a history
row off by one at the far end of the window (tests/test_fir_probe.py measures what it lets through).  Here every stream's `decimated` (and `filtered`, where
the case keeps it) is compared after every call with the model, sample by sample, within the bound derived in tests/fir_probe.py -- a bound the oracle
itself keeps on the same inputs (tests/test_fir_probe.py, which also asserts the layout conditions of every case from the impulse positions) -- and the
same case in exact mode must equal the oracle bit for bit.  The route is asserted: a fall-back does not pass silently.  On dense noise, the fast mode must
be no further from the float64 model than twice the oracle's own distance to it (rms per call)."""
import numpy as np
import pytest

import fir_probe as fp
import test_fir_probe as cpu

pytestmark = pytest.mark.gpu
CASES = cpu.CASES


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def schedule_exe(tmp_path_factory):
    try:
        return fp.build_schedule_program(tmp_path_factory.mktemp("ring"))
    except Exception:
        return None                      # (only the failure message's tile positions need it)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def engine_for(hd, monkeypatch, c, arith):
    for k in ("HD_RING_CHAIN", "HD_RING_SHORT_PCT", "HD_RING_RUN", "HD_NO_CLAIM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)
    if c.get("ring"):
        monkeypatch.setenv("HD_RING_RUN", str(c["ring"][0]))       # the run length the layout conditions were counted for
    kw = dict(lowpass_bw_hz=c["lowpass_bw"]) if c.get("lowpass_bw") else {}
    eng = hd.Engine(n_streams=c["S"], max_chunk=c["C"], sampling_rate=c["fs"], decimation=c["factor"], pipeline=c.get("pipeline", 0), arith=arith,
                    keep_filtered=bool(c.get("filtered")), enable_spectrum=False, ungated=c.get("ungated", False), **kw)
    for s, f in enumerate(c.get("tune", ())):
        eng.set_front_tune(s, f)
    return eng


def feeder(eng, c, x):
    """One call per push: from device memory where the case's model test does (the per-CU kernels), from host memory otherwise."""
    S, C, n = c["S"], c["C"], x.shape[1] // c["C"]
    if c.get("device") or c.get("ring"):
        import torch
        slab = torch.from_numpy(np.ascontiguousarray(x.reshape(S, n, C).transpose(1, 0, 2)).view(np.float32).reshape(n, S, C, 2)).cuda()
        return n, lambda k: eng.process_device(slab[k].data_ptr(), C, C)
    return n, lambda k: eng.process_host(np.ascontiguousarray(x[:, k * C:(k + 1) * C]))


def check_route(eng, c, k, variants):
    t = eng.timing()
    variants.append(t["step_variant"])
    if "path" in c:
        assert t["path"] == c["path"], ("path", k, t["path"], c["path"])
    if "variant" in c or c.get("first_call_classic"):
        # a stream's first call restarts its history and takes fixed shares / the classic grid; from then on the per-CU kernels (tests/test_gpu_scale.py)
        assert t["step_variant"] == (0 if k == 0 else c.get("variant", 1)), ("step variant", k, variants)
    if c.get("classic"):
        assert t["path"] in (0, 2) and t["step_variant"] == 0, ("the classic grid", k, t["path"], t["step_variant"])


@pytest.mark.parametrize("name", fp.CASE_NAMES)
def test_fast_mode_every_tap(hd, monkeypatch, schedule_exe, name):
    c = CASES[name]
    x = fp.case_input(c)[0]
    ref, pos, st = cpu.oracle_run(name)
    tiles = None
    if c.get("ring") and schedule_exe is not None:
        tiles = fp.schedule_tiles(schedule_exe, c["C"] // st[0][0], fp.halo_rows(st), *c["ring"])
    for arith in (1, 0):
        eng = engine_for(hd, monkeypatch, c, arith)
        try:
            n, feed = feeder(eng, c, x)
            worst, worst_f, variants, paths = 0.0, 0.0, [], set()
            for k in range(n):
                feed(k)
                for s in range(c["S"]):
                    (odec, ofilt), r = ref[s][0][k], ref[s][1][k]
                    dec = eng.decimated(s)
                    filt = eng.filtered(s) if c.get("filtered") else None
                    if arith == 0:
                        assert same_bits(dec, odec), ("exact mode: decimated differs from the oracle's", name, k, s)
                        assert filt is None or same_bits(filt, ofilt), ("exact mode: filtered differs from the oracle's", name, k, s)
                        continue
                    worst = max(worst, fp.check(dec, r, f"{name}: decimated", k, s, pos[s], st, c["C"], tiles))
                    if filt is not None:
                        assert (r["fy"] is None) == (filt.size == 0), ("filtered in other calls than the model", name, k, s, filt.size)
                        if r["fy"] is not None:
                            worst_f = max(worst_f, fp.check(filt, r, f"{name}: filtered", k, s, pos[s], st, c["C"], tiles, fy=True))
                check_route(eng, c, k, variants)
                paths.add(eng.timing()["path"])
            print(f"{name} arith={arith}: paths {sorted(paths)} variants {sorted(set(variants))} largest excess: decimated {worst:.3f} filtered {worst_f:.3f}")
            assert arith == 0 or (worst <= 1.0 and worst_f <= 1.0)
        finally:
            eng.close()


@pytest.mark.parametrize("name", fp.DENSE_NAMES)
def test_fast_mode_is_no_less_accurate_on_noise(hd, monkeypatch, name):
    """Gaussian noise as in test_fast_mode_every_decimation_plan: per call and stream, rms(gpu_fast - model) <= 2 rms(oracle - model) on `decimated` --
    measured against the oracle's own distance to the float64 model, never against the GPU's."""
    from oracle import pyoracle
    c = dict(CASES[name], filtered=False)
    assert c.get("dense")
    S, C, n = c["S"], c["C"], 4 if "ring" not in c else 6
    r = np.random.default_rng(c["factor"])
    x = (0.4 * (r.standard_normal((S, n * C)) + 1j * r.standard_normal((S, n * C)))).astype(np.complex64)
    st = fp.tables(c["factor"])
    eng = engine_for(hd, monkeypatch, c, 1)
    try:
        _, feed = feeder(eng, c, x)
        orcs = [pyoracle.Decoder("oracle", factor=c["factor"], ungated=True) for _ in range(S)]
        models = [fp.model_values(x[s].reshape(n, C), st) for s in range(S)]
        ratios, variants = [], []
        for k in range(n):
            feed(k)
            check_route(eng, c, k, variants)
            for s in range(S):
                orcs[s](x[s, k * C:(k + 1) * C], c["fs"])
                e_orc = fp.rms_to(orcs[s].array("last_decimated"), models[s][k])
                e_gpu = fp.rms_to(eng.decimated(s), models[s][k])
                ratios.append(e_gpu / e_orc)
                assert e_orc > 0 and e_gpu <= 2.0 * e_orc, (name, k, s, e_gpu, e_orc)
        print(f"{name}: rms(gpu_fast - model) / rms(oracle - model): {min(ratios):.3f} .. {max(ratios):.3f}, mean {np.mean(ratios):.3f}")
    finally:
        eng.close()
