"""The baud-rate probe on the GPU (hd_baud_probe_*, kernels/baud_probe.hip) and the framing trial behind it.

The probe's accumulators are integer sums: every comparison of state here is bit for bit, against the host restatement (hd_host_baud_probe_*), which
tests/test_baud_probe_host.py holds to the numpy model of the definition."""
import ctypes as C

import numpy as np
import pytest

import baud_probe_model as M
from habdec_amd import capi, synth

pytestmark = pytest.mark.gpu
PUSHES = (1, 63, 64, 65, 511, 512, 4097)
HD_ERR_INVALID, HD_ERR_DEVICE = -1, -2


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


# ---------------------------------------------------------------- kernel parity

def test_push_device_and_push_host_equal_the_host_probe(hd, torch):
    """Three streams with pushes of different sizes, one of them empty every third push: (a) a design signal, cut so that every window and the
    64-sample step straddle push boundaries, with (d) a reset in mid-stream; (c) the capped blocks; (b) NaN, Inf, zeros and denormals."""
    case = next(c for c in M.CASES if c[0] == "600_8n2")
    rows = [M.case_signal(case), M.capped_blocks()[0], M.specials_row(40000)]
    eng = hd.Engine(n_streams=3)                                     # (fsd = 32 kS/s, the probe's default grid)
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    from_host, from_dev = eng.baud_probe(), eng.baud_probe()
    ref = [hd.HostBaudProbe(fsd) for _ in rows]
    at, push, keep = [0, 0, 0], 0, []
    while any(at[s] < rows[s].size for s in range(3)):
        n = np.array([PUSHES[(push + 3 * s) % len(PUSHES)] for s in range(3)], np.uint32)
        if push % 3 == 0:
            n[push // 3 % 3] = 0
        n = np.minimum(n, [rows[s].size - at[s] for s in range(3)]).astype(np.uint32)
        stride = 4200
        slab = np.full((3, stride), np.nan, np.float32)
        for s in range(3):
            slab[s, :n[s]] = rows[s][at[s]:at[s] + n[s]]
            ref[s].push(slab[s, :n[s]])
            at[s] += int(n[s])
        from_host.push_host(slab, n)
        d = torch.from_numpy(slab).cuda()
        keep = [d]
        from_dev.push_device(d.data_ptr(), stride, n)
        push += 1
        if push == 40:                                               # (d)
            from_host.reset(0); from_dev.reset(0); ref[0].reset()
        if push in (1, 2, 7, 39, 40, 41) or push % 97 == 0:
            for s in range(3):
                M.assert_same_state(from_host.state(s), ref[s].state(), ("host memory", push, s))
    for s in range(3):
        want = ref[s].state()
        M.assert_same_state(from_host.state(s), want, ("host memory", "end", s))
        M.assert_same_state(from_dev.state(s), want, ("device memory", "end", s))
        assert want["samples"] > 0 and want["edges"].sum() > 0
    # (c) on the device: blocks of 4096 edges count, the block of 4097 does not
    st = from_dev.state(1)
    assert int(st["NB"][0]) == 3 and int(st["Q"][0]) == 4096 ** 2 + 101 ** 2 + 100 ** 2
    # reset of all streams
    from_dev.reset()
    fresh = hd.HostBaudProbe(fsd).state()
    for s in range(3):
        M.assert_same_state(from_dev.state(s), fresh, ("reset all", s))
    eng.close()


# ---------------------------------------------------------------- every route the discriminator output can take to the probe

RT = dict(S=64, fs=25600.0, baud=50, bits=7, stops=2, shift=100.0, bw=150.0, calls=14)
ROUTES = {
    # name: engine settings, samples per push, hd_timing.path, step_variant from the second call on, streams tuned at the input rate
    "sync_tail": (dict(), 4096, 2, None, {}),                               # the linear demod row
    "batch_tail_ring": (dict(pipeline=1), 4096, 2, None, {3: 1000.0}),      # a front-tuned stream keeps a batch engine's calls off the step kernel: k_tail, ring
    "batch_step_ring": (dict(pipeline=1), 4096, 3, 1, {}),                  # k_step_cu
    "separate": (dict(decimation=16, dc_remove=True), 4096, 0, None, {}),   # the DC blocker sends a call through the separate kernels
}


@pytest.fixture(scope="module")
def route_iq():
    S, n = RT["S"], 4096 * RT["calls"]
    out = np.zeros((S, n), np.complex64)
    for s in range(S):
        text = synth.make_sentence(f"P{s}", str(s % 10)) * 3
        out[s] = synth.fsk_iq(synth.rtty_bits(text, RT["bits"], RT["stops"], 2 + s % 5, 4), RT["fs"], RT["baud"], shift=RT["shift"], sigma=0.04,
                              seed=300 + s, n_samples=n)
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_push_engine_on_every_route(hd, route_iq, route):
    """push_engine behind every call against the host probe fed eng.demodulated(s) of the same calls.  In batch mode the call's output lies in the symbol
    ring only: a ring offset that is off by one, or not wrapped, fails here."""
    extra, n, path, variant, front = ROUTES[route]
    S, calls = RT["S"], RT["calls"]
    cfg = dict(n_streams=S, max_chunk=n, sampling_rate=RT["fs"], decimation=64, baud=RT["baud"], rtty_bits=RT["bits"], rtty_stops=RT["stops"],
               lowpass_bw_hz=RT["bw"])
    cfg.update(extra)
    eng, plain = hd.Engine(**cfg), hd.Engine(**cfg)                  # `plain` is never probed
    for s, f in front.items():
        eng.set_front_tune(s, f); plain.set_front_tune(s, f)
    fsd = eng.L.hd_engine_decimated_rate(eng.h)
    grid = dict(baud_lo=fsd / 40.0, baud_hi=fsd / 3.5)
    probe = eng.baud_probe(**grid)
    ref = [hd.HostBaudProbe(fsd, **grid) for _ in range(S)]
    fed = 0
    for k in range(calls):
        x = np.ascontiguousarray(route_iq[:, k * n:(k + 1) * n])
        eng.process_host(x); plain.process_host(x)
        probe.push_engine()
        t = eng.timing()
        assert t["path"] == path, (route, k, t)
        if variant is not None and k >= 1:
            assert t["step_variant"] == variant, (route, k, t)
        for s in range(S):
            d = eng.demodulated(s)
            ref[s].push(d)
            fed += d.size
        if k in (0, 5):                                              # a second push without a call in between changes nothing
            probe.push_engine()
        if k in (0, 1, 5, calls - 1):
            for s in range(S):
                M.assert_same_state(probe.state(s), ref[s].state(), (route, k, s))
    assert fed > S * 100 and probe.state(0)["edges"].sum() > 0, fed
    eng.flush(); plain.flush()
    for s in range(S):      # the probed engine went on decoding what an engine that was never probed decodes
        assert (eng.take_chars(s), eng.take_sentences(s), eng.bits_total(s), eng.demod_checksum_total(s)) == \
               (plain.take_chars(s), plain.take_sentences(s), plain.bits_total(s), plain.demod_checksum_total(s)), (route, s)
    eng.close(); plain.close()


# ---------------------------------------------------------------- end to end: probe -> set_baud -> trial -> set_rtty -> decode

# Eight streams at /64.  The decimated rate is the smallest multiple of 300 baud's whole samples per bit that keeps baud_hi = 310 <= fsd / 3.5 with room
# for the 300-baud signal's low-pass (800 Hz): 2400 S/s, eight samples per bit at 300 baud; pushes of a tenth of a second.  baud_lo = 40 settles in 6.4 s:
# the probe phase is 7 s.  Stream 7 starts 3 s late: its first blocks are noise, whose many edges weigh the coherence down for a long time, so at 7 s it is
# not valid -- it is reset and probed again over the next 7 s, while the others are in their framing trial.
E2E = dict(fs=153600.0, n=15360, bw=800.0, baud_hi=310.0, t_a=70, t_b=140, t_c=170, t_end=205)
PAYLOADS = [(45.45, 7, 1.0, 0.0), (50.0, 7, 2.0, 0.0), (75.0, 7, 2.0, 0.0), (100.0, 8, 1.0, 0.0), (300.0, 8, 2.0, 0.0), (300.0, 7, 1.0, 0.0), None,
            (300.0, 8, 2.0, 3.0)]
FORMAT_INDEX = {(7, 1.0): 0, (7, 2.0): 1, (8, 1.0): 2, (8, 2.0): 3}


@pytest.fixture(scope="module")
def e2e_inputs(hd):
    """(iq [8, samples], per stream and checkpoint the host probe's estimate of the ORACLE's discriminator output).  The oracle alone must already say:
    every payload stream valid with the right nominal, the noise stream not."""
    from oracle import pyoracle
    fs, n = E2E["fs"], E2E["n"]
    total = n * E2E["t_end"]
    iq = np.zeros((8, total), np.complex64)
    for s, p in enumerate(PAYLOADS):
        if p is None:
            iq[s] = synth.fsk_iq(np.zeros(1, np.uint8), fs, 50.0, amp=0.0, sigma=0.05, seed=40 + s, n_samples=total)
            continue
        baud, nbits, nstops, late = p
        lead = int(late * fs)
        chars = int((total - lead) / fs * baud / (1 + nbits + nstops)) + 2
        text = "".join(synth.make_sentence(f"S{s}", str(k % 10)) for k in range(chars // 10 + 1))
        sig = synth.fsk_iq(synth.rtty_bits(text, nbits, int(nstops), 3, 0), fs, baud, sigma=0.05, seed=40 + s, n_samples=total - lead)
        iq[s, lead:] = sig
        if lead:
            iq[s, :lead] = synth.fsk_iq(np.zeros(1, np.uint8), fs, 50.0, amp=0.0, sigma=0.05, seed=90 + s, n_samples=lead)
    want = []
    for s in range(8):
        dec = pyoracle.Decoder("oracle", factor=64, baud=300, bits=8, stops=2, lowpass_bw=E2E["bw"], with_fft=False)
        hp = hd.HostBaudProbe(fs / 64, baud_hi=E2E["baud_hi"])
        est = {}
        for k in range(E2E["t_b"]):
            dec(iq[s, k * n:(k + 1) * n], fs)
            hp.push(dec.array("last_demod"))
            if k + 1 == E2E["t_a"]:
                est["a"] = hp.estimate()
                if s == 7:
                    hp.reset()
            if k + 1 == E2E["t_b"]:
                est["b"] = hp.estimate()
        want.append(est)
    for s, p in enumerate(PAYLOADS):
        when = "b" if s == 7 else "a"
        if p is None:
            assert not want[s]["a"]["valid"] and not want[s]["b"]["valid"], want[s]
        else:
            assert want[s][when]["valid"] and want[s][when]["nominal"] == p[0], (s, want[s])
    assert not want[7]["a"]["valid"], want[7]
    return iq, want


@pytest.mark.parametrize("arith", [0, 1], ids=["exact", "fast"])
def test_from_an_unknown_payload_to_its_sentences(hd, e2e_inputs, arith):
    iq, want = e2e_inputs
    fs, n = E2E["fs"], E2E["n"]
    eng = hd.Engine(n_streams=8, max_chunk=n, sampling_rate=fs, decimation=64, lowpass_bw_hz=E2E["bw"], arith=arith)      # every stream: 300 baud 8N2
    probe = eng.baud_probe(baud_hi=E2E["baud_hi"])
    got = []
    eng.on_sentence(lambda s, call, data, crc: got.append((s, call)))

    def check_estimate(s, when):
        e, w = probe.estimate(s), want[s][when]
        print(arith, s, when, e)
        if arith == 0:
            assert e == w, (s, when, e, w)                           # the same integers, the same doubles
        else:
            assert (e["nominal"], e["valid"], e["settled"]) == (w["nominal"], w["valid"], w["settled"]), (s, when, e, w)
        return e

    on_trial, decoding_from = set(), {}
    for k in range(E2E["t_end"]):
        eng.process_host(np.ascontiguousarray(iq[:, k * n:(k + 1) * n]))
        if k < E2E["t_b"]:
            probe.push_engine()
        if k + 1 == E2E["t_a"]:
            for s, p in enumerate(PAYLOADS):
                e = check_estimate(s, "a")
                if s == 7:
                    probe.reset(7)
                elif p is not None:
                    eng.set_baud(s, e["nominal"]); eng.set_format_trial(s, True); on_trial.add(s)
        if k + 1 == E2E["t_b"]:
            for s in (6, 7):
                e = check_estimate(s, "b")
            eng.set_baud(7, e["nominal"]); eng.set_format_trial(7, True)
        if k + 1 in (E2E["t_b"], E2E["t_c"]):
            for s in (sorted(on_trial) if k + 1 == E2E["t_b"] else [7]):
                r = eng.format_trial(s)
                print(arith, s, r)
                assert r["best"] == FORMAT_INDEX[PAYLOADS[s][1:3]] and r["sentences_ok"][r["best"]] >= 1, (s, r)
                eng.set_rtty(s, r["best_bits"], r["best_stops"]); eng.set_format_trial(s, False)
                decoding_from[s] = len(got)
    for s, p in enumerate(PAYLOADS):
        if p is not None:           # after set_rtty the next sentence arrives through the ordinary callback
            mine = [c for (t, c) in got[decoding_from[s]:] if t == s]
            assert mine and all(c == f"S{s}" for c in mine), (s, mine)
    assert not [1 for (t, c) in got if t == 6]
    with pytest.raises(hd.HabdecError):
        eng.format_trial(6)                                          # never turned on
    eng.close()


# ---------------------------------------------------------------- errors

def test_bad_parameters_small_buffers_and_null_arguments(hd):
    eng = hd.Engine(n_streams=2, sampling_rate=25600.0, decimation=64, baud=50, lowpass_bw_hz=150.0)        # fsd = 400
    for kw in (dict(), dict(baud_hi=400 / 3.5 * 1.001, baud_lo=20), dict(baud_lo=0, baud_hi=100), dict(baud_lo=100, baud_hi=100),
               dict(baud_lo=20, baud_hi=100, min_coherence=float("nan"))):
        with pytest.raises(hd.HabdecError):                          # (the default grid reaches 1300 baud: too high for this engine)
            eng.baud_probe(**kw)
    p = eng.baud_probe(baud_lo=20, baud_hi=400 / 3.5)
    L = eng.L
    p.push_host(np.ones((2, 100), np.float32))
    h, cand = capi.hd_baud_probe_stream_state(), np.full(1023 * 40, 0x55, np.uint8).view(capi.PROBE_CANDIDATE_DTYPE)
    h.samples = 777
    assert L.hd_baud_probe_state(p.h, 0, C.byref(h), cand.ctypes.data, 1023) == 1024            # too small: nothing is written
    assert h.samples == 777 and (cand.view(np.uint8) == 0x55).all()
    assert L.hd_baud_probe_state(p.h, 2, C.byref(h), None, 1024) == HD_ERR_INVALID
    assert L.hd_baud_probe_estimate(p.h, 0, None) == HD_ERR_INVALID and L.hd_baud_probe_estimate(p.h, 5, C.byref(capi.hd_baud_estimate())) == HD_ERR_INVALID
    assert L.hd_baud_probe_reset(p.h, 2) == HD_ERR_INVALID and L.hd_baud_probe_push_engine(None) == HD_ERR_INVALID
    host_rows = np.ones((2, 100), np.float32)
    assert L.hd_baud_probe_push_device(p.h, host_rows.ctypes.data, 100, None, 100) == HD_ERR_INVALID      # host memory is not device memory
    assert L.hd_baud_probe_push_host(p.h, None, 100, None, 100) == HD_ERR_INVALID
    n = np.array([101, 3], np.uint32)
    assert L.hd_baud_probe_push_host(p.h, host_rows.ctypes.data, 100, n.ctypes.data, 0) == HD_ERR_INVALID   # a row longer than the stride
    assert p.state(0)["samples"] == 100 and p.state(1)["samples"] == 100
    p.push_engine()                                                  # no call yet: adds nothing
    assert p.state(0)["samples"] == 100
    assert L.hd_stream_set_format_trial(eng.h, 2, 1) == HD_ERR_INVALID and L.hd_stream_format_trial(eng.h, 0, None) == HD_ERR_INVALID
    eng.close()


def test_a_probe_on_a_failed_engine_reports_the_device_error(torch):
    """The engine's failed state is entered the way tests/test_gpu_fault.py enters it: the fault build's stream tail that leaves its result slot untagged."""
    from test_gpu_fault import load_fault_lib
    L = load_fault_lib()
    S, CH = 64, 16384
    cfg = capi.hd_engine_config()
    L.hd_engine_config_default(C.byref(cfg))
    cfg.n_streams, cfg.max_chunk = S, CH
    h, p = C.c_void_p(), C.c_void_p()
    assert L.hd_engine_create(C.byref(cfg), C.byref(h)) == 0, L.hd_last_error()
    assert L.hd_baud_probe_create(h, None, C.byref(p)) == 0, L.hd_last_error()
    iq = torch.randn((S, CH, 2), device="cuda", dtype=torch.float32) * 0.1
    assert L.hd_process_device(h, iq.data_ptr(), CH, None, CH) == 0
    assert L.hd_baud_probe_push_engine(p) == 0
    L.hd_debug_tail_fault_arm_no_tag()
    assert L.hd_process_device(h, iq.data_ptr(), CH, None, CH) == HD_ERR_DEVICE
    est, rows = capi.hd_baud_estimate(), np.ones((S, 8), np.float32)
    assert L.hd_baud_probe_push_engine(p) == HD_ERR_DEVICE and b"failed state" in L.hd_last_error()
    assert L.hd_baud_probe_push_host(p, rows.ctypes.data, 8, None, 8) == HD_ERR_DEVICE
    assert L.hd_baud_probe_estimate(p, 0, C.byref(est)) == HD_ERR_DEVICE
    assert L.hd_baud_probe_reset(p, 0) == HD_ERR_DEVICE
    q = C.c_void_p()
    assert L.hd_baud_probe_create(h, None, C.byref(q)) == HD_ERR_DEVICE and not q.value
    L.hd_baud_probe_destroy(p)
    L.hd_engine_destroy(h)
