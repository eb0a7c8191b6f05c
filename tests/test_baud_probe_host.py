"""The baud-rate probe and the framing trial on the host (hd_host_baud_probe_*, hd_host_format_trial_*; no GPU).

State: hd_host_baud_probe_state equals the numpy model of the definition (tests/baud_probe_model.py) integer for integer -- the accumulators are
integer sums, so there is no tolerance.  Estimate: on the signals the probe was designed against (synth.fsk_iq at the decimated rate, a 161-tap 1500 Hz
low-pass, a polar discriminator) `valid` is set, |baud / true - 1| <= 0.5 % (1.5 steps of the 0.34 % candidate grid) and `nominal` is exact.  The
design runs shorter than 6.4 s cannot be `settled` on a grid that starts at 40 baud (four blocks of the lowest candidate are 256 / baud_lo seconds), so
they raise baud_lo to what their length settles (baud_probe_model.baud_lo_for): 52 for the 5 s runs, 65, 87 and 131 for 4, 3 and 2 s."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import baud_probe_model as M
from oracle import pyoracle

ROOT = Path(__file__).resolve().parent.parent
PUSHES = (1, 63, 64, 65, 511, 512, 4097)      # every scale's window and the kernel's 64-sample step straddle a push boundary


@pytest.fixture(scope="module")
def hd():
    from habdec_amd.build import build
    build()
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def signals():
    return {c[0]: M.case_signal(c) for c in M.CASES}


def push_cut(probe, d, sizes=PUSHES):
    at, turn = 0, 0
    while at < d.size:
        n = sizes[turn % len(sizes)]
        probe.push(d[at:at + n])
        at += n
        turn += 1


@pytest.fixture(scope="module")
def probed(hd, signals):
    """One host probe per design signal, fed in cut pushes: (state, estimate)"""
    out = {}
    for c in M.CASES:
        p = hd.HostBaudProbe(c[4], baud_lo=M.baud_lo_for(c[6]))
        push_cut(p, signals[c[0]])
        out[c[0]] = (p.state(), p.estimate())
        p.close()
    return out


@pytest.mark.parametrize("case", M.CASES, ids=[c[0] for c in M.CASES])
def test_state_equals_the_model_on_the_design_signals(probed, signals, case):
    """(a): the pushes are cut into 1, 63, 64, 65, 511, 512 and 4097 samples; the model sees the whole stream."""
    M.assert_same_state(probed[case[0]][0], M.state(signals[case[0]], case[4], M.baud_lo_for(case[6])), case[0])


def test_state_on_nan_inf_zero_and_denormals(hd):
    """(b): only d > 0.0f counts: NaN, -Inf and both zeros give 0, the positive denormals give 1."""
    d = M.specials_row()
    assert np.isnan(d).any() and np.isinf(d).any() and (d == 0).any() and ((d != 0) & (np.abs(d) < 1e-38)).any()
    p = hd.HostBaudProbe(32000.0)
    push_cut(p, d)
    M.assert_same_state(p.state(), M.state(d, 32000.0), "specials")
    assert int(M.sign_bits(np.array([1e-45, -1e-45, 0.0, -0.0, np.nan, np.inf, -np.inf], np.float32)).sum()) == 2


def test_block_cap_4096_counts_and_4097_does_not(hd):
    """(c): a block with exactly 4096 edges is dumped into P, Q and NB, one with 4097 is dropped."""
    d, counts = M.capped_blocks()
    assert list(counts) == [0, 4096, 4097, 101, 100, 100]
    p = hd.HostBaudProbe(32000.0)
    push_cut(p, d)
    st, model = p.state(), M.state(d, 32000.0)
    M.assert_same_state(st, model, "cap")
    # candidate 0: blocks 1, 3 and 4 are in (block 2 is over the cap, block 5 is still open)
    assert int(st["NB"][0]) == 3 and int(st["Q"][0]) == 4096 ** 2 + 101 ** 2 + 100 ** 2 and int(st["n"][0]) == 100 and int(st["cur_block"][0]) == 5


def test_reset_in_mid_stream(hd, signals):
    """(d): after a reset the state is that of the samples behind it alone."""
    d = signals["600_8n2"]
    p = hd.HostBaudProbe(32000.0)
    push_cut(p, d[:33333])
    p.reset()
    push_cut(p, d[33333:])
    M.assert_same_state(p.state(), M.state(d[33333:], 32000.0), "reset")


def test_estimates_of_the_design_signals(probed):
    worst = 0.0
    for c in M.CASES:
        est = probed[c[0]][1]
        err = est["baud"] / c[1] - 1.0
        print(f"{c[0]}: baud {est['baud']:.4f} ({100 * err:+.4f} %), rho {est['rho']:.4f}, rho_max {est['rho_max']:.4f}, nominal {est['nominal']}")
        assert est["valid"] and est["settled"], (c[0], est)
        if c[7] is not None:           # one character over and over is periodic at its character rate too: asserted to be valid, not to be right
            continue
        worst = max(worst, abs(err))
        assert abs(err) <= 0.005, (c[0], est)
        assert est["nominal"] == c[1], (c[0], est)
    print(f"worst |baud / true - 1| = {100 * worst:.4f} %")


def test_no_estimate_from_noise_heavy_noise_or_a_short_run(hd):
    for name, d in (("noise", M.noise_demod(32000.0, 0.3, 10.0)), ("sigma 1.0", M.fsk_demod(50.0, 7, 2, 32000.0, 1.0, 10.0))):
        p = hd.HostBaudProbe(32000.0)
        p.push(d)
        est = p.estimate()
        print(name, est)
        assert est["settled"] and not est["valid"] and est["rho_max"] < 0.1, (name, est)
    p = hd.HostBaudProbe(32000.0)
    p.push(M.fsk_demod(50.0, 7, 2, 32000.0, 0.05, 3.0))
    est = p.estimate()
    print("3 s of 50 baud", est)
    assert not est["settled"] and not est["valid"], est


def test_bad_parameters_are_refused(hd):
    for kw in (dict(baud_lo=0.0), dict(baud_lo=-1.0), dict(baud_lo=1300.0), dict(baud_hi=32000.0 / 3.5 * 1.001), dict(min_coherence=float("nan")),
               dict(baud_lo=float("nan"))):
        with pytest.raises(hd.HabdecError):
            hd.HostBaudProbe(32000.0, **kw)
    hd.HostBaudProbe(32000.0, baud_hi=32000.0 / 3.5).close()
    # a state buffer that is too small: nothing is written
    from habdec_amd import capi
    import ctypes as C
    p = hd.HostBaudProbe(32000.0)
    p.push(np.ones(100, np.float32))
    h, cand = capi.hd_baud_probe_stream_state(), np.full(1023, 0x55, np.uint8).repeat(40).view(capi.PROBE_CANDIDATE_DTYPE)
    h.samples = 777
    assert p.L.hd_host_baud_probe_state(p.h, C.byref(h), cand.ctypes.data, 1023) == 1024
    assert h.samples == 777 and (cand.view(np.uint8) == 0x55).all()


# ---- framing trial

FS_TRIAL, FACTOR_TRIAL, BAUD_TRIAL = 128000.0, 4, 300.0
FORMATS = [(7, 1.0), (7, 2.0), (8, 1.0), (8, 2.0)]


def oracle_bits(iq, nbits, nstops, chunk=16384):
    """the bits the CPU oracle's symbol extractor makes of a stream, call by call"""
    dec = pyoracle.Decoder("oracle", factor=FACTOR_TRIAL, baud=BAUD_TRIAL, bits=nbits, stops=nstops, with_fft=False)
    out = []
    for at in range(0, len(iq) - chunk + 1, chunk):
        dec(iq[at:at + chunk], FS_TRIAL)
        out.append(dec.bits())
    return np.concatenate(out), dec.sentences()


def two_sentences():
    from habdec_amd import synth
    return synth.make_sentence("TRIAL", "1,12:00:01,52.1,-0.2,100") + synth.make_sentence("TRIAL", "2,12:00:09,52.2,-0.3,220")


@pytest.mark.parametrize("fmt", range(4), ids=["7n1", "7n2", "8n1", "8n2"])
def test_trial_finds_the_format_sent(hd, fmt):
    from habdec_amd import synth
    nbits, nstops = FORMATS[fmt]
    iq = synth.fsk_iq_for_text(two_sentences(), FS_TRIAL, BAUD_TRIAL, nbits, int(nstops), chunk=16384, sigma=0.05, seed=fmt)
    bits, sentences = oracle_bits(iq, nbits, nstops)
    assert len(sentences) == 2, sentences               # the oracle itself decodes both
    t = hd.HostFormatTrial()
    for at in range(0, bits.size, 97):                  # (uneven pieces)
        t.push_bits(bits[at:at + 97])
    r = t.get()
    print(FORMATS[fmt], r)
    assert r["best"] == fmt and r["best_bits"] == nbits and r["best_stops"] == nstops and r["sentences_ok"][fmt] == 2, r
    if fmt == 1:            # the tie rule: a one-stop framer frames the two-stop signal as well, the stricter format wins
        assert r["sentences_ok"][0] == r["sentences_ok"][1] == 2, r


def test_trial_of_noise_bits_has_no_answer(hd):
    from habdec_amd import synth
    iq = synth.fsk_iq(np.zeros(1, np.uint8), FS_TRIAL, BAUD_TRIAL, amp=0.0, sigma=0.3, seed=9, n_samples=16384 * 24)
    bits, sentences = oracle_bits(iq, 8, 2.0)
    assert bits.size > 500 and not sentences
    t = hd.HostFormatTrial()
    t.push_bits(bits)
    r = t.get()
    assert r["best"] == -1 and r["best_bits"] == 0 and sum(r["sentences_ok"]) == 0, r


# ---- the host code under the sanitizers: a stand-alone program, nothing loaded into Python

def test_host_code_under_address_and_ub_sanitizers(hd, signals, probed, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ (the compiler the oracle is built with) is needed"
    exe = tmp_path / "baud_probe_asan"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "habdec_amd" / "csrc"),
           str(ROOT / "tests" / "cpp" / "baud_probe_asan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("50_7n2", "600_8n2"):
        case = next(c for c in M.CASES if c[0] == name)
        f = tmp_path / (name + ".f32")
        signals[name].tofile(f)
        r = subprocess.run([str(exe), str(f), repr(case[4]), repr(M.baud_lo_for(case[6]))] + [str(n) for n in PUSHES], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "baud_probe_asan OK" in r.stdout, (name, r.stdout[-500:], r.stderr[-3000:])
        st, est = probed[name]
        got = [int(x) for x in r.stdout.splitlines()[0].split()[1:]]
        mod = 2 ** 64
        want = [st["samples"], int(st["edges"].astype(object).sum()), int(st["P"].astype(object).sum()) % mod, int(st["Q"].astype(object).sum()) % mod,
                int(st["NB"].astype(object).sum()), int(st["n"].astype(object).sum()), int(st["re"].astype(object).sum()) % mod,
                int(st["im"].astype(object).sum()) % mod]
        assert got == want, (name, got, want)
        assert float(r.stdout.splitlines()[1].split()[1]) == est["baud"], (name, r.stdout)
