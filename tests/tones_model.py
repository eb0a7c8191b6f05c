"""A numpy model of the tone-filter demodulator, written from its definition (include/habdec_amd.h, "tone-filter demodulator") and not from the C++: what
hd_host_tones_push and the rows of hd_tones_* are held to byte for byte.  Also the signals the demodulator's tests share.

The model works on a whole stream at once: the definition speaks of absolute sample indices only, so how a stream is cut into pushes cannot matter."""
import math

import numpy as np

import baud_probe_model as M
from habdec_amd import synth

MAX_SPB = 2048
C_TABLE = np.array([int(np.rint(32767.0 * math.cos(2.0 * math.pi * a / 1024.0))) for a in range(1024)], np.int64)


def modem(fsd, baud, f_hi, f_lo, window_q8=160):
    """F, full, W, L and the two steps."""
    F = int(math.floor(fsd / baud * 65536 + 0.5))
    full = (F + 32768) >> 16
    W = max(1, (F * window_q8 + (1 << 23)) >> 24)
    step = [int(np.rint(f / fsd * 2.0 ** 32)) & 0xFFFFFFFF for f in (f_hi, f_lo)]       # np.rint: ties to even
    return dict(F=F, full=full, W=W, L=8 * full, step_hi=step[0], step_lo=step[1])


def quantise(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        q = np.trunc(np.clip(v, np.float32(-8.0), np.float32(8.0)).astype(np.float64) * 256.0)
    return np.where(np.isnan(v), 0.0, q).astype(np.int64)


def isqrt(x):
    """floor(sqrt(x)) of non-negative int64 below 2^52: the float64 estimate, settled by integer comparisons."""
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r -= (r * r > x)
    r += ((r + 1) * (r + 1) <= x)
    assert np.all(r * r <= x) and np.all((r + 1) * (r + 1) > x)
    return r


def window_sum(v, W):
    """sum of v[max(0, i + 1 - W) .. i] for every i"""
    c = np.concatenate([[0], np.cumsum(v)])
    i = np.arange(v.size)
    return c[i + 1] - c[np.maximum(i + 1 - W, 0)]


def integers(iq, fsd, baud, f_hi, f_lo, window_q8=160):
    """o of the definition for the samples iq since a reset, int64."""
    m = modem(fsd, baud, f_hi, f_lo, window_q8)
    iq = np.ascontiguousarray(iq, np.complex64)
    q_re, q_im = quantise(iq.real), quantise(iq.imag)
    i = np.arange(iq.size, dtype=np.uint64)
    A = []
    for step in (m["step_hi"], m["step_lo"]):
        theta = (i * np.uint64(step)) & np.uint64(0xFFFFFFFF)
        a = (theta >> np.uint64(22)).astype(np.int64)
        c, s = C_TABLE[a], C_TABLE[(a + 768) & 1023]
        r_re, r_im = (q_re * c + q_im * s) >> 15, (q_im * c - q_re * s) >> 15            # arithmetic shifts: floor
        s_re, s_im = window_sum(r_re, m["W"]), window_sum(r_im, m["W"])
        assert iq.size == 0 or max(np.abs(s_re).max(), np.abs(s_im).max()) < 1 << 23
        A.append(isqrt(s_re * s_re + s_im * s_im))
    N = window_sum(A[0] + A[1], m["L"])
    assert iq.size == 0 or N.max() < 1 << 39
    num, den = (A[0] - A[1]) * 1024 * m["L"], np.maximum(N, 1)
    o = np.sign(num) * (np.abs(num) // den)                                              # truncated toward zero
    return np.clip(o, -4096, 4096)


def demod(iq, fsd, baud, f_hi, f_lo, window_q8=160):
    """The row of floats, o / 1024."""
    return (integers(iq, fsd, baud, f_hi, f_lo, window_q8).astype(np.float64) / 1024.0).astype(np.float32)


# ---- signals: (name, iq, fsd, baud, f_hi, f_lo, window_q8)

SHIFT = 500.0                                               # synth.fsk_iq's default: mark (1) at +250 Hz, space at -250 Hz


def case_iq(case):
    """The IQ of a design signal of baud_probe_model.CASES: what baud_probe_model.case_signal discriminates."""
    name, baud, nbits, nstops, fsd, sigma, seconds, text = case
    text = M.telemetry_text(seconds, baud, nbits, nstops) if text is None else text
    bits = synth.rtty_bits(text, nbits, nstops, idle_before=3, idle_after=0)
    return synth.fsk_iq(bits, fsd, baud, sigma=sigma, seed=3, n_samples=int(seconds * fsd))


def specials_iq(n=6000, seed=11):
    """NaN, +-Inf, +-0, denormals, +-8 and beyond and a few ordinary values in both components, in a seeded order."""
    vals = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 8.0, -8.0, 8.000001, -8.000001, 1e30, -1e30, 7.998, -7.998,
                     1.0, -1.0, 0.5, -0.25, 3e-3, -3e-3, 0.00390625, -0.00390625, 0.0039, -0.0039], np.float32)
    idx = np.random.PCG64(seed).random_raw(2 * n) % np.uint64(vals.size)
    return vals[idx.astype(np.int64)].view(np.complex64)


def streams():
    out = []
    for c in M.CASES:
        out.append((c[0], case_iq(c), c[4], c[1], SHIFT / 2, -SHIFT / 2, 160))
    out.append(("specials", specials_iq(), 32000.0, 300.0, 250.0, -250.0, 160))
    # W = 1: 3.5 samples per bit and the shortest window; W = 2048 and L = 16384: 2048 samples per bit and the longest
    out.append(("w1", synth.fsk_iq(synth.rtty_bits("$$W1,1*ABCD\n" * 20, 8, 2, 3, 0), 2100.0, 600.0, sigma=0.1, seed=5, n_samples=9000), 2100.0, 600.0, 250.0, -250.0, 32))
    out.append(("w2048", synth.fsk_iq(synth.rtty_bits("$$A,1*ABCD\n", 8, 2, 3, 0), 32000.0, 15.625, sigma=0.3, seed=6, n_samples=150000), 32000.0, 15.625, 250.0, -250.0, 256))
    # tones at 0, just inside +-fsd / 2, and both negative
    noisy = synth.fsk_iq(synth.rtty_bits("$$T,2*ABCD\n" * 8, 8, 2, 3, 0), 8000.0, 300.0, f0=-250.0, sigma=0.2, seed=7, n_samples=20000)
    out.append(("tone_at_0", noisy, 8000.0, 300.0, 0.0, -500.0, 160))
    out.append(("tones_at_the_edges", noisy, 8000.0, 300.0, 3999.999, -3999.999, 160))
    out.append(("tones_negative", noisy * np.exp(-2j * np.pi * 1000.0 / 8000.0 * np.arange(noisy.size)).astype(np.complex64), 8000.0, 300.0, -1000.0, -1500.0, 192))
    return out


# ---- the weak signal of tests/test_gpu_clocked.py (WEAK): 8 streams, 32 kS/s decimated by 4, 300 baud 8N2, seeds 500 + s, 12 s
WEAK = dict(fs=32000.0, D=4, n=16000, calls=24, S=8, baud=300.0, bits=8, stops=2, bw=1500.0)


def weak_iq(sigma):
    """(iq [S, n * calls], the sentences sent per stream)"""
    S, n = WEAK["S"], WEAK["n"] * WEAK["calls"]
    iq, sent = np.zeros((S, n), np.complex64), []
    for s in range(S):
        text = "".join(synth.make_sentence(f"W{s}", "%d,12:00:%02d,52.%04d,-0.1234,%d" % (k, k, 1000 + s * 7 + k, 100 * k)) for k in range(12))
        sent.append({t.strip("$\n") for t in text.split("\n") if t})
        iq[s] = synth.fsk_iq(synth.rtty_bits(text, 8, 2, 3, 0), WEAK["fs"], WEAK["baud"], sigma=sigma, seed=500 + s, n_samples=n)
    return iq, sent


def weak_oracle(iq):
    """Per stream: (the oracle's sentences, its last_decimated per call, its last_demod per call)."""
    from oracle import pyoracle
    out = []
    for s in range(iq.shape[0]):
        dec = pyoracle.Decoder("oracle", factor=WEAK["D"], baud=WEAK["baud"], bits=WEAK["bits"], stops=WEAK["stops"], lowpass_bw=WEAK["bw"], with_fft=False)
        decim, demod_rows = [], []
        for k in range(WEAK["calls"]):
            dec(iq[s, k * WEAK["n"]:(k + 1) * WEAK["n"]], WEAK["fs"])
            decim.append(dec.array("last_decimated"))
            demod_rows.append(dec.array("last_demod"))
        out.append((dec.sentences(), decim, demod_rows))
    return out
