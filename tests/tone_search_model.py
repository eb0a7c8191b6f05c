"""A numpy float64 model of the tone search, written from its definition (include/habdec_amd.h, "tone search"; include/habdec_amd_host.h,
hd_host_tone_search_detect) and not from the C++: what hd_host_tone_search_* is held to closely and the rows of hd_tone_search_* within the survey's gate.
Also the signals the tone search's tests share.

The spectrum works on a whole stream at once: the definition speaks of absolute sample indices only, so how a stream is cut into pushes cannot matter."""
import math

import numpy as np

import baud_probe_model as M
from habdec_amd import synth

N, HOP = 4096, 2048
HD_ERR_INVALID, HD_ERR_UNSUPPORTED = -1, -3


def window():
    """The periodic Hann float table of hd_host_survey_window."""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32)


def sum_w2():
    s = 0.0
    for v in window():
        s += float(v) * float(v)                                   # in table order
    return s


def segments_of(n):
    return 0 if n < N else 1 + (n - N) // HOP


def periodograms(x):
    """|FFT|^2 of every whole segment of the STREAM x, fftshifted, [segments, 4096] float64, not normalised: one rounded float product per part with the
    window, then the transform in double."""
    x = np.ascontiguousarray(x, np.complex64)
    w = window()
    out = np.zeros((segments_of(x.size), N))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(out.shape[0]):
            seg = x[j * HOP:j * HOP + N]
            re, im = (seg.real * w).astype(np.float32), (seg.imag * w).astype(np.float32)
            X = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64))
            out[j] = np.fft.fftshift(X.real ** 2 + X.imag ** 2)
    return out


def spectrum(x):
    """(power[4096], segments, Ppk, carry length): the accumulation in segment order; Ppk = the largest single-segment bin power, normalised like the average."""
    pg = periodograms(x)
    acc = np.zeros(N)
    for row in pg:
        acc = acc + row
    k = pg.shape[0]
    sw2 = sum_w2()
    with np.errstate(invalid="ignore"):
        p = acc / (k * sw2) if k else acc
    ppk = float(np.max(pg)) / sw2 if k else 0.0
    return p, k, ppk, len(x) - HOP * k


def detect(P, segments, fsd, baud, shift_lo_hz=170.0, shift_hi_hz=1000.0, min_quality=0.5):
    """The detector of habdec_amd_host.h, step by step: a dict as habdec_amd.tone_search_detect gives, or the error code."""
    P = [float(v) for v in P]
    par = (baud, fsd, shift_lo_hz, shift_hi_hz, min_quality)
    if any(math.isnan(v) or math.isinf(v) for v in par) or not baud > 0 or not fsd > 0 or not shift_lo_hz > 0 or not shift_hi_hz >= shift_lo_hz or min_quality < 0:
        return HD_ERR_INVALID
    if segments < 8:
        return HD_ERR_UNSUPPORTED
    b = fsd / N
    wd = max(1.0, float(np.rint(0.5 * baud / b)))
    if wd >= N:
        return HD_ERR_INVALID
    w = int(wd) | 1
    h = w // 2
    d0, d1 = math.ceil(shift_lo_hz / b), min(math.floor(shift_hi_hz / b), N - w)
    if d0 < 1 or d0 > d1:
        return HD_ERR_INVALID
    out = dict(f_hi_hz=0.0, f_lo_hz=0.0, quality=0.0, floor=0.0, segments=segments, bin_lo=0, shift_bins=0, w=w, valid=0)
    if not all(math.isfinite(v) for v in P):
        return out
    srt = sorted(P)
    floor = 0.5 * (srt[N // 2 - 1] + srt[N // 2])
    B = [0.0] * N
    for k in range(h, N - h):
        s = 0.0
        for m in range(k - h, k + h + 1):
            s += P[m] - floor
        B[k] = s
    Ba = np.array(B)
    score, lo_best, d_best = -math.inf, h, d0
    for d in range(d0, d1 + 1):
        sc = np.minimum(Ba[h:N - h - d], Ba[h + d:N - h])             # lo = h .. N - h - d - 1
        i = int(np.argmax(sc))                                        # the first greatest of this d
        if sc[i] > score:
            score, lo_best, d_best = float(sc[i]), h + i, d
    r = int(max(1.0, float(np.rint(0.3 * baud / b))))
    tones = []
    for c in (lo_best, lo_best + d_best):
        cf = float(c)
        for _ in range(3):
            sw = sm = 0.0
            for m in range(max(c - r, 0), min(c + r, N - 1) + 1):
                wt = max(P[m] - floor, 0.0)
                sw += wt
                sm += m * wt
            cf = sm / sw if sw > 0 else float(c)
            c = int(np.rint(cf))                                      # ties to even
        tones.append((cf - N // 2) * b)
    quality = score / (w * floor) if floor > 0 else 0.0
    valid = int(floor > 0 and quality >= max(min_quality, 10.0 / math.sqrt(w * segments)))
    out.update(f_lo_hz=tones[0], f_hi_hz=tones[1], quality=quality, floor=floor, bin_lo=lo_best, shift_bins=d_best, valid=valid)
    return out


# ---- signals.  ACCURACY: (name, baud, nbits, nstops, fsd, sigma, seconds, f0, shift_lo_hz, shift_hi_hz); the tones sent are f0 +- SHIFT / 2
SHIFT = 500.0
SEEDS = (3, 4)
ACCURACY = [
    ("50_7n2_s0.5", 50.0, 7, 2, 8000.0, 0.5, 20.0, 0.0, 300.0, 700.0),
    ("50_7n2_s1.0_off", 50.0, 7, 2, 8000.0, 1.0, 20.0, 562.3, 170.0, 1000.0),
    ("300_8n2_8k", 300.0, 8, 2, 8000.0, 0.35, 12.0, -1311.7, 170.0, 1000.0),
    ("300_8n2_39k", 300.0, 8, 2, 39062.5, 2.0, 3.0, 1000.0, 300.0, 700.0),
    ("50_7n2_39k", 50.0, 7, 2, 39062.5, 2.0, 6.0, 1000.0, 300.0, 700.0),
    ("100_8n1", 100.0, 8, 1, 8000.0, 0.5, 10.0, 0.0, 300.0, 700.0),
]


def signal(case, seed):
    name, baud, nbits, nstops, fsd, sigma, seconds, f0, _, _ = case
    bits = synth.rtty_bits(M.telemetry_text(seconds, baud, nbits, nstops), nbits, nstops, idle_before=3, idle_after=0)
    return synth.fsk_iq(bits, fsd, baud, f0=f0, sigma=sigma, seed=seed, n_samples=int(seconds * fsd))


def noise(n, sigma, seed):
    nz = synth._noise(n, seed)
    return (sigma * (nz[0::2] + 1j * nz[1::2])).astype(np.complex64)


def carrier(fsd, f, sigma, seconds, seed, amp=0.5):
    n = int(seconds * fsd)
    return (amp * np.exp(2j * np.pi * f / fsd * np.arange(n)) + noise(n, sigma, seed)).astype(np.complex64)
