"""A numpy model of the baud-rate probe, written from its definition (include/habdec_amd.h, "baud-rate probe") and not from the C++: what
hd_host_baud_probe_state and hd_baud_probe_state are held to integer for integer.  Also the signals the probe's tests share.

The model works on a whole stream at once: the definition speaks of absolute sample indices only, so how a stream is cut into pushes cannot matter."""
import math

import numpy as np

from habdec_amd import synth

WINDOWS = (1, 3, 7, 15, 31, 63, 127, 255, 511)
K = 1024
FIELDS = ("P", "Q", "NB", "re", "im", "n", "cur_block")


def tables(fsd, baud_lo=40.0, baud_hi=1300.0):
    """b_k, F_k, the scale index of every candidate and the cosine table."""
    b = [baud_lo * math.pow(baud_hi / baud_lo, k / 1023) for k in range(K)]
    F = [int(math.floor(x / fsd * 2.0 ** 32 + 0.5)) for x in b]
    scale = []
    for f in F:
        lim = max(1.0, (2.0 ** 32 / f) / 4.0)
        scale.append(max(i for i, w in enumerate(WINDOWS) if w <= lim))
    C = np.array([int(np.rint(32767.0 * math.cos(2.0 * math.pi * a / 1024.0))) for a in range(1024)], np.int64)
    return np.array(b), F, scale, C


def sign_bits(d):
    with np.errstate(invalid="ignore"):
        return (np.asarray(d, np.float32) > np.float32(0.0)).astype(np.int64)      # NaN gives 0


def majority_edges(bits, W):
    """(m_W per sample, the indices at which an edge of scale W stands)"""
    n = bits.size
    csum = np.concatenate([[0], np.cumsum(bits)])
    i = np.arange(n, dtype=np.int64)
    m = (csum[i + 1] - csum[np.maximum(i + 1 - W, 0)]) > (W - 1) // 2               # bits in front of the first sample are 0
    return m, np.flatnonzero((m != np.concatenate([[False], m[:-1]])) & (i >= W)).astype(np.uint64)


def state(d, fsd, baud_lo=40.0, baud_hi=1300.0):
    """The state after the samples d since a reset, as the dict habdec_amd.engine._probe_state makes of the C structs."""
    d = np.asarray(d, np.float32)
    n = d.size
    bits = sign_bits(d)
    _, F, scale, C = tables(fsd, baud_lo, baud_hi)
    out = {k: np.zeros(K, np.uint64 if k in ("P", "Q") else np.int32 if k in ("re", "im") else np.uint32) for k in FIELDS}
    edges, majority = np.zeros(9, np.uint64), np.zeros(9, np.uint32)
    for sc, W in enumerate(WINDOWS):
        m, e = majority_edges(bits, W)
        edges[sc] = e.size
        majority[sc] = int(m[-1]) if n else 0
        if not e.size:
            continue
        for k in (k for k in range(K) if scale[k] == sc):
            p = e * np.uint64(F[k])                                              # mod 2^64
            idx = ((p >> np.uint64(22)) & np.uint64(1023)).astype(np.int64)
            block = (p >> np.uint64(38)).astype(np.uint32)
            # runs of edges in one block; the first run goes on from cur_block = 0, n = 0, which is a fresh block either way
            start = np.concatenate([[0], np.flatnonzero(block[1:] != block[:-1]) + 1])
            stop = np.concatenate([start[1:], [e.size]])
            counted = np.minimum(stop, start + 4096)                             # the sums stop at the 4096th edge of a block, n goes on
            cre = np.concatenate([[0], np.cumsum(C[idx])])
            cim = np.concatenate([[0], np.cumsum(C[(idx + 768) & 1023])])
            re, im, cnt = cre[counted] - cre[start], cim[counted] - cim[start], stop - start
            closed = slice(0, len(start) - 1)                                    # every run but the last has been dumped
            ok = (cnt[closed] >= 8) & (cnt[closed] <= 4096)
            out["P"][k] = sum(int(a) * int(a) + int(c) * int(c) for a, c in zip(re[closed][ok], im[closed][ok])) % 2 ** 64
            out["Q"][k] = sum(int(a) * int(a) for a in cnt[closed][ok]) % 2 ** 64
            out["NB"][k] = int(ok.sum())
            out["re"][k], out["im"][k], out["n"][k], out["cur_block"][k] = re[-1], im[-1], cnt[-1], block[-1]
    hist = [0] * 8
    for j in range(max(0, n - 512), n):                                          # circular by absolute index: the newest 512 samples
        if bits[j]:
            hist[(j >> 6) & 7] |= 1 << (j & 63)
    out.update(samples=n, edges=edges, majority=majority, history=np.array(hist, np.uint64))
    return out


def assert_same_state(a, b, what=""):
    for k in FIELDS + ("edges", "majority", "history"):
        assert np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)), (what, k, np.flatnonzero(np.asarray(a[k]) != np.asarray(b[k]))[:8])
    assert a["samples"] == b["samples"], (what, a["samples"], b["samples"])


# ---- signals: synth.fsk_iq at the decimated rate, a 161-tap 1500 Hz low-pass and a polar discriminator

def telemetry_text(seconds, baud, nbits, nstops):
    """Sentences with a running counter, enough of them for `seconds` of signal."""
    chars = int(seconds * baud / (1 + nbits + nstops)) + 2
    text, k = "", 0
    while len(text) < chars:
        text += synth.make_sentence("PROBE%d" % (k % 7), "%d,12:%02d:%02d,52.%04d,-0.%04d,%d" % (k, k % 60, (7 * k) % 60, 1234 + 37 * k, 5678 - 11 * k, 100 * k))
        k += 1
    return text


def lowpass161(fsd, cutoff=1500.0):
    t = np.arange(161) - 80
    h = np.sinc(2.0 * cutoff / fsd * t) * np.hamming(161)
    return h / h.sum()


def discriminate(iq, fsd):
    y = np.convolve(iq.astype(np.complex128), lowpass161(fsd), mode="same")
    return np.angle(y[1:] * np.conj(y[:-1])).astype(np.float32)


def fsk_demod(baud, nbits, nstops, fsd, sigma, seconds, text=None, seed=3, lead_s=0.0):
    """Discriminator output of `seconds` of an RTTY stream (after lead_s seconds of noise alone)."""
    text = telemetry_text(seconds, baud, nbits, nstops) if text is None else text
    bits = synth.rtty_bits(text, nbits, nstops, idle_before=3, idle_after=0)
    n = int(seconds * fsd)
    iq = synth.fsk_iq(bits, fsd, baud, sigma=sigma, seed=seed, n_samples=n)
    if lead_s:
        iq = np.concatenate([synth.fsk_iq(np.zeros(1, np.uint8), fsd, baud, amp=0.0, sigma=sigma, seed=seed + 1, n_samples=int(lead_s * fsd)), iq])
    return discriminate(iq, fsd)


def noise_demod(fsd, sigma, seconds, seed=5):
    return discriminate(synth.fsk_iq(np.zeros(1, np.uint8), fsd, 50.0, amp=0.0, sigma=sigma, seed=seed, n_samples=int(seconds * fsd)), fsd)


# The signals the probe was designed against: (name, baud, data bits, stop bits, fsd, sigma, seconds, text).  `settled` asks for four blocks of the lowest
# candidate, 256 / baud_lo seconds: the runs shorter than 6.4 s set baud_lo to what their length settles (baud_lo_for), the others keep the default 40.
CASES = [
    ("50_7n2", 50.0, 7, 2, 32000.0, 0.05, 10.0, None),
    ("45_7n1", 45.45, 7, 1, 32000.0, 0.3, 10.0, None),
    ("100_8n1", 100.0, 8, 1, 39062.5, 0.3, 8.0, None),
    ("110_8n2", 110.0, 8, 2, 32000.0, 0.2, 5.0, None),
    ("150_7n1", 150.0, 7, 1, 32000.0, 0.2, 5.0, None),
    ("200_8n1", 200.0, 8, 1, 32000.0, 0.2, 5.0, None),
    ("300_8n2_32k", 300.0, 8, 2, 32000.0, 0.05, 4.0, None),
    ("300_8n2_156k", 300.0, 8, 2, 156250.0, 0.3, 2.0, None),
    ("600_8n2", 600.0, 8, 2, 32000.0, 0.1, 3.0, None),
    ("50_U", 50.0, 8, 2, 32000.0, 0.3, 10.0, "U" * 60),
    ("50_space", 50.0, 8, 2, 32000.0, 0.3, 10.0, " " * 60),
]


def baud_lo_for(seconds):
    """40, or the lowest candidate whose four blocks (256 / baud_lo seconds) fit into a shorter run, with a margin of two percent."""
    return 40.0 if seconds * 40.0 / 64.0 >= 4.08 else 256.0 / seconds * 1.02


def case_signal(case):
    name, baud, nbits, nstops, fsd, sigma, seconds, text = case
    return fsk_demod(baud, nbits, nstops, fsd, sigma, seconds, text)


def specials_row(n=6000, seed=11):
    """NaN, +-Inf, +-0, denormals of both signs and a few ordinary values, in a seeded order."""
    vals = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0, 3e-3, -3e-3], np.float32)
    idx = np.random.PCG64(seed).random_raw(n) % np.uint64(vals.size)
    return vals[idx.astype(np.int64)]


def capped_blocks(fsd=32000.0, baud_lo=40.0, baud_hi=1300.0):
    """A square wave of period two samples makes an edge at every sample on every scale (an odd window over alternating bits holds one more or one
    fewer ones than zeros).  Bursts of it inside blocks 1 .. 5 of the lowest candidate, silence elsewhere: exactly 4096 edges of that candidate's
    scale in block 1, 4097 in block 2 (a burst's edges come in pairs, so the odd one is a rise to a level held into block 3, where it falls: 101
    there), 100 each in blocks 4 and 5.  Returns (signal, the edge counts per block of candidate 0)."""
    _, F, scale, _ = tables(fsd, baud_lo, baud_hi)
    W = WINDOWS[scale[0]]
    block_len = 2.0 ** 38 / F[0]
    d = -np.ones(int(6 * block_len), np.float32)
    for blk, want in ((1, 4096), (2, 4096), (3, 100), (4, 100), (5, 100)):
        at = int(blk * block_len) + 600
        for length in range(want + W - 4, want + W + 5):           # (the window has to fill before the majority starts to alternate)
            burst = np.zeros(length + 2 * W + 8, np.int64)
            burst[W + 4:W + 4 + length:2] = 1
            if majority_edges(burst, W)[1].size == want:
                break
        d[at:at + length:2] = 1.0
    d[int(2 * block_len) + 10000:int(3 * block_len) + 300] = 1.0
    _, e = majority_edges(sign_bits(d), W)
    counts = np.bincount(((e * np.uint64(F[0])) >> np.uint64(38)).astype(np.int64), minlength=6)
    return d, counts
