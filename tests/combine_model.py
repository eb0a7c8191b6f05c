"""A numpy model of the diversity combiner, written from its definition (include/habdec_amd.h, "diversity combiner") and not from the C++: what
hd_host_combine_* and the rows, scores and results of hd_combine_* are held to byte for byte.  Also the signals the combiner's tests share.

The model works on whole rows at once: the definition speaks of absolute sample indices only, so how a row is cut into pushes cannot matter."""
import functools

import numpy as np

import tones_model as TM
from habdec_amd import synth

MAX_MEMBERS, MAX_DELAY, RING = 8, 8192, 32768


def quantise(v):
    """The clocked decoder's rule: 0 for NaN, else (int32)(clamp(v, -4, 4) * 1024) truncated toward zero."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        q = np.trunc(np.clip(v, np.float32(-4.0), np.float32(4.0)).astype(np.float64) * 1024.0)
    return np.where(np.isnan(v), 0.0, q).astype(np.int64)


def integers(rows, schedule):
    """o of the definition.  rows: float32 [M, n] since a reset; schedule: [(from index, delays [M], weights [M])], ascending, the first from index 0 --
    delays and weights hold from the push that starts at their index on."""
    rows = np.atleast_2d(np.asarray(rows, np.float32))
    M, n = rows.shape
    q = quantise(rows)
    o = np.zeros(n, np.int64)
    for k, (start, delays, weights) in enumerate(schedule):
        end = schedule[k + 1][0] if k + 1 < len(schedule) else n
        j = np.arange(start, end)
        total = np.zeros(j.size, np.int64)
        for m in range(M):
            assert 0 <= delays[m] <= MAX_DELAY and 0 <= weights[m] <= 256
            i = j - delays[m]
            total += weights[m] * np.where(i >= 0, q[m, np.maximum(i, 0)], 0)
        assert j.size == 0 or np.abs(total).max() <= 1 << 23
        wt = max(1, int(np.sum(weights)))
        o[start:end] = np.sign(total) * (np.abs(total) // wt)                             # truncated toward zero
    return o


def combine(rows, schedule):
    """The row of floats, o / 1024."""
    return (integers(rows, schedule).astype(np.float64) / 1024.0).astype(np.float32)


def lag_scores(row_r, row_m, N, L):
    """c(l) for l = -L .. L over the n samples both rows hold (n >= N + 2 L), int64 [2 L + 1]."""
    b_r, b_m = quantise(row_r) > 0, quantise(row_m) > 0
    n = b_r.size
    assert b_m.size == n and n >= N + 2 * L
    ref = b_r[n - L - N:n - L]
    out = np.zeros(2 * L + 1, np.int64)
    for l in range(-L, L + 1):
        out[l + L] = 2 * int(np.count_nonzero(ref == b_m[n - L - N + l:n - L + l])) - N
    return out


def lag_result(scores, N, L, guard, min_peak_q8=76, min_margin_q8=16):
    """(lag, peak, second, valid) of one member's scores."""
    l = np.arange(-L, L + 1)
    peak = int(scores.max())
    ties = l[scores == peak]
    ties = ties[np.abs(ties) == np.abs(ties).min()]
    lag = int(ties.min())                                                                  # the negative one of +-l
    far = np.abs(l - lag) > guard
    second = int(scores[far].max()) if far.any() else -N
    valid = 256 * peak >= min_peak_q8 * N and 256 * (peak - second) >= min_margin_q8 * N
    return lag, peak, second, bool(valid)


def align(results, delays, weights):
    """The align step: results [(lag, valid)] per member, the reference's (0, True) first.  Returns (delays, weights, how many are valid)."""
    top = max([0] + [lag for lag, valid in results if valid])
    delays, weights = list(delays), list(weights)
    for m, (lag, valid) in enumerate(results):
        if valid:
            delays[m] = top - lag
        else:
            weights[m] = 0
    return delays, weights, sum(1 for _, valid in results if valid)


# ---- signals

def specials_row(n=6000, seed=12):
    """NaN, +-Inf, +-4 and beyond, denormals, +-0 and a few ordinary values, in a seeded order."""
    vals = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 4.0, -4.0, 4.000001, -4.000001, 1e30, -1e30, 3.9995, -3.9995,
                     1.0, -1.0, 0.5, -0.25, 3e-3, -3e-3, 0.0009765625, -0.0009765625, 0.00097, -0.00097], np.float32)
    idx = np.random.PCG64(seed).random_raw(n) % np.uint64(vals.size)
    return vals[idx.astype(np.int64)]


def random_rows(M, n, seed):
    """Rows of quantised-looking floats in about [-1.5, 1.5] with every eighth sample a special."""
    raw = np.random.PCG64(seed).random_raw(M * n).reshape(M, n)
    rows = (((raw >> np.uint64(11)) % np.uint64(3073)).astype(np.float64) / 1024.0 - 1.5).astype(np.float32)
    sp = specials_row(M * n, seed + 1).reshape(M, n)
    mask = (raw & np.uint64(7)) == 0
    rows[mask] = sp[mask]
    return rows


def random_signs(n, seed):
    """n samples of random sign and an amplitude in [0.25, 0.75)."""
    r = np.random.PCG64(seed).random_raw(n)
    amp = 0.25 + ((r >> np.uint64(30)) % np.uint64(512)).astype(np.float64) / 1024.0
    return (np.where(r & np.uint64(1 << 20), 1.0, -1.0) * amp).astype(np.float32)


def shifted(ref, lag, seed, flip=0.2):
    """A member row for `ref`: the reference's sample i is the member's sample i + lag, with a fraction `flip` of the signs wrong; samples without a
    partner are random."""
    n = ref.size
    mem = random_signs(n, seed)
    if lag >= 0:
        mem[lag:] = ref[:n - lag]
    else:
        mem[:n + lag] = ref[-lag:]
    wrong = (np.random.PCG64(seed + 1).random_raw(n) % np.uint64(1000)) < np.uint64(int(1000 * flip))
    mem[wrong] = -mem[wrong]
    return mem


def planted(n, lag, seed, flip=0.2):
    """(reference row, member row) of n samples."""
    ref = random_signs(n, seed)
    return ref, shifted(ref, lag, seed + 7, flip)


# ---- the ladder's receivers: the WEAK signal of tones_model, stream s heard by receiver m with its own noise (seed 500 + s + 100 m)

FSD = TM.WEAK["fs"] / TM.WEAK["D"]
GUARD = 27                                                   # a bit of 300 baud at 8 kS/s, rounded


def weak_text(s):
    text = "".join(synth.make_sentence(f"W{s}", "%d,12:00:%02d,52.%04d,-0.1234,%d" % (k, k, 1000 + s * 7 + k, 100 * k)) for k in range(12))
    return text, {t.strip("$\n") for t in text.split("\n") if t}


def receiver_iq(sigma, s, m, late=0):
    """Receiver m of payload s: the input-rate IQ, `late` input samples late (zeros in front)."""
    n = TM.WEAK["n"] * TM.WEAK["calls"]
    iq = synth.fsk_iq(synth.rtty_bits(weak_text(s)[0], 8, 2, 3, 0), TM.WEAK["fs"], TM.WEAK["baud"], sigma=sigma, seed=500 + s + 100 * m, n_samples=n)
    return np.concatenate([np.zeros(late, np.complex64), iq[:n - late]]) if late else iq


def oracle_decimated(iq):
    """The oracle's last_decimated per call of the WEAK engine."""
    from oracle import pyoracle
    dec = pyoracle.Decoder("oracle", factor=TM.WEAK["D"], baud=TM.WEAK["baud"], bits=TM.WEAK["bits"], stops=TM.WEAK["stops"], lowpass_bw=TM.WEAK["bw"], with_fft=False)
    out = []
    for k in range(TM.WEAK["calls"]):
        dec(iq[k * TM.WEAK["n"]:(k + 1) * TM.WEAK["n"]], TM.WEAK["fs"])
        out.append(dec.array("last_decimated"))
    return out


@functools.lru_cache(maxsize=None)
def receiver_row(sigma, s, m, late=0):
    """The whole tone row of the receiver: oracle's decimated IQ through the host tone filters at +-250 Hz.  Computed once; read-only."""
    import habdec_amd
    t = habdec_amd.HostTones(FSD, TM.WEAK["baud"], TM.SHIFT / 2, -TM.SHIFT / 2)
    row = np.concatenate([t.push(d) for d in oracle_decimated(receiver_iq(sigma, s, m, late))])
    row.setflags(write=False)
    return row


@functools.lru_cache(maxsize=None)
def noise_row(seed, n=100000):
    """Complex Gaussian noise alone through the same tone filters."""
    import habdec_amd
    v = synth._noise(n, seed).astype(np.float32)
    t = habdec_amd.HostTones(FSD, TM.WEAK["baud"], TM.SHIFT / 2, -TM.SHIFT / 2)
    row = t.push(np.ascontiguousarray(v).view(np.complex64))
    row.setflags(write=False)
    return row


def clocked_sentences(hd, rows, repair=True):
    """[(pos, flips, text)] the host clocked decoder delivers from a row (or a list of rows pushed in turn)."""
    h = hd.HostClocked(FSD, TM.WEAK["baud"], TM.WEAK["bits"], TM.WEAK["stops"], **({} if repair else dict(repair_bits=0)))
    for r in (rows if isinstance(rows, list) else [rows]):
        h.push(r)
    return h.take_sentences(256)
