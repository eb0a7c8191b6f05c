"""A numpy model of the clocked decoder, written from its definition (include/habdec_amd.h, "clocked soft-decision decoder") and not from the C++: what
hd_host_clocked_records and hd_clocked_records are held to record for record.  Also the streams and the noise ladder the decoder's tests share.

The model works on a whole stream at once: the definition speaks of absolute sample indices only, so how a stream is cut into pushes cannot matter."""
import math

import numpy as np

import baud_probe_model as M
from habdec_amd import synth

MAX_SPB = 2048


def quantise(v, invert=False):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        q = np.trunc(np.clip(v, np.float32(-4.0), np.float32(4.0)).astype(np.float64) * 1024.0)
    q = np.where(np.isnan(v), 0.0, q).astype(np.int64)
    return -q if invert else q


def clock(fsd, baud, nbits, nstops):
    F = int(math.floor(fsd / baud * 65536 + 0.5))
    full, h, K = (F + 32768) >> 16, max(2, (F + 65536) >> 17), 1 + nbits + nstops
    return F, full, h, K, h + ((K * F + 32768) >> 16)


def decode(d, fsd, baud, nbits, nstops, invert=False):
    """(records, counters) after the samples d since a reset.  A record: (pos, ch, data[8], start, stop, stop2)."""
    F, full, h, K, look = clock(fsd, baud, nbits, nstops)
    q = quantise(d, invert)
    n = q.size
    P = np.concatenate([[0], np.cumsum(q)])                # S(a, b) = P[b] - P[a]
    S = lambda a, b: int(P[b] - P[a])
    B = lambda x, k: x + ((k * F + 32768) >> 16)
    last = n - look                                         # the last position that is decided
    records, rejects, p = [], 0, h
    if last >= h:
        i = np.arange(h, last + 1)
        cand = i[((P[i] - P[i - h]) > 0) & ((P[i + h] - P[i]) < 0)]
    else:
        cand = np.zeros(0, np.int64)
    while True:
        j = np.searchsorted(cand, p)
        if j == cand.size:
            p = max(p, last + 1)
            break
        p = int(cand[j])
        xs = np.arange(p, p + h + 1)
        cost = (P[xs + full] - P[xs]) - (P[xs] - P[xs - h])
        x = int(xs[np.argmin(cost)])                        # argmin: the first of equal minima
        start, stop = S(B(x, 0), B(x, 1)), S(B(x, 1 + nbits), B(x, 2 + nbits))
        if start < 0 and stop > 0:
            data = [S(B(x, 1 + k), B(x, 2 + k)) for k in range(nbits)] + [0] * (8 - nbits)
            ch = sum((data[k] > 0) << k for k in range(nbits))
            stop2 = S(B(x, 2 + nbits), B(x, 3 + nbits)) if nstops == 2 else 0
            records.append((x, ch, data, start, stop, stop2))
            p = x + (((2 * (1 + nbits) + 1) * F + 65536) >> 17)
        else:
            rejects += 1
            p += 1
    return records, dict(samples=n, cursor=p, characters=len(records), rejects=rejects)


def as_tuples(rec_array):
    """An array of capi.CLOCKED_RECORD_DTYPE as the model's tuples."""
    return [(int(r["pos"]), int(r["ch"]), [int(v) for v in r["data"]], int(r["start"]), int(r["stop"]), int(r["stop2"])) for r in rec_array]


def assert_same(records, counters, want_records, want_counters, what=""):
    assert len(records) == len(want_records), (what, len(records), len(want_records))
    for i, (a, b) in enumerate(zip(records, want_records)):
        assert a == b, (what, i, a, b)
    for k, v in want_counters.items():
        assert counters[k] == v, (what, k, counters[k], v)


# ---- the streams of the parity tests: (name, row, fsd, baud, nbits, nstops)

def square_wave(n=3000):
    d = np.ones(n, np.float32)
    d[1::2] = -1.0
    return d


def streams():
    out = []
    for c in M.CASES:
        name, baud, nbits, nstops, fsd, sigma, seconds, text = c
        if text is None and fsd / baud <= MAX_SPB:
            out.append((name, M.case_signal(c), fsd, baud, nbits, nstops))
    out.append(("specials", M.specials_row(), 32000.0, 300.0, 8, 2))
    out.append(("zeros", np.zeros(5000, np.float32), 32000.0, 300.0, 8, 2))
    out.append(("positive", np.full(5000, 0.5, np.float32), 32000.0, 300.0, 8, 2))
    out.append(("square", square_wave(), 2400.0, 400.0, 7, 1))      # h = 3: the sum of three alternating samples changes sign at every second position
    out.append(("spb4", M.fsk_demod(600.0, 8, 2, 2400.0, 0.05, 2.0), 2400.0, 600.0, 8, 2))
    out.append(("spb130", M.fsk_demod(300.0, 8, 2, 39062.5, 0.1, 1.5), 39062.5, 300.0, 8, 2))
    out.append(("spb52", M.fsk_demod(45.45, 7, 1, 2400.0, 0.2, 6.0), 2400.0, 45.45, 7, 1))
    out.append(("spb2048", M.fsk_demod(15.625, 8, 2, 32000.0, 0.05, 8.0, text="$$A,1*ABCD\n"), 32000.0, 15.625, 8, 2))
    return out


def sent_sentences(seconds, baud, nbits, nstops):
    """The sentences of M.telemetry_text, as callsign,data*CRC."""
    return {s.strip("$\n") for s in M.telemetry_text(seconds, baud, nbits, nstops).split("\n") if s}


# ---- the noise ladder (tests/test_clocked_ladder.py, NOTES.md): fsd 8000, fixed seeds, 13 sentences or more per rung
LADDER = {
    "300_8n2": dict(baud=300.0, nbits=8, nstops=2, seconds=34.0, sigmas=(0.10, 0.14, 0.16, 0.18, 0.20, 0.22, 0.24, 0.26, 0.28)),
    "50_7n2": dict(baud=50.0, nbits=7, nstops=2, seconds=150.0, sigmas=(0.20, 0.25, 0.30, 0.35, 0.40, 0.45, 0.50)),
}
LADDER_FSD = 8000.0


def ladder_signal(modem, sigma):
    m = LADDER[modem]
    return M.fsk_demod(m["baud"], m["nbits"], m["nstops"], LADDER_FSD, sigma, m["seconds"], seed=3)


def oracle_sentences(row, fsd, baud, nbits, nstops, chunk=4096):
    """What the oracle's symbol extractor, framer and sentence scan decode from a row of discriminator output: [callsign,data*CRC] with a matching CRC."""
    from oracle import pyoracle
    st = pyoracle.Stages("oracle")
    sx, rt = st.symex(fsd, baud), st.rtty(nbits, float(nstops))
    stream, out = "", []
    for at in range(0, row.size, chunk):
        sx.push(row[at:at + chunk])
        bits = sx.run()
        if not bits.size:
            continue
        rt.push(bits)
        raw = rt.run()
        stream += "".join(chr(c) for c in raw if 0x20 <= c <= 0x7e or c == 10)
        while len(stream) > 20:
            m = st.extract_sentence(stream)
            if m is None:
                break
            stream = m["stream"]
            if st.crc16(m["callsign"] + "," + m["data"]) == m["crc"]:
                out.append(m["callsign"] + "," + m["data"] + "*" + m["crc"])
        if len(stream) > 1000:
            stream = stream[stream.rfind("$"):] if "$" in stream else ""
    return out
