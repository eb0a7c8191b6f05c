"""A numpy model of the Horus Binary 4FSK modem, written from its definition (include/habdec_amd.h, "Horus Binary 4FSK") and not from the C++: what
hd_host_fsk4_* and the records of hd_fsk4_* are held to byte for byte.  Also the signals the modem's tests share.

The model works on a whole stream at once: the definition speaks of absolute sample and slot indices only, so how a stream is cut into pushes cannot
matter.  Its Golay decoder goes another way than the C++: it looks for the nearest of the 4096 codewords, no syndrome table."""
import math

import numpy as np

import tones_model as TM

V1 = dict(P=22, uw=(0x24, 0x24), mul=337, seed=0x4A80, poly=0xC75)
V2 = dict(P=32, uw=(0x24, 0x24), mul=503, seed=0x4A80, poly=0xC75)
PAD_CONFIDENCE = 1 << 24
SETTLE = 16                    # slots behind a group's first candidate in which its members contest the delivery


def codewords(P):
    return -(-8 * P // 12)


def body_bytes(P):
    return P + -(-11 * codewords(P) // 8)


def n_symbols(P):
    return 4 * (2 + body_bytes(P))


def poly_rem(w, poly):
    """Remainder of the polynomial w by the generator (degree 11)."""
    for b in range(max(w.bit_length() - 1, 10), 10, -1):
        if (w >> b) & 1:
            w ^= poly << (b - 11)
    return w


def crc16(data):
    crc = 0xFFFF
    for byte in bytes(data):
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def with_crc(data):
    c = crc16(data)
    return bytes(data) + bytes([c & 0xFF, c >> 8])


def scrambler(seed, n):
    out, state = np.zeros(n, np.uint8), seed
    for i in range(n):
        o = ((state >> 1) ^ state) & 1
        state = (state >> 1) | (o << 14)
        out[i] = o
    return out


def payload_bits(payload):
    """Most significant bit first."""
    return np.unpackbits(np.frombuffer(bytes(payload), np.uint8))


def encode(payload, fr, flips=()):
    """payload (P bytes, CRC included) -> the frame's 2 + B bytes.  flips: (k, b) pairs, bit b of codeword k (0 its most significant data bit, 22 its last
    parity bit) is sent wrong -- channel errors, put in before the interleaver."""
    P, K, B = fr["P"], codewords(fr["P"]), body_bytes(fr["P"])
    assert len(payload) == P
    bits = np.concatenate([payload_bits(payload), np.zeros(12 * K - 8 * P, np.uint8)])
    parity = []
    for k in range(K):
        data = int("".join(map(str, bits[12 * k:12 * k + 12])), 2)
        r = poly_rem(data << 11, fr["poly"])
        parity += [(r >> (10 - b)) & 1 for b in range(11)]
    parity += [0] * (8 * (B - P) - len(parity))
    bits = bits[:8 * P].copy()
    for k, b in flips:
        if b < 12:
            bits[12 * k + b] ^= 1                                # (a zero-padded position is not sent: flipping one is an IndexError)
        else:
            parity[11 * k + b - 12] ^= 1
    body = np.concatenate([np.packbits(bits), np.packbits(np.array(parity, np.uint8))])
    lsb = np.unpackbits(body, bitorder="little")                 # bit i <-> byte i / 8, bit i % 8
    mixed = np.zeros_like(lsb)
    mixed[(fr["mul"] * np.arange(8 * B)) % (8 * B)] = lsb
    mixed ^= scrambler(fr["seed"], 8 * B)
    return bytes(fr["uw"]) + np.packbits(mixed, bitorder="little").tobytes()


def symbols(frame_bytes):
    b = np.unpackbits(np.frombuffer(bytes(frame_bytes), np.uint8))
    return (2 * b[0::2] + b[1::2]).astype(np.int64)


# ---- the tone bank and the slots

def modem(fsd, baud, f0, spacing, window_q8=256):
    F = int(math.floor(fsd / baud * 65536 + 0.5))
    W = max(1, (F * window_q8 + (1 << 23)) >> 24)
    step = [int(np.rint((f0 + t * spacing) / fsd * 2.0 ** 32)) & 0xFFFFFFFF for t in range(4)]       # np.rint: ties to even
    return dict(F=F, W=W, step=step)


def slot_end(F, g):
    return (((g + 8) * F) >> 19) - 1


def slot_records(iq, fsd, baud, f0, spacing, window_q8=256):
    """uint32 [G, 4]: the record of every slot whose last sample is in iq (the samples since a reset)."""
    m = modem(fsd, baud, f0, spacing, window_q8)
    iq = np.ascontiguousarray(iq, np.complex64)
    ends = []
    g = 0
    while slot_end(m["F"], g) < iq.size:
        ends.append(slot_end(m["F"], g))
        g += 1
    ends = np.array(ends, np.int64)
    assert np.all(np.diff(ends) > 0)
    q_re, q_im = TM.quantise(iq.real), TM.quantise(iq.imag)
    i = np.arange(iq.size, dtype=np.uint64)
    out = np.zeros((ends.size, 4), np.uint32)
    for t, step in enumerate(m["step"]):
        theta = (i * np.uint64(step)) & np.uint64(0xFFFFFFFF)
        a = (theta >> np.uint64(22)).astype(np.int64)
        c, s = TM.C_TABLE[a], TM.C_TABLE[(a + 768) & 1023]
        r_re, r_im = (q_re * c + q_im * s) >> 15, (q_im * c - q_re * s) >> 15            # arithmetic shifts: floor
        s_re, s_im = TM.window_sum(r_re, m["W"])[ends], TM.window_sum(r_im, m["W"])[ends]
        assert ends.size == 0 or max(np.abs(s_re).max(), np.abs(s_im).max()) < 1 << 23
        out[:, t] = TM.isqrt(s_re * s_re + s_im * s_im)
    return out


# ---- the frame search

_CODEBOOK = {}


def codebook(poly):
    if poly not in _CODEBOOK:
        _CODEBOOK[poly] = np.array([d << 11 | poly_rem(d << 11, poly) for d in range(4096)], np.int64)
        w = _CODEBOOK[poly]
        assert poly_rem((1 << 23) | 1, poly) == 0                                            # x^23 + 1 is a multiple of the generator
        assert min(bin(int(x)).count("1") for x in w[1:]) == 7                               # minimum weight 7
    return _CODEBOOK[poly]


def popcount(x):
    x = np.asarray(x, np.int64)
    n = np.zeros(x.shape, np.int64)
    for b in range(23):
        n += (x >> b) & 1
    return n


def nearest_codeword(w, poly):
    book = codebook(poly)
    d = popcount(book ^ w)
    k = int(np.argmin(d))
    assert d[k] <= 3 and np.count_nonzero(d <= 3) == 1                                       # perfect: exactly one within distance 3
    return int(book[k])


def soft_golay(soft, chase_bits, poly):
    """soft: 23 values, position 0 the most significant bit.  -> (codeword, corrected bits)"""
    conf = [abs(int(v)) for v in soft]
    h = 0
    for b in range(23):
        h |= (1 if soft[b] > 0 else 0) << (22 - b)
    order = sorted(range(23), key=lambda b: (conf[b], b))[:chase_bits]                      # ties: the position nearer the most significant bit
    best = None
    for pn in range(1 << chase_bits):
        w = h
        for c in range(chase_bits):
            if (pn >> c) & 1:
                w ^= 1 << (22 - order[c])
        cw = nearest_codeword(w, poly)
        cost = sum(conf[b] for b in range(23) if ((cw ^ h) >> (22 - b)) & 1)
        if best is None or cost < best[0]:
            best = (cost, cw)
    return best[1], bin(best[1] ^ h).count("1")


def decode_candidate(E, fr, uw_max_errors=2, chase_bits=4):
    """E: int [nsym, 4], the records of the candidate's symbols.  None: the gate refused it; else the candidate record as a dict."""
    P, K, B = fr["P"], codewords(fr["P"]), body_bytes(fr["P"])
    E = np.asarray(E, np.int64)
    assert E.shape == (n_symbols(P), 4)
    hard = np.argmax(E, axis=1)                                                               # the lowest t on ties
    uw = symbols(bytes(fr["uw"]))
    uw_errors = int(sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(hard[:8], uw)))
    if uw_errors > uw_max_errors:
        return None
    hi = np.maximum(E[:, 2], E[:, 3]) - np.maximum(E[:, 0], E[:, 1])
    lo = np.maximum(E[:, 1], E[:, 3]) - np.maximum(E[:, 0], E[:, 2])
    air = np.stack([hi, lo], axis=1).reshape(-1)[16:]                                        # the body's on-air soft bits
    r = np.arange(8 * B)
    mixed = np.zeros(8 * B, np.int64)
    mixed[8 * (r // 8) + 7 - r % 8] = air                                                    # on-air bit r is byte r / 8, bit 7 - r % 8
    mixed = np.where(scrambler(fr["seed"], 8 * B) == 1, -mixed, mixed)
    body = mixed[(fr["mul"] * np.arange(8 * B)) % (8 * B)]                                   # bit i came from j = mul i mod 8 B
    msb = body.reshape(B, 8)[:, ::-1].reshape(-1)                                            # bytes most significant bit first
    data_soft = np.concatenate([msb[:8 * P], np.full(12 * K - 8 * P, -PAD_CONFIDENCE, np.int64)])
    parity_soft = msb[8 * P:]
    bits, corrected = [], 0
    for k in range(K):
        cw, n = soft_golay(list(data_soft[12 * k:12 * k + 12]) + list(parity_soft[11 * k:11 * k + 11]), chase_bits, fr["poly"])
        corrected += n
        bits += [(cw >> (22 - b)) & 1 for b in range(12)]
    payload = np.packbits(np.array(bits[:8 * P], np.uint8)).tobytes()
    return dict(metric=int(E.max(axis=1).sum()), crc_ok=int(crc16(payload[:-2]) == (payload[-2] | payload[-1] << 8)), corrected=corrected,
                uw_errors=uw_errors, payload=payload)


def candidates(slots, fr, uw_max_errors=2, chase_bits=4):
    """Every decided candidate behind the gate, in slot order, and how many are decided, for the slot records slots[0 .. G - 1]."""
    nsym = n_symbols(fr["P"])
    G = slots.shape[0]
    decided = max(0, G - 8 * (nsym - 1))
    hard = np.argmax(slots, axis=1)
    uw = symbols(bytes(fr["uw"]))
    err = np.zeros(decided, np.int64)
    for m in range(8):
        x = hard[8 * m:8 * m + decided] ^ uw[m]
        err += (x & 1) + (x >> 1)
    out = []
    for g in np.flatnonzero(err <= uw_max_errors):
        c = decode_candidate(slots[g:g + 8 * nsym:8], fr, uw_max_errors, chase_bits)
        c["slot"] = int(g)
        out.append(c)
    return out, decided


def select(cands, fr, F, decided, max_corrected=None):
    """The frames delivered once `decided` candidates are decided, and the counters (gate_passes, crc_failures, refused, frames)."""
    nsym, K = n_symbols(fr["P"]), codewords(fr["P"])
    limit = 2 * K if max_corrected is None or max_corrected < 0 else max_corrected
    good = [c for c in cands if c["crc_ok"] and c["corrected"] <= limit]
    frames, overlaps, k = [], 0, 0
    while k < len(good):
        first = good[k]["slot"]
        if decided < first + SETTLE:
            break                                                                             # the contest is still open
        grp = [c for c in good[k:] if c["slot"] < first + SETTLE]
        b = min(grp, key=lambda c: (c["corrected"], -c["metric"], c["slot"]))
        frames.append(dict(slot=b["slot"], start_sample=(b["slot"] * F) >> 19, metric=b["metric"], payload_bytes=fr["P"], corrected=b["corrected"],
                           phase=b["slot"] % 8, uw_errors=b["uw_errors"], payload=b["payload"]))
        k += len(grp)
        while k < len(good) and good[k]["slot"] < b["slot"] + 8 * (nsym - 1):
            overlaps += 1
            k += 1
    counters = dict(candidates=decided, gate_passes=len(cands), crc_failures=sum(1 for c in cands if not c["crc_ok"]),
                    refused=sum(1 for c in cands if c["crc_ok"] and c["corrected"] > limit), overlaps=overlaps, frames=len(frames))
    return frames, counters


def receive(iq, fsd, baud, f0, spacing, fr, window_q8=256, uw_max_errors=2, chase_bits=4, max_corrected=None):
    """The whole modem over the samples since a reset: (slot records, candidates behind the gate, frames, counters)."""
    slots = slot_records(iq, fsd, baud, f0, spacing, window_q8)
    cands, decided = candidates(slots, fr, uw_max_errors, chase_bits)
    frames, counters = select(cands, fr, modem(fsd, baud, f0, spacing, window_q8)["F"], decided, max_corrected)
    counters.update(samples=int(np.asarray(iq).size), slots=int(slots.shape[0]))
    return slots, cands, frames, counters


def clean_records(syms, level=1000):
    """The slot records of perfectly timed clean symbols, one per symbol: `level` at the symbol's tone, 0 elsewhere."""
    E = np.zeros((len(syms), 4), np.int64)
    E[np.arange(len(syms)), np.asarray(syms)] = level
    return E


# ---- signals

def fsk4_iq(syms, fs, baud, f0, spacing, sigma=0.0, seed=0, start=0.0, n_samples=None, alt=None):
    """The same signal as habdec_amd.fsk4.fsk4_iq, restated: continuous-phase tones, symbol k from sample start + k fs / baud on.  alt: {k: (v, w)},
    symbol k is sent as (1 - w) of its own tone and w of tone v -- a symbol the receiver is unsure of."""
    syms = np.asarray(syms, np.int64)
    spb = fs / baud
    n = int(np.ceil(start + syms.size * spb)) if n_samples is None else int(n_samples)
    i = np.arange(n, dtype=np.float64)
    k = np.floor((i - start) / spb).astype(np.int64)
    on = (k >= 0) & (k < syms.size)
    f = np.where(on, f0 + spacing * syms[np.clip(k, 0, syms.size - 1)], 0.0) if syms.size else np.zeros(n)
    iq = np.where(on, np.exp(2j * np.pi * np.cumsum(f) / fs), 0.0)
    for kk, (v, w) in (alt or {}).items():
        sel = k == kk
        iq[sel] = (1.0 - w) * iq[sel] + w * np.exp(2j * np.pi * (f0 + spacing * v) * i[sel] / fs)
    if sigma:
        rng = np.random.default_rng(seed)
        iq = iq + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return iq.astype(np.complex64)


def make_payload(fr, k=0):
    """A payload of the frame's length with its CRC: a counter, then seeded bytes."""
    rng = np.random.default_rng(1000 + k)
    return with_crc(bytes([k & 0xFF]) + rng.integers(0, 256, fr["P"] - 3, dtype=np.uint8).tobytes())


# ---- the sensitivity ladder (tests/golden/fsk4_ladder.json, made by tools/gen_golden_fsk4.py)

def ladder_signal(g, rung):
    """(iq, the payloads sent): g["frames"] frames of the ladder's preset, g["gap"] samples of noise between them, noise of the rung's sigma and seed."""
    fr = V1 if g["preset"] == 1 else V2
    spb = g["fsd"] / g["baud"]
    period = n_symbols(fr["P"]) * spb + g["gap"]
    n = int(g["frames"] * period + 2 * g["gap"])
    payloads = [make_payload(fr, 100 + k) for k in range(g["frames"])]
    iq = np.zeros(n, np.complex128)
    for k, p in enumerate(payloads):
        iq += fsk4_iq(symbols(encode(p, fr)), g["fsd"], g["baud"], g["f0"], g["spacing"], start=g["gap"] + k * period + 0.37 * k, n_samples=n)
    rng = np.random.default_rng(rung["seed"])
    return (iq + rung["sigma"] * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64), payloads
