"""numpy model of the SSDV packet receiver (hd_ssdv_*), written from the definition in include/habdec_amd.h -- not from the C++.

The codeword of a trial is found by another method than the product's (which runs Berlekamp-Massey): Peterson-Gorenstein-Zierler.  With the erasure
locator G(x) and the modified syndromes T = (G S)[f ..], the error locator's coefficients solve a linear system, tried from the largest admissible
number of errors down; the error values solve a second linear system over the syndromes; and whatever comes out counts only if the corrected word has
32 zero syndromes and 2 e + f <= 32 -- the definition itself.  The CRC is zlib's.  The file also holds the packet maker, the gap rule and the
ladder's signal."""
import zlib

import numpy as np

POLY, NROOTS, FCR, PRIM = 0x187, 32, 112, 11
EXP = np.zeros(512, np.int64)
LOG = np.zeros(256, np.int64)
_v = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _v
    LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= POLY
EXP[510], EXP[511] = EXP[0], EXP[1]
ROOT = EXP[(PRIM * (FCR + np.arange(NROOTS))) % 255]            # alpha^(11 (112 + m))
LOCATOR = EXP[(PRIM * ((255 - np.arange(256)) % 255)) % 255]     # of byte j: beta^(255 - j), beta = alpha^11
XINV = EXP[(255 - LOG[LOCATOR]) % 255]
NOFEC, TYPE_NOFEC, CONF_MAX = 255, 0x67, 0xFFFFFF


def gmul(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a == 0) | (b == 0), 0, EXP[LOG[a] + LOG[b]])


def ginv(a):
    return EXP[255 - LOG[np.asarray(a, np.int64)]]


def gpow(a, k):
    a = np.asarray(a, np.int64)
    return np.where(a == 0, 0 if k else 1, EXP[(LOG[a] * k) % 255])


def alpha_order() -> int:
    v, k = 2, 1
    while v != 1:
        v = int(gmul(v, 2)); k += 1
    return k


def generator() -> list:
    """Coefficients of the product of (x + ROOT[m]), x^0 first."""
    g = [1]
    for m in range(NROOTS):
        g = [0] + g
        for k in range(len(g) - 1):
            g[k] ^= int(gmul(g[k + 1], ROOT[m]))
    return g


def encode(data223) -> bytes:
    """Parity = the remainder of data(x) x^32 by the generator, by long division."""
    g = generator()
    rem = list(bytes(data223)) + [0] * NROOTS
    for i in range(223):
        c = rem[i]
        if c:
            for k in range(1, NROOTS + 1):
                rem[i + k] ^= int(gmul(c, g[NROOTS - k]))
    return bytes(rem[223:])


def crc32(b) -> int:
    return zlib.crc32(bytes(b)) & 0xFFFFFFFF


def callsign_code(s: str) -> int:
    x = 0
    for ch in reversed(s.upper()[:6]):
        x = x * 40 + (ord(ch) - ord("A") + 14 if "A" <= ch <= "Z" else ord(ch) - ord("0") + 1 if "0" <= ch <= "9" else 0)
    return x


def callsign_text(code: int) -> str:
    out = ""
    while code:
        s = code % 40
        out += "-" if s == 0 or 11 <= s < 14 else chr(ord("0") + s - 1) if s < 11 else chr(ord("A") + s - 14)
        code //= 40
    return out


def make_packet(payload, type=0x66, callsign="", image_id=0, packet_id=0, width=0, height=0, flags=0, mcu_offset=0, mcu_index=0) -> bytes:
    payload = bytes(payload)
    assert len(payload) == 205
    body = bytes([type]) + callsign_code(callsign).to_bytes(4, "big") + bytes([image_id]) + packet_id.to_bytes(2, "big") + \
        bytes([width // 16, height // 16, flags, mcu_offset]) + mcu_index.to_bytes(2, "big") + payload
    body += crc32(body).to_bytes(4, "big")
    return b"\x55" + body + (bytes(32) if type == TYPE_NOFEC else encode(body))


def header(data: bytes) -> dict:
    return dict(type=data[1], callsign=callsign_text(int.from_bytes(data[2:6], "big")), image_id=data[6], packet_id=int.from_bytes(data[7:9], "big"),
                width=data[9] * 16, height=data[10] * 16, flags=data[11], mcu_offset=data[12], mcu_index=int.from_bytes(data[13:15], "big"))


def syndromes(words) -> np.ndarray:
    """words [N, 256] (column 0 is the sync byte): [N, 32], the polynomial r_1 x^254 + ... + r_255 at every root."""
    words = np.asarray(words, np.int64)
    s = np.zeros((words.shape[0], NROOTS), np.int64)
    for j in range(1, 256):
        s = gmul(s, ROOT[None, :]) ^ words[:, j, None]
    return s


def solve(A, b):
    """Gauss-Jordan over the field for a batch: A [N, e, e], b [N, e] -> x [N, e], regular [N]."""
    N, e, _ = A.shape
    M = np.concatenate([A, b[:, :, None]], axis=2).astype(np.int64)
    ok, idx = np.ones(N, bool), np.arange(N)
    for col in range(e):
        sub = M[:, col:, col] != 0
        ok &= sub.any(axis=1)
        piv = col + np.argmax(sub, axis=1)
        rc, rp = M[idx, col].copy(), M[idx, piv].copy()
        M[idx, col], M[idx, piv] = rp, rc
        p = M[:, col, col]
        M[:, col, :] = gmul(M[:, col, :], ginv(np.where(p == 0, 1, p))[:, None])
        fac = M[:, :, col].copy()
        fac[:, col] = 0
        M ^= gmul(fac[:, :, None], M[:, col, :][:, None, :])
    return M[:, :, e], ok


def _erasure_locator(era):
    """era [N, f] positions: G [N, f + 1], the product of (1 + LOCATOR[j] x)."""
    N, f = era.shape
    G = np.zeros((N, f + 1), np.int64)
    G[:, 0] = 1
    for i in range(f):
        G[:, 1:] ^= gmul(G[:, :-1], LOCATOR[era[:, i]][:, None])
    return G


def _polymul(a, b):
    """[N, p] times [N, q] -> [N, p + q - 1]"""
    out = np.zeros((a.shape[0], a.shape[1] + b.shape[1] - 1), np.int64)
    for i in range(a.shape[1]):
        out[:, i:i + b.shape[1]] ^= gmul(a[:, i, None], b)
    return out


def _key_system(T, e):
    """sum over k = 1 .. e of sigma_k T[n - k] = T[n] for n = e .. 2 e - 1"""
    A = np.stack([np.stack([T[:, i + e - k] for k in range(1, e + 1)], axis=1) for i in range(e)], axis=1)
    return A, T[:, e:2 * e]


def _root_mask(lam):
    """lam [N, d + 1] -> [N, 256] bool: byte j is a root position (column 0 never)"""
    v = np.zeros((lam.shape[0], 256), np.int64)
    for k in range(lam.shape[1] - 1, -1, -1):
        v = gmul(v, XINV[None, :]) ^ lam[:, k, None]
    m = v == 0
    m[:, 0] = False
    return m


def _finish(r, S, erased, f, lam, e):
    """The codeword behind the locator lam, by solving for the error values; None unless everything the definition asks holds."""
    at = np.nonzero(_root_mask(lam[None, :])[0])[0]
    if len(at) != f + e or not all(j in at for j in erased):
        return None
    w = r.copy()
    if len(at):
        X = LOCATOR[at]
        A = np.stack([gpow(X, FCR + m) for m in range(len(at))], axis=0)[None]
        y, ok = solve(A, S[None, :len(at)])
        if not ok[0]:
            return None
        w[at] ^= y[0]
    if syndromes(w[None, :]).any():
        return None
    diff = [j for j in range(1, 256) if w[j] != r[j]]
    errs, ch = sum(j not in erased for j in diff), sum(j in erased for j in diff)
    return (w, errs, ch) if 2 * errs + f <= NROOTS else None


def _trial_one(r, S, erased, f):
    G = _erasure_locator(np.asarray(erased, np.int64).reshape(1, f))
    T = _polymul(G, S[None, :])[:, f:NROOTS]
    top = (NROOTS - f) // 2 if T.any() else 0     # (all of T zero: every system with e > 0 is singular)
    for e in range(top, -1, -1):
        sigma = np.ones((1, 1), np.int64)
        if e:
            x, ok = solve(*_key_system(T, e))
            if not ok[0]:
                continue
            sigma = np.concatenate([sigma, x], axis=1)
        got = _finish(r, S, set(erased), f, _polymul(G, sigma)[0], e)
        if got:
            return got
    return None


def trial(R, S, era, f):
    """R [N, 256], S [N, 32], era [N, 24] (positions by ascending key): per candidate None or (w, errors, erasures_changed)."""
    N = R.shape[0]
    out = [None] * N
    if not N:
        return out
    e = (NROOTS - f) // 2
    G = _erasure_locator(era[:, :f])
    T = _polymul(G, S)[:, f:NROOTS]
    x, ok = solve(*_key_system(T, e))
    lam = _polymul(G, np.concatenate([np.ones((N, 1), np.int64), x], axis=1))
    # regular at the largest e: a codeword in reach has exactly e errors and its locator is this one -- no candidate unless it has f + e roots
    hopeless = ok & (_root_mask(lam).sum(axis=1) != f + e)
    for i in np.nonzero(~hopeless)[0]:
        out[i] = _trial_one(R[i], S[i], [int(j) for j in era[i, :f]], f)
    return out


def decode_stream(b, c=None):
    """The whole definition for one stream: (packets, counters).  packets: dicts with pos, trial, errors, erasures, erasures_changed, data and the header."""
    b = np.frombuffer(bytes(b), np.uint8).astype(np.int64)
    c = np.full(b.size, CONF_MAX, np.int64) if c is None else np.minimum(np.asarray(c, np.int64), CONF_MAX)
    cnt = dict(bytes=int(b.size), decided=max(0, b.size - 255), fillers=0, crc_bad=0, overlaps=0, packets=[0] * 5)
    if b.size < 256:
        return [], cnt
    R = np.lib.stride_tricks.sliding_window_view(b, 256)
    Cw = np.lib.stride_tricks.sliding_window_view(c, 256)
    N = R.shape[0]
    found = {}

    def crc_ok(w):
        return crc32(bytes(w[1:220].astype(np.uint8))) == int.from_bytes(bytes(w[220:224].astype(np.uint8)), "big")

    alive = []
    for i in range(N):
        if R[i, 0] == 0x55 and R[i, 1] == TYPE_NOFEC and crc_ok(R[i]):
            found[i] = (NOFEC, 0, 0, 0, R[i].copy())
        else:
            alive.append(i)
    alive = np.asarray(alive, np.int64)
    S = syndromes(R[alive])
    key = (Cw[alive, 1:] << 8) | np.arange(1, 256)[None, :]
    era = np.argsort(key, axis=1, kind="stable")[:, :24] + 1
    sel = np.arange(alive.size)
    for t in range(4):
        res = trial(R[alive[sel]], S[sel], era[sel], 8 * t)
        keep = []
        for k, got in zip(sel, res):
            if got and crc_ok(got[0]):
                found[int(alive[k])] = (t, got[1], 8 * t, got[2], got[0])
                continue
            cnt["crc_bad"] += bool(got)
            keep.append(k)
        sel = np.asarray(keep, np.int64)
    packets, last = [], None
    for i in sorted(found):
        if last is not None and i < last + 256:
            cnt["overlaps"] += 1
            continue
        last = i
        t, e, f, ch, w = found[i]
        data = b"\x55" + bytes(w[1:].astype(np.uint8))
        cnt["packets"][4 if t == NOFEC else t] += 1
        packets.append(dict(pos=i, trial=t, errors=e, erasures=f, erasures_changed=ch, data=data, **header(data)))
    return packets, cnt


def gap_rule(pos, ch, data, char_len, max_fill=7, prev=None):
    """Records -> (bytes, confidences, fillers, the last pos): the door hd_ssdv_push_records."""
    b, c, fillers = [], [], 0
    for p, x, d in zip(pos, ch, data):
        p = int(p)
        if char_len and prev is not None and p > prev:
            k = (p - prev + char_len // 2) // char_len
            if 2 <= k <= 1 + max_fill:
                b += [0] * (k - 1); c += [0] * (k - 1); fillers += k - 1
        prev = p
        b.append(int(x) & 0xFF)
        c.append(min(CONF_MAX, min(abs(int(v)) for v in d)))
    return bytes(b), np.asarray(c, np.int64), fillers, prev


def ladder_packets(seed: int, count: int = 6) -> list:
    """The ladder's packets: random payloads, one image."""
    rng = np.random.default_rng(1000 + seed)
    return [make_packet(rng.integers(0, 256, 205, dtype=np.uint8).tobytes(), callsign="HABAMD", image_id=seed, packet_id=k, width=320, height=240, mcu_index=5 * k)
            for k in range(count)]


def ladder_row(seed: int, sigma: float, fsd: float = 8000.0, baud: float = 300.0):
    """Discriminator output of the ladder's six back-to-back packets, 300 baud 8N2, and the packets."""
    import baud_probe_model as M
    pk = ladder_packets(seed)
    text = b"".join(pk).decode("latin-1")
    seconds = (len(text) * 11 + 12) / baud
    return M.fsk_demod(baud, 8, 2, fsd, sigma, seconds, text=text, seed=seed), pk


def case_table() -> dict:
    """The case table: name -> (bytes, confidences or None, expected or None).  expected: the (pos, trial, errors, erasures, erasures_changed) of every
    delivered packet, where the case's construction says them; None: whatever the model says."""
    rng = np.random.default_rng(77)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    P = make_packet(rnd(205), callsign="TEST01", image_id=3, packet_id=0x0102, width=320, height=240, flags=4, mcu_offset=7, mcu_index=0x0304)
    Q = make_packet(rnd(205), callsign="TEST01", image_id=3, packet_id=0x0103, width=320, height=240, mcu_index=0x0310)
    N = make_packet(rnd(205), type=TYPE_NOFEC, callsign="NOFEC", image_id=9)
    hi = np.full(256, CONF_MAX, np.int64)

    def hit(pkt, at):
        b = bytearray(pkt)
        for k, j in enumerate(at):
            b[j] ^= 1 + (k * 37) % 255
        return bytes(b)

    def spread(n, first=2, step=9):              # distinct positions in 1 .. 255 for n <= 28
        return [first + step * k for k in range(n)]

    def low(at):
        c = hi.copy()
        for k, j in enumerate(at):
            c[j] = 10 + k
        return c

    t = {}
    t["size255"] = (rnd(255), None, [])
    t["size256"] = (P, None, [(0, 0, 0, 0, 0)])
    for o in (0, 1, 63, 64, 255, 256, 257):
        t["offset%d" % o] = (rnd(o) + P + rnd(40), None, None)
    for n in (1, 15, 16):
        t["errors%d" % n] = (hit(P, spread(n)), hi, [(0, 0, n, 0, 0)])
    t["errors17_equal"] = (hit(P, spread(17)), hi, [])
    t["errors17_low"] = (hit(P, spread(17)), low(spread(17)), [(0, 1, 9, 8, 8)])
    l24, l16, l8 = spread(24), spread(16), spread(8)
    t["low24_plus4"] = (hit(P, l24 + [240, 241, 250, 255]), low(l24), [(0, 3, 4, 24, 24)])
    t["low24_plus5"] = (hit(P, l24 + [240, 241, 250, 255, 1]), low(l24), [])
    t["low16_plus8"] = (hit(P, l16 + [200, 201, 210, 220, 230, 240, 250, 255]), low(l16), [(0, 2, 8, 16, 16)])
    # low confidence on bytes that are right costs nothing: trial 0 never looks at it
    t["low24_right"] = (hit(P, [230, 231, 232, 233]), low(l24), [(0, 0, 4, 0, 0)])
    # eight erasures of which six were wrong, eleven errors beside them: 17 wrong bytes fail trial 0, 2 * 11 + 8 = 30 passes trial 1, and the two erased
    # bytes that were right stay as they are
    t["low8_six_wrong"] = (hit(P, l8[:6] + spread(11, 100, 13)), low(l8), [(0, 1, 11, 8, 6)])
    for j in (1, 223, 224, 255):
        t["error_at%d" % j] = (hit(P, [j]), None, [(0, 0, 1, 0, 0)])
    t["error_at_all4"] = (hit(P, [1, 223, 224, 255]), None, [(0, 0, 4, 0, 0)])
    t["sync_wrong"] = (rnd(5) + b"\x00" + P[1:] + rnd(5), None, [(5, 0, 0, 0, 0)])
    t["nofec_clean"] = (rnd(3) + N + rnd(3), None, [(3, NOFEC, 0, 0, 0)])
    t["nofec_one_wrong"] = (rnd(3) + hit(N, [100]) + rnd(3), None, [])
    t["zeros"] = (bytes(600), None, [])
    t["two_packets"] = (rnd(7) + P + Q + rnd(7), None, [(7, 0, 0, 0, 0), (263, 0, 0, 0, 0)])
    t["same_twice"] = (P + P, None, [(0, 0, 0, 0, 0), (256, 0, 0, 0, 0)])
    t["noise"] = (rnd(4096), None, [])
    out = {}
    for k, (b, c, want) in t.items():
        if c is not None and len(c) != len(b):
            c = np.concatenate([c, np.full(len(b) - len(c), CONF_MAX, np.int64)])
        out[k] = (b, c, want)
    return out
