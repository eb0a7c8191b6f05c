"""numpy model of the AFSK / AX.25 modem (hd_afsk_*), written from the definition in include/habdec_amd.h and not from the C++.

One stream: push(row) appends samples and scans; slots, candidates, frames and counters are held as the definition names them.  Where the C++ streams
(a CRC register behind a seven-bit delay, an address check byte by byte) the model collects the kept bits, cuts the flag off, packs bytes and checks
them whole."""
from itertools import combinations

import numpy as np

RING, MAX_FRAME, MIN_FRAME, MAX_SPB = 65536, 332, 17, 2048
OPEN, ABORT, UNSHAPED, FCS_FAILED, REFUSED, PLAIN, REPAIRED = range(7)
C = np.rint(32767.0 * np.cos(2 * np.pi * np.arange(1024) / 1024.0)).astype(np.int64)


def crc16(data: bytes) -> int:
    crc = 0xFFFF
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return crc ^ 0xFFFF


def walk_bits(max_frame_bytes: int) -> int:
    return -(-8 * max_frame_bytes * 6 // 5) + 8


def quantise(v) -> np.ndarray:
    v = np.asarray(v, np.float32)
    finite = np.where(np.isnan(v), np.float32(0), v)
    return (np.clip(finite, np.float32(-4), np.float32(4)) * np.float32(1024)).astype(np.int64)      # (astype truncates toward zero)


def isqrt(x: np.ndarray) -> np.ndarray:
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r -= r * r > x
    r += (r + 1) * (r + 1) <= x
    return r


def address_ok(data: bytes) -> bool:
    """data: the frame without its FCS."""
    ends = [i for i, b in enumerate(data) if b & 1]
    if not ends:
        return False
    end = ends[0]
    if (end + 1) % 7 or not 2 <= (end + 1) // 7 <= 10:
        return False
    for i in range(end + 1):
        if i % 7 < 6:
            c = data[i] >> 1
            if data[i] & 1 or not (65 <= c <= 90 or 48 <= c <= 57 or c == 32):
                return False
    return True


def walk(levels, limit):
    """levels[r], r = 0 the flag's last bit.  -> (kind, at, kept bits in front of the closing flag or None)."""
    ones, kept = 0, []
    levels = [int(v) for v in levels[:limit + 1]]
    for r in range(1, limit + 1):
        bit = 1 if levels[r] == levels[r - 1] else 0
        if bit:
            ones += 1
            if ones == 7:
                return ABORT, r, None
            kept.append(1)
        else:
            was, ones = ones, 0
            if was == 5:
                continue
            if was == 6:
                return "close", r, kept[:-7] if len(kept) >= 7 else []
            kept.append(0)
    return OPEN, limit, None


def pack(bits) -> bytes:
    return bytes(sum(b << k for k, b in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))


class AfskModel:
    def __init__(self, fsd, baud=None, mark=1200.0, space=2200.0, max_push=4096, max_frame_bytes=MAX_FRAME, repair_bits=8, repair_flips=2, require_addr=1):
        self.fsd, self.max_frame_bytes, self.require_addr = float(fsd), max_frame_bytes, require_addr
        self.L = walk_bits(max_frame_bytes)
        self.patterns = [()]
        if repair_bits and repair_flips:
            for size in range(1, min(repair_flips, repair_bits) + 1):
                self.patterns += list(combinations(range(repair_bits), size))
        assert len(self.patterns) <= 64 and 8 * self.L + 72 + max_push <= RING
        self.repair_bits = repair_bits if len(self.patterns) > 1 else 0
        self.F = 0
        self.waiting = []
        if baud is not None:
            self.set_modem(baud, mark, space)

    def set_modem(self, baud, mark, space):
        spb = self.fsd / baud
        if not 8 <= spb <= MAX_SPB:
            raise ValueError("unsupported")
        if not (0 < mark < self.fsd / 2 and 0 < space < self.fsd / 2 and mark != space):
            raise ValueError("invalid")
        self.F = int(np.floor(spb * 65536.0 + 0.5))
        self.W = (self.F + 32768) >> 16
        self.phi = [int(np.rint(f / self.fsd * 2.0 ** 32)) & 0xFFFFFFFF for f in (mark, space)]
        self.reset()

    def reset(self):
        self.n = self.g = 0
        self.P = np.zeros((4, 1), np.int64)          # true running sums, P[:, j] after j samples
        self.d, self.d0 = np.zeros(0, np.int64), 0     # slot records from slot d0 on
        self.decided = 0
        self.counters = dict(flags=0, unshaped=0, fcs_failures=0, frames_plain=0, frames_repaired=0, refused=0, overlaps=0)
        self.open, self.group_first, self.blocked_until, self.best = False, 0, 0, None
        self.candidates = []

    def stats(self) -> dict:
        return dict(samples=self.n, slots=self.g, F=self.F, W=self.W, step=list(self.phi), **self.counters)

    def take_frames(self) -> list:
        out, self.waiting = self.waiting, []
        return out

    # ---- samples -> slots
    def push(self, row):
        if not self.F:
            return
        q = quantise(row)
        i = np.arange(self.n, self.n + q.size, dtype=np.uint64)
        r = np.zeros((4, q.size), np.int64)
        for t in range(2):
            a = (((i * np.uint64(self.phi[t])) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)
            r[2 * t] = (q * C[a]) >> 15
            r[2 * t + 1] = (-q * C[(a + 768) & 1023]) >> 15
        P = np.concatenate([self.P, self.P[:, -1:] + np.cumsum(r, axis=1)], axis=1)      # P[:, j]: the sums after p0 + j samples
        p0 = self.n - (self.P.shape[1] - 1)
        self.n += q.size
        # slot g exists once its last sample end(g) = ((g + 8) F >> 19) - 1 is pushed: (g + 8) F < (n + 1) 2^19
        g1 = max(-(-((self.n + 1) << 19) // self.F) - 8, self.g)
        g = np.arange(self.g, g1, dtype=np.int64)
        end = (((g + 8) * self.F) >> 19) - 1
        lo = np.maximum(end + 1 - self.W, 0)
        w = P[:, end + 1 - p0] - P[:, lo - p0]
        A = [isqrt(w[2 * t] ** 2 + w[2 * t + 1] ** 2) for t in range(2)]
        self.d = np.concatenate([self.d, A[0] - A[1]])
        self.g = g1
        self.P = P[:, -(self.W + 1):]                 # (the model keeps what a later window reads, and below the slots a later scan reads)
        self.scan()
        keep = max(self.decided - 64, self.d0)
        self.d, self.d0 = self.d[keep - self.d0:], keep

    def slot(self, g):
        """d of slot g (an index or an array of them)."""
        return self.d[g - self.d0]

    # ---- slots -> candidates
    def scan(self):
        n = self.g - 8 * self.L - self.decided
        if n <= 0:
            return
        first = max(self.decided, 64)
        g = np.arange(first, self.decided + n, dtype=np.int64)
        if g.size:
            lv = np.stack([self.slot(g - 8 * (8 - j)) > 0 for j in range(9)])
            nrzi = lv[1:] == lv[:-1]
            flag = ~nrzi[0] & nrzi[1:7].all(axis=0) & ~nrzi[7]
            for slot in g[flag]:
                self.accept(self.decode(int(slot)))
        self.decided += n
        if self.open and self.decided >= self.group_first + 8:
            self.deliver()

    def frame_of(self, levels, limit):
        kind, at, bits = walk(levels, limit)
        if kind != "close":
            return kind, at, None
        nb = len(bits) // 8
        shaped = len(bits) % 8 == 0 and MIN_FRAME <= nb <= self.max_frame_bytes
        return "close", at, pack(bits) if shaped else None

    def decode(self, slot) -> dict:
        d = self.slot(slot + 8 * np.arange(self.L + 1))
        levels, conf = (d > 0).astype(np.int64), np.abs(d)
        o = dict(slot=slot, close_slot=0, metric=0, result=OPEN, bits=0, len=0, flips=0, addr_ok=0, fcs=0, data=b"")
        kind, at, frame = self.frame_of(levels, self.L)
        o["bits"], o["metric"] = at, int(conf[1:at + 1].sum())
        if kind != "close":
            o["result"] = kind
            return o
        o["close_slot"] = slot + 8 * at
        if frame is None:
            o["result"] = UNSHAPED
            return o

        def fill(frame, flips, result):
            o.update(result=result, len=len(frame), flips=flips, data=frame, fcs=frame[-2] | frame[-1] << 8, addr_ok=int(address_ok(frame[:-2])))
            return o

        good = lambda f: crc16(f[:-2]) == (f[-2] | f[-1] << 8)
        if good(frame):
            return fill(frame, 0, PLAIN if address_ok(frame[:-2]) or not self.require_addr else REFUSED)
        # the repair_bits least confident levels of the bits 1 .. at - 8, ties to the earlier bit
        order = sorted(range(1, at - 7), key=lambda r: (int(conf[r]), r))[:self.repair_bits]
        refused = False
        for pat in self.patterns[1:]:
            if any(p >= len(order) for p in pat):
                continue
            lv = levels.copy()
            for p in pat:
                lv[order[p]] ^= 1
            k2, at2, f2 = self.frame_of(lv, at)
            if k2 != "close" or at2 != at or f2 is None or not good(f2):
                continue
            if not address_ok(f2[:-2]):
                refused = True
                continue
            return fill(f2, len(pat), REPAIRED)
        return fill(frame, 0, REFUSED if refused else FCS_FAILED)

    # ---- candidates -> frames
    def accept(self, o):
        c = self.counters
        c["flags"] += 1
        self.candidates.append(o)
        if o["result"] in (OPEN, ABORT, UNSHAPED):
            c["unshaped"] += 1
        elif o["result"] == FCS_FAILED:
            c["fcs_failures"] += 1
        elif o["result"] == REFUSED:
            c["refused"] += 1
        else:
            if o["slot"] < self.blocked_until:
                c["overlaps"] += 1
                return
            if self.open and o["slot"] < self.group_first + 8:
                b = self.best
                if (o["flips"], -o["metric"]) < (b["flips"], -b["metric"]):
                    self.best = o
                return
            if self.open:
                self.deliver()
                if o["slot"] < self.blocked_until:
                    c["overlaps"] += 1
                    return
            self.open, self.group_first, self.best = True, o["slot"], o

    def deliver(self):
        b = self.best
        self.waiting.append(dict(slot=b["slot"], start_sample=((b["slot"] + 8) * self.F) >> 19, close_slot=b["close_slot"], metric=b["metric"], len=b["len"] - 2,
                                 flips=b["flips"], phase=b["slot"] & 7, addr_ok=b["addr_ok"], fcs=b["fcs"], data=b["data"][:-2]))
        self.counters["frames_repaired" if b["flips"] else "frames_plain"] += 1
        self.open = False
        self.blocked_until = max(b["close_slot"] - 8, 0)
