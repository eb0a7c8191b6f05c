"""The rows tests/test_afsk_host.py and tests/test_gpu_afsk.py decode: AX.25 frames assembled bit by bit here in Python (not by the library's encoder,
which one host test holds to this file), turned into audio by habdec_amd.afsk.afsk_audio.

A case is (modem, params, row, expect): modem = (baud, mark, space); params for Afsk / HostAfsk / AfskModel; row float32 at FS; expect: the frames that
must be delivered, as (frame bytes without FCS, flips), in order."""
import numpy as np

from afsk_model import crc16, walk_bits

FS = 32000.0
BELL = (1200.0, 1200.0, 2200.0)
HF = (300.0, 1600.0, 1800.0)
FAST = (4000.0, 4000.0, 8000.0)                      # 8 samples a bit at 32 kS/s
SMALL = dict(max_frame_bytes=64, max_push=8192)      # L = 623 bits: a short tail behind every frame
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def address(call: str, ssid=0, last=False, h=False) -> bytes:
    return bytes(ord(c) << 1 for c in call.ljust(6)) + bytes([0x60 | ssid << 1 | int(last) | (0x80 if h else 0)])


def with_fcs(body: bytes) -> bytes:
    c = crc16(body)
    return body + bytes([c & 0xFF, c >> 8])


def ui_frame(info: bytes, dst="APRS", src="N0CALL", ssid=11, digis=()) -> bytes:
    a = address(dst) + address(src, ssid, last=not digis)
    for k, (call, s, h) in enumerate(digis):
        a += address(call, s, last=k + 1 == len(digis), h=h)
    return with_fcs(a + b"\x03\xf0" + info)


def stuffed(frame: bytes) -> list:
    """The frame's bits, least significant first, a 0 behind every five 1s."""
    out, ones = [], 0
    for byte in frame:
        for k in range(8):
            b = byte >> k & 1
            out.append(b)
            ones = ones + 1 if b else 0
            if ones == 5:
                out.append(0)
                ones = 0
    return out


def nrzi(bits, level=0) -> list:
    out = []
    for b in bits:
        if not b:
            level ^= 1
        out.append(level)
    return out


def on_air(frames, before=8, between=1, after=2) -> list:
    """Bits: `before` flags, the frames with `between` flags between two of them, `after` flags."""
    bits = FLAG * before
    for k, f in enumerate(frames):
        if k:
            bits = bits + FLAG * between
        bits = bits + stuffed(f)
    return bits + FLAG * after


def row_of(levels, modem=BELL, params=SMALL, start=300.25, bit_peak=None, tail_bits=None, peak=0.5) -> np.ndarray:
    """The levels as audio with silence around them; behind them the walk's L bits and a few more, so that every candidate is decided."""
    from habdec_amd.afsk import afsk_audio
    baud, mark, space = modem
    L = walk_bits(params.get("max_frame_bytes", 332))
    tail = L + 24 if tail_bits is None else tail_bits
    n = int(start + (len(levels) + tail) * FS / baud)
    return afsk_audio(levels, FS, baud, mark, space, peak=peak, start=start, n_samples=n, bit_peak=bit_peak).astype(np.float32)


def isolated(levels, lo, hi) -> list:
    """The positions lo <= r < hi whose level differs from both neighbours': a weak wrong tone there reads wrong on every timing phase."""
    return [r for r in range(lo, hi) if levels[r - 1] != levels[r] != levels[r + 1]]


def calm(levels, lo, hi) -> list:
    """Those of them that stand in a run of four 0 bits (five alternating levels): turned over, they make 0,1,1,0 and move no stuffing."""
    return [r for r in isolated(levels, lo, hi) if levels[r - 2] != levels[r - 1] and levels[r + 1] != levels[r + 2]]


def weak_wrong(levels, positions, wrong_peak=0.06):
    """(levels, bit_peak) with the levels at `positions` replaced by a weak opposite tone."""
    lv, pk = list(levels), [0.5] * len(levels)
    for r in positions:
        lv[r] ^= 1
        pk[r] = wrong_peak
    return lv, pk


INFO = b"!4903.50N/07201.75W-balloon 0123"          # 32 bytes: a 50-byte frame


def frame_cases() -> dict:
    """name -> (modem, params, row, expect)."""
    cases = {}
    f = ui_frame(INFO)
    body0 = 8 * len(FLAG)                                # the first bit behind the preamble of 8 flags

    def add(name, bits, expect, modem=BELL, params=SMALL, **kw):
        cases[name] = (modem, params, row_of(nrzi(bits), modem, params, **kw), expect)

    add("plain", on_air([f]), [(f[:-2], 0)])
    f17 = with_fcs(address("APRS") + address("N0CALL", 11, last=True) + b"\x03")
    add("min_17_bytes", on_air([f17]), [(f17[:-2], 0)])
    f16 = with_fcs(address("APRS") + address("N0CALL", 11, last=True))
    add("16_bytes_unshaped", on_air([f16]), [])
    f64 = ui_frame(bytes(range(65, 65 + 46)))
    assert len(f64) == 64
    add("max_small", on_air([f64]), [(f64[:-2], 0)])
    f65 = ui_frame(bytes(range(65, 65 + 47)))
    add("one_byte_more_unshaped", on_air([f65]), [])
    f332 = ui_frame(bytes((37 * k + 11) % 95 + 32 for k in range(332 - 18)))
    assert len(f332) == 332
    add("max_332", on_air([f332]), [(f332[:-2], 0)], params=dict(max_push=8192))
    fff = ui_frame(b"\xff" * 24)
    add("payload_ff", on_air([fff]), [(fff[:-2], 0)])
    bits = on_air([f])
    add("abort_inside", bits[:body0 + 200] + [1] * 9 + bits[body0 + 200:], [])
    g = ui_frame(b">second frame", src="W1AW", ssid=0, digis=(("WIDE1", 1, True), ("WIDE2", 2, False)))
    add("shared_flag", on_air([f, g], between=1), [(f[:-2], 0), (g[:-2], 0)])
    add("preamble_1", on_air([f], before=1), [(f[:-2], 0)])
    add("preamble_40", on_air([f], before=40), [(f[:-2], 0)])
    add("open_walk", FLAG * 4 + [0, 1] * 400 + FLAG * 2, [])
    add("hf_300_baud", on_air([f]), [(f[:-2], 0)], modem=HF)

    # ---- repair: chosen levels replaced by a weak opposite tone
    lv = nrzi(on_air([f]))
    end = len(lv) - 2 * 8 - 8
    iso = calm(lv, body0 + 16, end)
    pick = [iso[len(iso) // 5], iso[len(iso) // 2], iso[4 * len(iso) // 5]]

    def add_weak(name, levels, positions, expect, extra_weak=(), **kw):
        wl, pk = weak_wrong(levels, positions)
        for r, p in extra_weak:
            pk[r] = p
        cases[name] = (BELL, dict(SMALL, **kw), row_of(wl, BELL, SMALL, bit_peak=pk), expect)

    add_weak("repair_1", lv, pick[:1], [(f[:-2], 1)])
    add_weak("repair_2", lv, pick[:2], [(f[:-2], 2)])
    add_weak("repair_3_fails", lv, pick, [])
    add_weak("repair_off", lv, pick[:1], [], repair_flips=0)
    # a byte 0x1F is 1,1,1,1,1,(stuffed 0),0,0,0 on air: the level behind the stuffed bit differs from both neighbours'
    fs_ = ui_frame(b"abc\x1fdefgh")
    sb = stuffed(fs_)
    at = next(i for i in range(16 * 8, len(sb) - 4) if sb[i - 5:i + 3] == [1, 1, 1, 1, 1, 0, 0, 0] and sb[i - 6] == 0)      # i: the stuffed bit
    lvs = nrzi(on_air([fs_]))
    assert body0 + at + 1 in isolated(lvs, body0, len(lvs) - 24)
    add_weak("repair_next_to_stuffed", lvs, [body0 + at + 1], [(fs_[:-2], 1)])
    # '~' (0x7E) at frame byte 17 is 0,1,1,1,1,1,(stuffed 0),1,0 on air: the stuffed bit's level turned over makes 0,1,1,1,1,1,1,0, a flag behind 17 bytes.
    # The level behind it is correct but weaker still, so that the late timing phases read the wrong level too.
    ft = ui_frame(b"A~ and more text")
    st = stuffed(ft)
    at = next(i for i in range(17 * 8, 18 * 8 + 2) if st[i - 6:i + 3] == [0, 1, 1, 1, 1, 1, 0, 1, 0])
    lvt = nrzi(on_air([ft]))
    add_weak("false_closing_flag", lvt, [body0 + at], [], extra_weak=[(body0 + at + 1, 0.02)])
    # a callsign byte that is none, under a right FCS: the repair finds the frame and the address check turns it away
    fb = with_fcs(address("APRS") + address("N0call", 11, last=True) + b"\x03\xf0" + INFO)
    lvb = nrzi(on_air([fb]))
    isob = calm(lvb, body0 + 16 * 8, len(lvb) - 24)
    add_weak("repair_refused_callsign", lvb, isob[len(isob) // 2:len(isob) // 2 + 1], [])
    add("plain_refused_callsign", on_air([fb]), [])
    # eight samples a bit, a slot a sample: 66000 samples of faint noise in front of the frame take the slot ring round once
    quiet = (0.02 * np.random.default_rng(77).standard_normal(66000)).astype(np.float32)
    cases["ring_wrap"] = (FAST, SMALL, np.concatenate([quiet, row_of(nrzi(on_air([f])), FAST, SMALL)]), [(f[:-2], 0)])
    cases["plain_bad_callsign_allowed"] =(BELL, dict(SMALL, require_addr=0), cases["plain_refused_callsign"][2], [(fb[:-2], 0)])
    return cases


def specials(row: np.ndarray, seed=5) -> np.ndarray:
    """The row with NaN, +-Inf and values beyond +-4 in it."""
    out = row.copy()
    rng = np.random.default_rng(seed)
    at = rng.choice(out.size, 64, replace=False)
    out[at] = np.tile(np.array([np.nan, np.inf, -np.inf, 4.5, -4.5, 1e30, -1e30, 3.99999], np.float32), 8)
    return out


def cuts(n, sizes=(1, 63, 64, 65, 4097), shift=0):
    """(start, stop) of the pushes that take n samples in pieces of `sizes` in turn."""
    at, k = 0, shift
    while at < n:
        m = min(sizes[k % len(sizes)], n - at)
        yield at, at + m
        at += m
        k += 1
