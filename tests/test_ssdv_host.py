"""The SSDV receiver's host restatement (hd_host_ssdv_*) against the numpy model of the definition (tests/ssdv_model.py) -- no GPU.

The model finds a trial's codeword by linear elimination (Peterson-Gorenstein-Zierler), the restatement by Berlekamp-Massey and Forney; both accept a
word only if it has 32 zero syndromes, so a mistake the two share would have to lie in the definition's own terms, which the first tests pin.

One reading of the issue's case table is this file's: "erased positions whose bytes were right succeed with erasures_changed 0" cannot happen behind
trial 0 -- a trial with erasures runs only after 17 or more wrong bytes, and erasing right bytes repairs none of them.  The table therefore has the two
cases next to it: low confidence on 24 right bytes costs nothing (trial 0, erasures_changed 0), and eight erasures of which two were right succeed at
trial 1 with erasures_changed 6."""
import zlib

import numpy as np
import pytest

import ssdv_model as SM

CUTS = (1, 255, 256, 257, 4097)
F300 = int(np.floor(8000.0 / 300.0 * 65536 + 0.5))
CHAR_LEN = (11 * F300 + 32768) >> 16                               # 293 samples per 8N2 character at 300 baud and 8 kS/s


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    import habdec_amd.ssdv
    return habdec_amd


@pytest.fixture(scope="module")
def modelled():
    """The case table and the model's answer to every case, computed once."""
    table = SM.case_table()
    return table, {name: SM.decode_stream(b, c) for name, (b, c, _) in table.items()}


def key(p):
    return (p["pos"], p["trial"], p["errors"], p["erasures"], p["erasures_changed"])


def same_packets(got, want):
    fields = ("pos", "trial", "errors", "erasures", "erasures_changed", "data", "type", "callsign", "image_id", "packet_id", "width", "height", "flags",
              "mcu_offset", "mcu_index")
    return len(got) == len(want) and all(all(a[f] == b[f] for f in fields) for a, b in zip(got, want))


# ---------------------------------------------------------------- facts that depend on neither implementation

def test_field_and_code_facts(hd):
    assert SM.alpha_order() == 255
    g = SM.generator()
    assert g == g[::-1] and g[:6] == [1, 91, 127, 86, 16, 30] and len(g) == 33
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 223, dtype=np.uint8).tobytes()
    for enc in (SM.encode, hd.ssdv.encode):
        word = np.frombuffer(b"\x00" + data + enc(data), np.uint8)
        assert not SM.syndromes(word[None, :]).any()
    assert hd.ssdv.encode(data) == SM.encode(data)


def test_crc32(hd):
    assert SM.crc32(b"123456789") == 0xCBF43926
    rng = np.random.default_rng(2)
    for _ in range(4):
        payload = rng.integers(0, 256, 205, dtype=np.uint8).tobytes()
        pkt = hd.ssdv.make_packet(payload, callsign="CRC", packet_id=7)
        assert int.from_bytes(pkt[220:224], "big") == zlib.crc32(pkt[1:220]) & 0xFFFFFFFF      # the restatement's own CRC against zlib
    kw = dict(callsign="AB1", width=320, height=240, packet_id=5, mcu_index=300, image_id=2, flags=1, mcu_offset=3)
    assert hd.ssdv.make_packet(bytes(205), **kw) == SM.make_packet(bytes(205), **kw)
    assert hd.ssdv.make_packet(bytes(205), type=0x67, **kw) == SM.make_packet(bytes(205), type=0x67, **kw)


# ---------------------------------------------------------------- the case table

def test_model_gives_what_the_cases_were_built_for(modelled):
    table, model = modelled
    for name, (b, c, want) in table.items():
        pk, cnt = model[name]
        if want is not None:
            assert [key(p) for p in pk] == want, (name, [key(p) for p in pk])
        assert cnt["decided"] == max(0, len(b) - 255)
    assert model["size255"][1]["decided"] == 0 and model["size256"][1]["decided"] == 1
    for o in (0, 1, 63, 64, 255, 256, 257):
        assert [key(p) for p in model["offset%d" % o][0]] == [(o, 0, 0, 0, 0)]
    assert model["zeros"][1]["crc_bad"] == 4 * 345                   # the zero word is a codeword: every trial of every position finds it
    assert model["sync_wrong"][0][0]["data"][0] == 0x55
    assert model["same_twice"][0][0]["data"] == model["same_twice"][0][1]["data"]
    p = model["size256"][0][0]
    assert (p["callsign"], p["image_id"], p["packet_id"], p["width"], p["height"], p["flags"], p["mcu_offset"], p["mcu_index"], p["type"]) == \
        ("TEST01", 3, 0x0102, 320, 240, 4, 7, 0x0304, 0x66)


@pytest.mark.parametrize("cut", CUTS + (0,))
def test_restatement_equals_model(hd, modelled, cut):
    """Byte for byte, in pushes of `cut` bytes (0: one push, behind other bytes and a reset)."""
    table, model = modelled
    rng = np.random.default_rng(9)
    for name, (b, c, _) in table.items():
        h = hd.ssdv.HostSsdv()
        if cut == 0:
            h.push_bytes(rng.integers(0, 256, 300, dtype=np.uint8).tobytes())
            h.take_packets()
            h.reset()
        step = cut or len(b)
        for at in range(0, len(b), step):
            h.push_bytes(b[at:at + step], None if c is None else c[at:at + step])
        got, st = h.take_packets(), h.stats()
        assert same_packets(got, model[name][0]), (name, cut, [key(p) for p in got], [key(p) for p in model[name][0]])
        assert st == model[name][1], (name, cut, st, model[name][1])


# ---------------------------------------------------------------- the gap rule

def records(hd, pos, ch, conf=1000):
    r = np.zeros(len(pos), hd.capi.CLOCKED_RECORD_DTYPE)
    r["pos"], r["ch"] = pos, ch
    r["data"] = conf
    return r


def test_gap_rule(hd):
    pkt = SM.make_packet(bytes(range(205)), callsign="GAP")
    L = CHAR_LEN
    pos = 5000 + L * np.arange(256)

    def run(keep, char_len, pushes=1, max_fill=7, shift=None):
        p = pos.copy() if shift is None else pos + shift
        r = records(hd, p[keep], np.frombuffer(pkt, np.uint8)[keep])
        r["data"][:, 3] = -77                                        # the smallest magnitude is the confidence
        h = hd.ssdv.HostSsdv(max_fill=max_fill)
        for part in np.array_split(r, pushes):
            h.push_records(part, char_len)
        b, c, fillers, _ = SM.gap_rule(r["pos"], r["ch"], r["data"], char_len, max_fill)
        want, cnt = SM.decode_stream(b, c)
        cnt["fillers"] = fillers
        got, st = h.take_packets(), h.stats()
        assert same_packets(got, want) and st == cnt, (st, cnt)
        return got, st

    every = np.ones(256, bool)
    got, st = run(every, L)
    assert len(got) == 1 and st["fillers"] == 0 and st["bytes"] == 256
    one = every.copy(); one[100] = False
    got, st = run(one, L)
    assert [key(p) for p in got] == [(0, 0, 1, 0, 0)] and st["fillers"] == 1 and got[0]["data"] == pkt     # the filler is one wrong byte in its place
    three = every.copy(); three[[50, 51, 52]] = False
    got, st = run(three, L)
    assert [key(p) for p in got] == [(0, 0, 3, 0, 0)] and st["fillers"] == 3
    got, st = run(one, 0)                                            # the rule switched off: 255 bytes decide nothing
    assert got == [] and st["fillers"] == 0 and st["decided"] == 0
    # a pause of 9 characters or more inserts nothing (k = 9 > 1 + 7), one of 8 is filled
    late = np.where(np.arange(256) >= 128, 8 * L, 0)
    got, st = run(every, L, shift=late)
    assert st["fillers"] == 0 and st["bytes"] == 256 and len(got) == 1
    got, st = run(every, L, shift=np.where(np.arange(256) >= 128, 7 * L, 0))
    assert st["fillers"] == 7 and st["bytes"] == 263
    # a gap that straddles two pushes: the record in front of the gap ends the first push
    keep = every.copy(); keep[128] = False
    got, st = run(keep, L, pushes=2)                                 # array_split of 255 records: 128 + 127, the gap between them
    assert st["fillers"] == 1 and [key(p) for p in got] == [(0, 0, 1, 0, 0)]
    # jitter of less than half a character changes nothing
    got, st = run(one, L, shift=(np.arange(256) * 37) % 100 - 50)
    assert st["fillers"] == 1 and len(got) == 1


# ---------------------------------------------------------------- the ladder

@pytest.fixture(scope="module")
def ladder(hd):
    """sigma -> [plain, gap rule only, all] delivered packets that were sent (of 18), and the packets that were not sent (must be none)."""
    out = {}
    for sigma in (0.26, 0.28, 0.30):
        cells, strangers = [0, 0, 0], 0
        for seed in (3, 4, 5):
            row, sent = SM.ladder_row(seed, sigma)
            hc = hd.HostClocked(8000.0, baud=300.0, bits=8, stops=2)
            hc.push(row)
            rec = hc.records()
            for col, (char_len, only0) in enumerate(((0, True), (CHAR_LEN, True), (CHAR_LEN, False))):
                h = hd.ssdv.HostSsdv()
                h.push_records(rec, char_len)
                got = [p["data"] for p in h.take_packets() if not only0 or p["trial"] == 0]
                strangers += sum(d not in sent for d in got)
                cells[col] += len(set(got) & set(sent))
        out[sigma] = (cells, strangers)
    return out


def test_ladder(ladder):
    """Measured with the restatement (NOTES.md "SSDV packets" has the table): 0.26: 9 / 16 / 16, 0.28: 2 / 2 / 9, 0.30: 0 / 0 / 1 of 18."""
    for sigma, (cells, strangers) in ladder.items():
        print("sigma", sigma, "plain / gap rule / all:", cells, "of 18; not sent:", strangers)
        assert strangers == 0
    a, b, c = ladder[0.28][0]
    assert 2 * a < 18 and c >= b + 3
    a, b, c = ladder[0.26][0]
    assert c >= a + 3


def test_golden_ladder_row_is_current(hd):
    """tests/golden/ssdv_ladder_s3_028.*: what tools/ssdv_host_check.cpp runs under the sanitizers is the ladder's row of seed 3 at sigma 0.28."""
    from pathlib import Path
    gold = Path(__file__).resolve().parent / "golden"
    row, sent = SM.ladder_row(3, 0.28)
    hc = hd.HostClocked(8000.0, baud=300.0, bits=8, stops=2)
    hc.push(row)
    assert hc.records().tobytes() == (gold / "ssdv_ladder_s3_028.records").read_bytes()
    assert b"".join(sent) == (gold / "ssdv_ladder_s3_028.packets").read_bytes()
