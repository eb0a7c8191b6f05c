"""SSDV packets on the GPU (hd_ssdv_*, kernels/ssdv.hip).

Packets and counters are compared byte for byte with the host restatement (hd_host_ssdv_*), which tests/test_ssdv_host.py holds to the numpy model of
the definition; the guard words around the device buffers must be whole afterwards."""
import numpy as np
import pytest

import baud_probe_model as BM
import ssdv_model as SM

pytestmark = pytest.mark.gpu
S = 8
CUTS = (1, 255, 256, 257, 4097)
F300 = int(np.floor(8000.0 / 300.0 * 65536 + 0.5))
CHAR_LEN = (11 * F300 + 32768) >> 16


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    import habdec_amd.ssdv
    return habdec_amd


@pytest.fixture(scope="module")
def cases(hd):
    """The case table and the restatement's answer to every case (one push), computed once."""
    table = SM.case_table()
    ref = {}
    for name, (b, c, _) in table.items():
        h = hd.ssdv.HostSsdv()
        h.push_bytes(b, c)
        ref[name] = (h.take_packets(), h.stats())
    return table, ref


def rounds(table):
    """The cases dealt to the streams 0 .. 6, seven at a time; stream 7 stays empty."""
    names = list(table)
    return [names[k:k + S - 1] for k in range(0, len(names), S - 1)]


@pytest.mark.parametrize("scan_every_push", [True, False])
def test_case_table_equals_the_host_restatement(hd, cases, scan_every_push):
    table, ref = cases
    eng = hd.Engine(n_streams=S, sampling_rate=32000.0, decimation=4, baud=300, rtty_bits=8, rtty_stops=2, lowpass_bw_hz=1500.0)
    eng.set_rtty(6, 7, 2)                                            # (framing plays no part behind push_bytes: the stream decodes like the others)
    v = hd.ssdv.Ssdv(eng)
    for cut in CUTS:
        for names in rounds(table):
            v.reset()
            longest = max(len(table[n][0]) for n in names)
            for at in range(0, longest, cut):
                for s, n in enumerate(names):
                    b, c, _ = table[n]
                    if at < len(b):
                        v.push_bytes(s, b[at:at + cut], None if c is None else c[at:at + cut])
                if scan_every_push:
                    v.scan()
            v.scan()
            for s, n in enumerate(names):
                got, st = v.take_packets(s), v.stats(s)
                assert got == ref[n][0], (cut, n, [(p["pos"], p["trial"], p["errors"]) for p in got])
                assert st == ref[n][1], (cut, n, st, ref[n][1])
            assert v.take_packets(7) == [] and v.stats(7)["bytes"] == 0
    assert [v.debug_guards(s) for s in range(S)] == [0] * S
    eng.close()


def test_ring_wrap(hd):
    """Three times the ring's capacity, packets across both wraps, in pushes that are no divisor of it -- and all of it in one push and one scan."""
    rng = np.random.default_rng(5)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    pk = [SM.make_packet(rnd(205), callsign="WRAP", packet_id=k) for k in range(4)]
    hit = bytearray(pk[1])
    for j in range(10, 250, 20):
        hit[j] ^= 0x3C                                               # twelve errors in the packet across the first wrap
    b = rnd(4096 - 100) + bytes(hit) + rnd(8192 - 128 - (4096 + 156)) + pk[2] + rnd(500) + pk[3] + pk[0]
    b += rnd(3 * 4096 - len(b))
    assert len(b) == 3 * hd.capi.SSDV_RING
    c = rng.integers(0, 1 << 24, len(b), dtype=np.uint32)
    h = hd.ssdv.HostSsdv()
    h.push_bytes(b, c)
    want, want_st = h.take_packets(), h.stats()
    assert [p["pos"] for p in want] == [3996, 8064, 8820, 9076] and want[0]["errors"] == 12
    eng = hd.Engine(n_streams=2)
    v = hd.ssdv.Ssdv(eng)
    for s, cut in enumerate((1000, len(b))):
        for at in range(0, len(b), cut):
            v.push_bytes(s, b[at:at + cut], c[at:at + cut])
            v.scan()
        assert v.take_packets(s) == want and v.stats(s) == want_st, (s, v.stats(s), want_st)
        assert v.debug_guards(s) == 0
    eng.close()


@pytest.fixture(scope="module")
def chain():
    """The ladder's rows at sigma 0.28 (streams 0 .. 2), one telemetry row (stream 3), and the first row again for a 7-bit modem (stream 6)."""
    rows = [SM.ladder_row(seed, 0.28)[0] for seed in (3, 4, 5)]
    text = BM.fsk_demod(300.0, 8, 2, 8000.0, 0.05, 6.0, seed=11)
    return rows, text


def test_end_to_end_and_nothing_crosses_over(hd, chain):
    rows, text = chain
    n = max(len(r) for r in rows)
    eng = hd.Engine(n_streams=S, sampling_rate=32000.0, decimation=4, baud=300, rtty_bits=8, rtty_stops=2, lowpass_bw_hz=1500.0)
    with_v, without = eng.clocked(), eng.clocked()
    for clk in (with_v, without):
        clk.set_modem(6, 300.0, 7, 2)
    v = hd.ssdv.Ssdv(eng)
    src = {0: rows[0], 1: rows[1], 2: rows[2], 3: text, 6: rows[0]}
    buf = np.zeros((S, 4096), np.float32)
    for at in range(0, n, 4096):
        lens = np.zeros(S, np.uint32)
        for s, r in src.items():
            part = r[at:at + 4096]
            buf[s, :len(part)] = part
            lens[s] = len(part)
        with_v.push_host(buf, lens)
        without.push_host(buf, lens)
        v.push_clocked(with_v)
    # the CPU chain
    for s in range(3):
        hc = hd.HostClocked(8000.0, baud=300.0, bits=8, stops=2)
        hc.push(rows[s])
        hs = hd.ssdv.HostSsdv()
        hs.push_records(hc.records(), CHAR_LEN)
        got, want = v.take_packets(s), hs.take_packets()
        print("stream", s, "packets", [(p["pos"], p["trial"], p["errors"], p["erasures"]) for p in got], v.stats(s))
        assert got == want and v.stats(s) == hs.stats()
    assert sum(sum(v.stats(s)["packets"]) for s in range(3)) >= 3
    # the clocked decoder is what it is without the SSDV object; the 7-bit stream was passed by
    assert with_v.waiting(6) == without.waiting(6) > 0 and v.stats(6)["bytes"] == 0
    assert with_v.waiting(0) == 0 and without.waiting(0) > 0
    for s in range(S):
        sent = without.take_sentences(s)
        assert with_v.take_sentences(s) == sent and (s != 3 or len(sent) >= 1), (s, sent)
        a, b = with_v.stats(s), without.stats(s)
        assert a == b, (s, a, b)
    assert [v.debug_guards(s) for s in range(S)] == [0] * S
    eng.close()


def test_the_engines_own_text_path_is_unaffected(hd):
    """Two engines take the same telemetry IQ; one has a clocked decoder and an SSDV object fed behind every call.  Sentences and their count are the same."""
    from habdec_amd import synth
    text = "".join(synth.make_sentence("PIC", "%d,12:00:%02d,52.1,-0.2,%d" % (k, k, 100 * k)) for k in range(4))
    n = 16000
    iq = synth.fsk_iq_for_text(text, 32000.0, 300.0, chunk=n, sigma=0.05, seed=21)
    got = []
    for with_object in (False, True):
        eng = hd.Engine(n_streams=2, max_chunk=n, sampling_rate=32000.0, decimation=4, baud=300, rtty_bits=8, rtty_stops=2, lowpass_bw_hz=1500.0)
        if with_object:
            clk, v = eng.clocked(), hd.ssdv.Ssdv(eng)
        for at in range(0, len(iq), n):
            eng.process_host(np.ascontiguousarray(np.stack([iq[at:at + n]] * 2)))
            if with_object:
                clk.push_engine()
                v.push_clocked(clk)
        eng.flush()
        got.append(([eng.take_sentences(s) for s in range(2)], eng.sentences_ok()))
        if with_object:
            assert v.stats(0)["bytes"] >= len(text) // 2 and v.take_packets(0) == []       # (the object was fed: the text's characters, no packet among them)
        eng.close()
    # (the first of the four sentences starts inside the chain's start-up and may be lost, with or without the object: the other three are there)
    assert got[0] == got[1] and got[0][1] == sum(len(x) for x in got[0][0]) and all(len(x) >= 3 for x in got[0][0]), got


def test_doors_refuse_what_the_siblings_refuse(hd):
    eng, other = hd.Engine(n_streams=2), hd.Engine(n_streams=2)
    v, clk = hd.ssdv.Ssdv(eng), other.clocked()
    L = eng.L
    assert L.hd_ssdv_push_bytes(None, 0, None, None, 0) == -1 and L.hd_ssdv_push_bytes(v.h, 2, None, None, 0) == -1
    assert L.hd_ssdv_push_bytes(v.h, 0, None, None, 4) == -1 and L.hd_ssdv_stats(v.h, 0, None) == -1
    assert L.hd_ssdv_push_clocked(v.h, clk.h) == -1 and L.hd_ssdv_push_clocked(v.h, None) == -1
    assert L.hd_ssdv_reset(v.h, 2) == -1 and L.hd_ssdv_reset(v.h, 0xFFFFFFFF) == 0
    with pytest.raises(hd.HabdecError):
        hd.ssdv.Ssdv(eng, max_fill=65)
    eng.close(); other.close()
