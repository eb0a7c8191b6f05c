"""The tone-filter demodulator's host restatement (hd_host_tones_*) against the numpy model of its definition (tests/tones_model.py), byte for byte, and
the noise ladder of NOTES.md: what the clocked decoder delivers from the tone row where the discriminator's row carries nothing.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import tones_model as TM

PUSHES = (1, 63, 64, 65, 4097)
HD_ERR_INVALID, HD_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def hd():
    from habdec_amd.build import build
    build()
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def streams():
    """[(name, iq, fsd, baud, f_hi, f_lo, window_q8, the model's row)]: computed once."""
    return [s + (TM.demod(*s[1:]),) for s in TM.streams()]


def host(hd, fsd, baud, f_hi, f_lo, window_q8):
    return hd.HostTones(fsd, baud, f_hi, f_lo, window_q8=window_q8)


def test_model_streams_are_what_they_are_meant_to_be(hd, streams):
    by = {s[0]: s for s in streams}
    assert len(streams) == 11 + 6
    m = TM.modem(*by["w1"][2:7])
    assert (m["W"], m["full"], m["L"]) == (1, 4, 32) and by["w1"][2] / by["w1"][3] == 3.5
    m = TM.modem(*by["w2048"][2:7])
    assert (m["W"], m["full"], m["L"]) == (2048, 2048, 16384) and by["w2048"][1].size > 4 * 16384
    assert TM.modem(*by["tone_at_0"][2:7])["step_hi"] == 0
    m = TM.modem(*by["tones_at_the_edges"][2:7])
    assert 0x7FFFF000 < m["step_hi"] < 0x80000000 < m["step_lo"] < 0x80001000
    m = TM.modem(*by["tones_negative"][2:7])
    assert m["step_hi"] > m["step_lo"] > 0x80000000
    # a strong signal's row swings to both rails' neighbourhood and follows the bits: positive on the upper tone
    row = by["300_8n2_32k"][7]
    assert row.max() > 0.8 and row.min() < -0.8 and np.abs(by["specials"][7]).max() <= 4.0
    for name, iq, fsd, baud, f_hi, f_lo, q8, want in streams:
        h = host(hd, fsd, baud, f_hi, f_lo, q8)
        st, m = h.stats(), TM.modem(fsd, baud, f_hi, f_lo, q8)
        assert all(st[k] == v for k, v in m.items()) and st["samples"] == 0, (name, st, m)


def test_host_equals_model_in_one_push(hd, streams):
    for name, iq, fsd, baud, f_hi, f_lo, q8, want in streams:
        h = host(hd, fsd, baud, f_hi, f_lo, q8)
        got = h.push(iq)
        assert got.size == iq.size and h.stats()["samples"] == iq.size
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])
        # the clocked decoder's quantisation of the float gives the integer back
        assert np.array_equal(np.trunc(np.clip(got, -4, 4).astype(np.float64) * 1024).astype(np.int64), TM.integers(iq, fsd, baud, f_hi, f_lo, q8)), name


@pytest.fixture(scope="module")
def raw_push(hd):
    """hd_host_tones_push by address: a push of one sample costs a call and no numpy slice."""
    f = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(("hd_host_tones_push", hd.lib()))

    def push(h, iq, size):
        iq = np.ascontiguousarray(iq, np.complex64)
        out = np.zeros(iq.size, np.float32)
        src, dst, n = iq.ctypes.data, out.ctypes.data, iq.size
        for at in range(0, n, size):
            f(h.h, src + 8 * at, min(size, n - at), dst + 4 * at)
        return out
    return push


@pytest.mark.parametrize("size", PUSHES, ids=[str(p) for p in PUSHES])
def test_however_the_stream_is_cut(hd, streams, raw_push, size):
    for name, iq, fsd, baud, f_hi, f_lo, q8, want in streams:
        h = host(hd, fsd, baud, f_hi, f_lo, q8)
        got = raw_push(h, iq, size)
        assert h.stats()["samples"] == iq.size and got.tobytes() == want.tobytes(), (name, size)


def test_reset_set_modem_and_errors(hd, streams):
    by = {s[0]: s for s in streams}
    a, b = by["600_8n2"], by["w1"]
    h = host(hd, *a[2:7])
    h.push(a[1][:30011])
    h.reset()
    assert h.stats()["samples"] == 0 and h.stats()["W"] == TM.modem(*a[2:7])["W"]
    assert h.push(a[1][30011:50000]).tobytes() == TM.demod(a[1][30011:50000], *a[2:7]).tobytes()
    h.push(a[1][:777])
    h.set_modem(1000.0, 300.0, -300.0)                                         # another modem in mid-stream: the stream starts again
    assert h.stats()["samples"] == 0
    assert h.push(b[1]).tobytes() == TM.demod(b[1], a[2], 1000.0, 300.0, -300.0).tobytes()
    h2 = hd.HostTones(a[2])
    assert h2.push(a[1][:100]).size == 0                                       # no modem: passed by
    L = h2.L
    fsd = a[2]
    assert L.hd_host_tones_set_modem(h2.h, fsd / 3.4, 250.0, -250.0) == HD_ERR_UNSUPPORTED
    assert L.hd_host_tones_set_modem(h2.h, fsd / 2049.0, 250.0, -250.0) == HD_ERR_UNSUPPORTED
    assert L.hd_host_tones_set_modem(h2.h, 300.0, fsd / 2, -250.0) == HD_ERR_INVALID
    assert L.hd_host_tones_set_modem(h2.h, 300.0, 250.0, -fsd / 2) == HD_ERR_INVALID
    assert L.hd_host_tones_set_modem(h2.h, 300.0, 250.0, 250.0) == HD_ERR_INVALID
    assert L.hd_host_tones_set_modem(h2.h, 300.0, -250.0, 250.0) == HD_ERR_INVALID
    assert L.hd_host_tones_set_modem(h2.h, 300.0, float("nan"), -250.0) == HD_ERR_INVALID
    assert h2.stats()["F"] == 0
    for q8 in (31, 257):
        h3 = hd.HostTones(fsd, window_q8=q8)
        assert L.hd_host_tones_set_modem(h3.h, 300.0, 250.0, -250.0) == HD_ERR_UNSUPPORTED
    for q8 in (32, 256):
        hd.HostTones(fsd, 300.0, 250.0, -250.0, window_q8=q8)


# ---- the ladder: the weak signal of tests/test_gpu_clocked.py at two noise levels, the oracle's decimated IQ through the tone filters and its discriminator
# row, each into the host clocked decoder.  CRC-valid sentences over the 8 streams.  Measured with this code on the CPU (NOTES.md, "Tone filters"):
#   sigma 0.85: oracle chain 20, discriminator row 28 / 48 (plain / with repair), tone row 55 / 60
#   sigma 1.0:  oracle chain 0,  discriminator row 2 / 4,                          tone row 25 / 39

def ladder_counts(hd, sigma, window_q8=160, offset_hz=0.0):
    iq, sent = TM.weak_iq(sigma)
    fsd = TM.WEAK["fs"] / TM.WEAK["D"]
    out = dict(oracle=0, disc=0, disc_repaired=0, tone=0, tone_repaired=0, false=0)
    for s, (oracle, decim, demod_rows) in enumerate(TM.weak_oracle(iq)):
        out["oracle"] += len(oracle)
        out["false"] += len([t for t in oracle if t not in sent[s]])
        t = hd.HostTones(fsd, TM.WEAK["baud"], TM.SHIFT / 2 + offset_hz, -TM.SHIFT / 2 + offset_hz, window_q8=window_q8)
        tone_rows = [t.push(d) for d in decim]
        for key, rows in (("disc", demod_rows), ("tone", tone_rows)):
            for suffix, kw in (("", dict(repair_bits=0)), ("_repaired", dict())):
                h = hd.HostClocked(fsd, TM.WEAK["baud"], TM.WEAK["bits"], TM.WEAK["stops"], **kw)
                for r in rows:
                    h.push(r)
                got = [x for (_, _, x) in h.take_sentences(256)]
                assert len(set(got)) == len(got)
                out[key + suffix] += len(got)
                out["false"] += len([x for x in got if x not in sent[s]])
    return out


def test_ladder(hd):
    for sigma in (0.85, 1.0):
        c = ladder_counts(hd, sigma)
        print("tones ladder: sigma", sigma, "oracle chain", c["oracle"], "discriminator row", c["disc"], "/", c["disc_repaired"], "tone row", c["tone"], "/",
              c["tone_repaired"], "not sent", c["false"])
        assert c["false"] == 0, (sigma, c)                           # nothing delivered that was not sent
        if sigma == 1.0:
            assert 2 * c["disc_repaired"] < 56, c
            assert c["tone"] >= c["disc_repaired"] + 3, c
            assert c["tone_repaired"] >= c["tone"] + 3, c
