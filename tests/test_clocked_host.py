"""The clocked decoder's host restatement (hd_host_clocked_*) against the numpy model of its definition (tests/clocked_model.py), what it decodes
against what the oracle's chain decodes from the same rows, and the noise ladder of NOTES.md.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import baud_probe_model as M
import clocked_model as CM
from habdec_amd import synth

PUSHES = (1, 63, 64, 65, 511, 512, 4097, None)           # None: the whole stream in one push
BIG = 1 << 16                                             # a record ring nothing of these streams overflows


@pytest.fixture(scope="module")
def hd():
    from habdec_amd.build import build
    build()
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def streams():
    """[(name, row, fsd, baud, nbits, nstops, the model's records, the model's counters)]: computed once."""
    return [s + CM.decode(*s[1:]) for s in CM.streams()]


@pytest.fixture(scope="module")
def raw_push(hd):
    """hd_host_clocked_push by address: a push of one sample costs a call and no numpy slice."""
    f = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_size_t)(("hd_host_clocked_push", hd.lib()))

    def push(h, row, size):
        row = np.ascontiguousarray(row, np.float32)
        base, n = row.ctypes.data, row.size
        for at in range(0, n, size or max(n, 1)):
            f(h.h, base + 4 * at, min(size or n, n - at))
    return push


def test_model_streams_are_what_they_are_meant_to_be(streams):
    by = {s[0]: s for s in streams}
    assert len([s for s in streams if s[0] in {c[0] for c in M.CASES}]) == 9
    assert by["positive"][6] == [] and by["positive"][7]["rejects"] == 0
    assert by["zeros"][6] == [] and by["zeros"][7]["rejects"] == 0
    assert by["square"][6] == [] and by["square"][7]["rejects"] > 1000          # every second position a candidate: rejects only
    assert by["spb4"][3] * 4 == by["spb4"][2] and len(by["spb4"][6]) > 50
    assert by["spb2048"][2] / by["spb2048"][3] == CM.MAX_SPB and len(by["spb2048"][6]) >= 8
    assert "".join(chr(r[1]) for r in by["spb2048"][6]).startswith("$$A,1*ABCD")
    assert len(by["spb130"][6]) > 20 and len(by["spb52"][6]) > 20 and by["specials"][7]["rejects"] > 0


@pytest.mark.parametrize("size", PUSHES, ids=[str(p) for p in PUSHES])
def test_host_equals_model_however_the_stream_is_cut(hd, streams, raw_push, size):
    for name, row, fsd, baud, nbits, nstops, want, counters in streams:
        h = hd.HostClocked(fsd, baud, nbits, nstops, record_cap=BIG)
        raw_push(h, row, size)
        CM.assert_same(CM.as_tuples(h.records()), h.stats(), want, counters, (name, size))
        assert h.stats()["dropped"] == 0
        h.close()


def test_reset_and_set_modem_in_mid_stream(hd, streams):
    by = {s[0]: s for s in streams}
    a, b = by["600_8n2"], by["150_7n1"]
    h = hd.HostClocked(a[2], a[3], a[4], a[5], record_cap=BIG)
    h.push(a[1][:30011])
    assert h.waiting() > 0
    h.reset()
    assert h.waiting() == 0 and h.stats()["samples"] == 0
    h.push(a[1][30011:])
    CM.assert_same(CM.as_tuples(h.records()), h.stats(), *CM.decode(a[1][30011:], *a[2:6]), "across a reset")
    h.push(a[1][:20000])
    h.set_modem(b[3], b[4], b[5])
    for at in range(0, b[1].size, 511):
        h.push(b[1][at:at + 511])
    CM.assert_same(CM.as_tuples(h.records()), h.stats(), b[6], b[7], "across set_modem")
    # tones swapped: the inverted stream with `invert` decodes as the stream itself
    h.set_modem(a[3], a[4], a[5], invert=True)
    h.push(-a[1])
    CM.assert_same(CM.as_tuples(h.records()), h.stats(), a[6], a[7], "invert")
    assert CM.decode(-a[1], *a[2:6], invert=True)[0] == a[6]
    with pytest.raises(hd.HabdecError):
        h.set_modem(a[2] / 3.4, 8, 2)                                          # fewer than 3.5 samples per bit
    with pytest.raises(hd.HabdecError):
        h.set_modem(a[2] / 2049.0, 8, 2)
    with pytest.raises(hd.HabdecError):
        h.set_modem(300, 5, 2)
    with pytest.raises(hd.HabdecError):
        h.set_modem(300, 8, 3)


def test_record_ring_overflow_on_the_host(hd, streams):
    name, row, fsd, baud, nbits, nstops, want, counters = next(s for s in streams if s[0] == "600_8n2")
    h = hd.HostClocked(fsd, baud, nbits, nstops, record_cap=16)
    for at in range(0, row.size, 4097):
        h.push(row[at:at + 4097])
    assert h.stats()["dropped"] == len(want) - 16 and h.stats()["characters"] == len(want)
    assert CM.as_tuples(h.records()) == want[-16:]


def test_nothing_lost_and_nothing_invented(hd):
    """On every text-carrying design signal: what the oracle's extractor, framer and sentence scan decode from the row is among the clocked decoder's
    plain sentences, and every sentence the clocked decoder delivers was transmitted."""
    total = 0
    for c in M.CASES:
        name, baud, nbits, nstops, fsd, sigma, seconds, text = c
        if text is not None or fsd / baud > CM.MAX_SPB:
            continue
        row = M.case_signal(c)
        sent = CM.sent_sentences(seconds, baud, nbits, nstops)
        oracle = CM.oracle_sentences(row, fsd, baud, nbits, nstops)
        h = hd.HostClocked(fsd, baud, nbits, nstops, record_cap=BIG)
        for at in range(0, row.size, 4096):
            h.push(row[at:at + 4096])
        got = h.take_sentences(256)
        plain = [t for (_, flips, t) in got if flips == 0]
        print(name, "oracle", len(oracle), "clocked", len(plain), "repaired", len(got) - len(plain))
        assert oracle and set(oracle) <= set(plain), (name, oracle, plain)
        assert all(t in sent for (_, _, t) in got), (name, got)
        st = h.stats()
        assert st["sentences_plain"] == len(plain) and st["sentences_repaired"] == len(got) - len(plain)
        total += len(got)
    assert total >= 9


# ---- the ladder (NOTES.md has the whole table).  The rungs: the largest sigma of clocked_model.LADDER at which, measured with this code on the CPU,
#   (a) the oracle still loses nothing; (b) the oracle delivers fewer than half and the clocked decoder at least three sentences more; (c) the clocked
#   decoder without repair delivers fewer than half and repair adds at least three.
RUNGS = {"300_8n2": dict(a=0.14, b=0.24, c=0.28), "50_7n2": dict(a=0.25, b=0.40, c=0.45)}


def whole_sentences(modem):
    """The sentences whose last character ends inside the signal."""
    m = CM.LADDER[modem]
    text = M.telemetry_text(m["seconds"], m["baud"], m["nbits"], m["nstops"])
    n, per_char, out, at = int(m["seconds"] * CM.LADDER_FSD), 1 + m["nbits"] + m["nstops"], [], 0
    for s in text.split("\n")[:-1]:
        at += len(s) + 1
        if (3 + at * per_char) * CM.LADDER_FSD / m["baud"] <= n:
            out.append(s.strip("$"))
    return out


def ladder_counts(hd, modem, sigma):
    m = CM.LADDER[modem]
    row = CM.ladder_signal(modem, sigma)
    sent = CM.sent_sentences(m["seconds"], m["baud"], m["nbits"], m["nstops"])
    oracle = CM.oracle_sentences(row, CM.LADDER_FSD, m["baud"], m["nbits"], m["nstops"])
    out = {}
    for name, kw in (("clocked", dict(repair_bits=0)), ("repaired", dict())):
        h = hd.HostClocked(CM.LADDER_FSD, m["baud"], m["nbits"], m["nstops"], record_cap=BIG, **kw)
        h.push(row)
        out[name] = [t for (_, _, t) in h.take_sentences(256)]
    false = [t for t in oracle + out["clocked"] + out["repaired"] if t not in sent]
    assert len(set(oracle)) == len(oracle) and len(set(out["repaired"])) == len(out["repaired"])
    return len(oracle), len(out["clocked"]), len(out["repaired"]), len(false)


@pytest.mark.parametrize("modem", list(RUNGS))
def test_ladder(hd, modem):
    n_sent = len(whole_sentences(modem))
    assert n_sent >= 13
    for rung, sigma in RUNGS[modem].items():
        oracle, clocked, repaired, false = ladder_counts(hd, modem, sigma)
        print(modem, rung, sigma, "sent", n_sent, "oracle", oracle, "clocked", clocked, "with repair", repaired, "false", false)
        assert clocked >= oracle and repaired >= clocked and false == 0, (modem, rung)
        if rung == "a":
            assert oracle == n_sent and clocked == n_sent
        if rung == "b":
            assert 2 * oracle < n_sent and clocked >= oracle + 3
        if rung == "c":
            assert 2 * clocked < n_sent and repaired >= clocked + 3
