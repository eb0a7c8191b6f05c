"""Chained tiles of the /32 worker waves (kernels/stage1_ring.h: ring_worker, host/ring_schedule.hpp) against the CPU oracle, on EVERY stream.

A further tile of a chained run takes over the sums that wrapped past lane 63 of the tile before it, so what can go wrong sits at tile and run boundaries,
at the closing run pulled back to the end of a push, at the history carry (moved to whichever tile the schedule marks as a stream's last) and in the ticket
space (chained streams by runs, the guided hand-out's plain streams tile by tile).  The shapes are the smallest that take each path: pushes of 2048 samples
(64 rows: one tile's rows -- a /64 engine refuses so short a push, see the test), 4096 and 6144 (a run shorter than the run length plus a closing tile), 65536 (the full schedule: eight
runs of four and a closing tile, 33 tiles); 64 and 256 streams (8 and 32 per XCD); HD_RING_SHORT_PCT 0 / 25 / 100 (every stream chained / the last quarter
of a share plain / none chained) and HD_RING_CHAIN=0 (the plain grid: the lever).

Every stream is one of five delayed copies of one FSK signal, so the oracle runs five times per shape (once, shared by all cases) and still vouches for
every stream.  Exact mode: every delivered call's discriminator checksum (per call where the read-out shows it, and all of them folded: the engine's
running hash), the symbol count at every read-out and the characters.  Fast mode: symbol counts and characters."""
import numpy as np
import pytest

from habdec_amd import synth

pytestmark = pytest.mark.gpu

K = 5                       # distinct signals; stream s carries signal s % K (5 and the 8 XCDs share no factor: every share sees all of them)
FS, BAUD = 2.048e6, 300
_oracle_cache = {}
_signal_cache = {}


def ck(d):
    d = np.ascontiguousarray(d).view(np.uint32).astype(np.uint64)
    return len(d), int(d.sum() & 0xFFFFFFFF), int((d * np.arange(1, len(d) + 1, dtype=np.uint64)).sum() & 0xFFFFFFFF)


def fold(h, rec):
    for x in rec:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def signals(C, n_calls):
    key = (C, n_calls)
    if key not in _signal_cache:
        _signal_cache.clear()
        frame = synth.rtty_bits(synth.make_sentence("CHAIN", "7,52.1,21.4,100"), 8, 2, 3, 3)
        n = n_calls * C
        base = synth.fsk_iq(np.concatenate([frame] * 4), FS, BAUD, sigma=0.06, seed=71, n_samples=n + 1024 * K)
        _signal_cache[key] = [np.ascontiguousarray(base[977 * k: 977 * k + n]).reshape(n_calls, C) for k in range(K)]
    return _signal_cache[key]


def oracle(C, n_calls, factor):
    """per signal: [(n, ck0, ck1) per call], [cumulative symbols per call], characters, the folded hash"""
    key = (C, n_calls, factor)
    if key not in _oracle_cache:
        from oracle import pyoracle
        out = []
        for sig in signals(C, n_calls):
            o = pyoracle.Decoder("oracle", factor=factor, baud=BAUD, bits=8, stops=2)
            cks, cum, nb, h = [], [], 0, 0xCBF29CE484222325
            for k in range(n_calls):
                o(sig[k], FS)
                cks.append(ck(o.array("last_demod"))); nb += len(o.bits()); cum.append(nb); h = fold(h, cks[-1])
            out.append(dict(cks=cks, cum=cum, chars=o.text("chars_log"), hash=h))
        _oracle_cache[key] = out
    return _oracle_cache[key]


def slab_of(torch, C, n_calls, S):
    sig = torch.from_numpy(np.stack(signals(C, n_calls)).view(np.float32).reshape(K, n_calls, C, 2)).cuda()
    idx = torch.arange(S, device="cuda") % K
    return sig[idx].permute(1, 0, 2, 3).contiguous()          # [n_calls][S][C][2]


def run(monkeypatch, slab, C, S, factor, *, chain=None, pct=None, pipeline=2, arith=0):
    """One engine over the slab's calls.  Returns (per-stream read-outs after every call, end state)."""
    import habdec_amd
    for k, v in (("HD_RING_CHAIN", chain), ("HD_RING_SHORT_PCT", pct)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    eng = habdec_amd.Engine(n_streams=S, max_chunk=C, sampling_rate=FS, decimation=factor, baud=BAUD, rtty_bits=8, rtty_stops=2, pipeline=pipeline, arith=arith)
    try:
        polls = []
        for k in range(slab.shape[0]):
            eng.process_device(slab[k].data_ptr(), C, C)
            polls.append([(eng.demod_checksum(s), eng.bits_total(s)) for s in range(S)])
        t = eng.timing()
        eng.flush()
        end = dict(path=t["path"], variant=t["step_variant"], total=[eng.demod_checksum_total(s) for s in range(S)], bits=[eng.bits_total(s) for s in range(S)],
                   chars=[eng.take_chars(s) for s in range(S)])
    finally:
        eng.close()
    return polls, end


def check_exact(polls, end, orc, n_calls, S, what):
    bad = []
    for k, row in enumerate(polls):
        for s, ((ci, n, c0, c1), nbits) in enumerate(row):
            o = orc[s % K]
            if n is None:                         # nothing delivered yet
                continue
            if (n, c0, c1) != o["cks"][ci]:
                bad.append(("checksum", what, "after call", k, "stream", s, "delivered call", ci))
            if nbits != o["cum"][ci]:
                bad.append(("symbols", what, "after call", k, "stream", s, "delivered call", ci, nbits, o["cum"][ci]))
    for s in range(S):
        o = orc[s % K]
        calls, unknown, h = end["total"][s]
        if (calls, unknown, h) != (n_calls, 0, o["hash"]):
            bad.append(("folded checksums", what, "stream", s, calls, unknown))
        if end["bits"][s] != o["cum"][-1]:
            bad.append(("symbols at the end", what, "stream", s))
        if end["chars"][s] != o["chars"]:
            bad.append(("characters", what, "stream", s))
    assert not bad, (len(bad), bad[:12])


def n_calls_for(C):
    return 6 if C >= 65536 else 12            # (at least six: history carries, both counter sets; the short pushes are cheap)


@pytest.mark.parametrize("S", [64, 256])
@pytest.mark.parametrize("C", [2048, 4096, 6144, 65536])
def test_batch_mode_every_stream_every_hand_out(monkeypatch, C, S):
    """k_step_cu in batch mode: every hand-out setting and the lever give the oracle's checksums, symbol counts and characters on every stream -- and so
    the same checksums as each other."""
    torch = pytest.importorskip("torch")
    n_calls = n_calls_for(C)
    settings = (("chained, short 25", None, 25), ("chained, short 0", None, 0), ("chained, short 100", None, 100), ("HD_RING_CHAIN=0", 0, None))
    if C // 32 < 68:
        # A 2048-sample push is 64 stage-1 outputs, fewer than the 68 samples of history the second stage (/2, 69 taps) carries: the reference leaves that
        # undefined and the engine refuses the call before any launch.  Nothing of the kernel runs at this size; what holds is the refusal, at every setting.
        from habdec_amd.capi import HabdecError
        slab = slab_of(torch, C, 1, S)
        for what, chain, pct in settings:
            with pytest.raises(HabdecError, match="shorter than the second stage's history"):
                run(monkeypatch, slab, C, S, 64, chain=chain, pct=pct)
        return
    orc = oracle(C, n_calls, 64)
    slab = slab_of(torch, C, n_calls, S)
    hashes = {}
    for what, chain, pct in settings:
        polls, end = run(monkeypatch, slab, C, S, 64, chain=chain, pct=pct)
        assert end["path"] == 3 and end["variant"] == 1, (what, end["path"], end["variant"])      # the per-CU step kernel, not a fallback
        check_exact(polls, end, orc, n_calls, S, what)
        hashes[what] = [t[2] for t in end["total"]]
    assert all(h == hashes["HD_RING_CHAIN=0"] for h in hashes.values())
    del slab
    torch.cuda.empty_cache()


def test_stage1_alone_synchronous(monkeypatch):
    """k_stage1_cu<212,32>: stage 1 as a launch of its own (synchronous delivery), eight worker waves per CU."""
    torch = pytest.importorskip("torch")
    C, S, n_calls = 6144, 64, 6
    orc = oracle(C, n_calls, 64)
    slab = slab_of(torch, C, n_calls, S)
    for what, chain in (("chained", None), ("HD_RING_CHAIN=0", 0)):
        polls, end = run(monkeypatch, slab, C, S, 64, chain=chain, pipeline=0)
        assert end["variant"] == 1, (what, end["path"], end["variant"])
        check_exact(polls, end, orc, n_calls, S, what)


def test_plan_128_six_halo_rows(monkeypatch):
    """/128: the /32 first stage with 174 taps, HR = 6 (runs of 250 outputs), in batch mode."""
    torch = pytest.importorskip("torch")
    C, S, n_calls = 65536, 64, 6
    orc = oracle(C, n_calls, 128)
    slab = slab_of(torch, C, n_calls, S)
    for what, chain in (("chained", None), ("HD_RING_CHAIN=0", 0)):
        polls, end = run(monkeypatch, slab, C, S, 128, chain=chain)
        assert end["path"] == 3 and end["variant"] == 1, (what, end["path"], end["variant"])
        check_exact(polls, end, orc, n_calls, S, what)


@pytest.mark.parametrize("C", [4096, 65536])
def test_fast_mode_symbols_and_characters(monkeypatch, C):
    """Fast mode carries both chains of a sum (acc and acc_b) across the tile boundary: symbol counts and characters of every stream."""
    torch = pytest.importorskip("torch")
    S, n_calls = 64, n_calls_for(C)
    orc = oracle(C, n_calls, 64)
    slab = slab_of(torch, C, n_calls, S)
    for pct in (25, 0):
        polls, end = run(monkeypatch, slab, C, S, 64, pct=pct, arith=1)
        assert end["path"] == 3 and end["variant"] == 1
        bad = [(s, end["bits"][s], orc[s % K]["cum"][-1]) for s in range(S) if end["bits"][s] != orc[s % K]["cum"][-1] or end["chars"][s] != orc[s % K]["chars"]]
        bad += [("after call", k, s) for k, row in enumerate(polls) for s, ((ci, n, _, _), nb) in enumerate(row) if n is not None and nb != orc[s % K]["cum"][ci]]
        assert not bad, (pct, len(bad), bad[:12])
