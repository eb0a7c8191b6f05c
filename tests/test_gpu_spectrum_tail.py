"""The in-wave spectrum at the end of a stream tail, byte for byte against fixtures recorded before its twiddles became a lane-major table, its
division by the rate a guarded product and its `valid` flag a test of the sum (kernels/spectrum_wave.h, spectrum_math.h).

The scenario, the engines and the fixtures' format are tools/record_spectrum_tail.py (which recorded tests/golden/spectrum_tail_*.npz from the parent
commit's library): 64 streams at /64 and 2.048 MS/s, pushes of 65536 samples, nine calls -- the buffer completes in calls 4 and 8 --, through

  batch   the per-CU step kernel, statistics only in the tail, spectrum and power by k_spectrum_wave when the getter asks  (path 3, variant 1)
  eager   the same with HD_EAGER_SPECTRA=1: the tail stores them
  k_step  the single-wave step kernel (HD_NO_CU_STEP=1)
  sync    a synchronous engine: k_tail
  dc      the DC blocker on every stream: the separate kernels, k_spectrum_wave with statistics
  d16     /16: each call's 4096-sample chunk fills the buffer alone (fft_run == 2)

Streams: tone + noise; all zeros; a NaN sample; an Inf sample; amplitude 1e-20 (powers underflow, the division's slow path); amplitude 1e15
(overflow).  Spectrum, power and the seven AFC fields of every stream behind calls 4, 8 and 9 (d16: 1 and 2) must be the recorded bytes, and the
`valid` flag of the statistics -- the AFC takes a noise floor from valid statistics only -- must be set for every ordinary stream and never for
the other five.

Byte for byte means: every value that is not a NaN has the recorded bytes, and a NaN stands exactly where a NaN was recorded.  The sign and payload of a
NaN computed from NaNs are not compared (rec.canonical): IEEE 754 leaves them open, and here they follow the operand order the compiler picks for a
commutative instruction -- the streams with a NaN or an Inf sample showed other NaN bits in the first build of this change, in an all-NaN spectrum."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("record_spectrum_tail", ROOT / "tools" / "record_spectrum_tail.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def hd():
    import habdec_amd
    habdec_amd.lib()
    return habdec_amd


@pytest.fixture(scope="module")
def slab():
    torch = pytest.importorskip("torch")
    return rec.make_slab(torch)


@pytest.fixture(scope="module")
def golden():
    return {g: rec.unpack(np.load(rec.GOLDEN / f"spectrum_tail_{g}.npz")) for g in sorted({c[0] for c in rec.CASES.values()})}


@pytest.mark.parametrize("case", list(rec.CASES))
def test_spectrum_power_and_afc_are_the_recorded_bytes(hd, slab, golden, monkeypatch, case):
    group, S = rec.CASES[case][0], rec.CASES[case][1]
    got = rec.run_case(hd, slab, case, setenv=monkeypatch.setenv, delenv=monkeypatch.delenv)
    want = golden[group]
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    nf = rec.AFC_FIELDS.index("noise_floor")
    for k in sorted(got):
        for s in range(S):
            for kind in ("spec", "power", "afc"):
                assert rec.same_bytes(rec.canonical(got[k][kind][s]), rec.canonical(want[k][kind][s])), (case, "call", k, "stream", s, kind)
            # valid, explicitly: AfcTracker::step takes the noise floor (the mean, dB: never exactly 0 here) from valid statistics and from no others
            valid_seen = got[k]["afc"][s][nf] != 0.0
            assert valid_seen == (s not in rec.INVALID), (case, "call", k, "stream", s, "valid", valid_seen, got[k]["afc"][s])
        for s in rec.INVALID:
            assert not np.isfinite(got[k]["power"][s]).all(), (case, k, s)      # (what makes them invalid shows in the power itself)
