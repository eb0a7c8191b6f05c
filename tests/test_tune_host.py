"""Per-stream digital tuning, host side (include/habdec_amd_host.h hd_host_tune_*): the step, the phasor tables and the rotation the kernels run,
pinned against a numpy float32 restatement of the contract in include/habdec_amd.h.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from habdec_amd.build import build
    build()
    import habdec_amd
    return habdec_amd.lib()


def model_tables():
    coarse = np.array([[math.cos(2 * math.pi * a / 256), math.sin(2 * math.pi * a / 256)] for a in range(256)], np.float32)
    fine = np.array([[math.cos(2 * math.pi * b / 65536), math.sin(2 * math.pi * b / 65536)] for b in range(256)], np.float32)
    return coarse, fine


def cmul(ur, ui, vr, vi):
    # numpy float32 rounds every product and every sum on its own: (ur vr - ui vi, ur vi + ui vr) without FMA
    return ur * vr - ui * vi, ur * vi + ui * vr


def model_rotate(x: np.ndarray, phase: int, step: int) -> np.ndarray:
    coarse, fine = model_tables()
    theta = (np.uint64(phase) + np.arange(len(x), dtype=np.uint64) * np.uint64(step)) & np.uint64(0xFFFFFFFF)
    a, b = (theta >> np.uint64(24)).astype(np.int64), ((theta >> np.uint64(16)) & np.uint64(255)).astype(np.int64)
    pr, pi = cmul(coarse[a, 0], coarse[a, 1], fine[b, 0], fine[b, 1])
    yr, yi = cmul(x.real.astype(np.float32), x.imag.astype(np.float32), pr, pi)
    out = np.empty(len(x), np.complex64)
    out.real, out.imag = yr, yi
    return out


def model_step(f: float, fs: float) -> int:
    return int(np.int64(np.round(-(f / fs) * 4294967296.0))) & 0xFFFFFFFF     # np.round: half to even, like nearbyint


def host_step(L, f, fs):
    d = C.c_uint32(0)
    rc = L.hd_host_tune_step(f, fs, C.byref(d))
    return rc, d.value


def test_tables_equal_libm_rounded_once(L):
    coarse, fine = np.zeros(512, np.float32), np.zeros(512, np.float32)
    L.hd_host_tune_tables(coarse, fine)
    mc, mf = model_tables()
    assert np.array_equal(coarse.view(np.uint32), mc.reshape(-1).view(np.uint32))
    assert np.array_equal(fine.view(np.uint32), mf.reshape(-1).view(np.uint32))
    assert coarse[0] == 1.0 and coarse[1] == 0.0 and fine[0] == 1.0 and fine[1] == 0.0


@pytest.mark.parametrize("fs", [32000.0, 128000.0, 2.048e6 / 64, 2.5e6 / 16])
def test_step_matches_the_formula(L, fs):
    offsets = [0.0, 1.0, -1.0, 300.0, -300.0, 2500.5, -2500.5, -4000.0, 4000.0, fs / 2 - 1, -(fs / 2 - 1), 1e-3, 0.123456789]
    # ties: offsets whose step is an exact half-integer before rounding (k + 1/2) / 2^32 * fs
    offsets += [(k + 0.5) / 4294967296.0 * fs for k in (0, 1, 2, 3, 1000, 1001)] + [-(k + 0.5) / 4294967296.0 * fs for k in (0, 1, 2, 3)]
    for f in offsets:
        rc, d = host_step(L, f, fs)
        assert rc == 0, f
        assert d == model_step(f, fs), (f, d, model_step(f, fs))
    assert host_step(L, 0.0, fs) == (0, 0)
    for bad in (fs / 2, -fs / 2, fs, -fs, float("inf"), float("nan")):
        assert host_step(L, bad, fs)[0] == -1, bad


def test_step_ties_round_half_to_even(L):
    fs = 4294967296.0          # one Hz is one unit of the step: -(f / fs) * 2^32 = -f exactly
    for f, want in [(0.5, 0), (1.5, -2), (2.5, -2), (-0.5, 0), (-1.5, 2), (-2.5, 2), (3.5, -4)]:
        rc, d = host_step(L, f, fs)
        assert rc == 0 and d == want & 0xFFFFFFFF, (f, d)


@pytest.mark.parametrize("n,phase,step", [(1000, 0, 123456789), (4097, 0xFFFFF000, 0x01234567), (63, 0x80000000, 0xFFFFFFFF),
                                          (130, 7, 0x7FFFFFFF), (777, 0xFFFFFFFF, model_step(2500.5, 32000.0))])
def test_rotate_equals_the_model(L, n, phase, step):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(3.0)
    x[:4] = [0, -0.0, 1e-30, -1e30]
    out = np.zeros(2 * n, np.float32)
    L.hd_host_tune_rotate(x.view(np.float32), n, phase, step, out)
    want = model_rotate(x, phase, step)
    assert np.array_equal(out.view(np.uint32), want.view(np.float32).view(np.uint32))
    # the phase wraps inside the run
    assert (phase + (n - 1) * step) >> 32 or step == 0 or n < 2


def test_rotate_shifts_a_tone_to_zero():
    """A tone at +f rotated with the step of +f lands at 0 Hz (the rest of the chain sees a receiver tuned f higher)."""
    import habdec_amd
    L = habdec_amd.lib()
    fs, f, n = 32000.0, 2500.0, 4096
    x = np.exp(2j * np.pi * f / fs * np.arange(n)).astype(np.complex64)
    rc, d = host_step(L, f, fs)
    assert rc == 0
    out = np.zeros(2 * n, np.float32)
    L.hd_host_tune_rotate(x.view(np.float32), n, 0, d, out)
    y = out.view(np.complex64)
    assert np.abs(y - y[0]).max() < 1e-3 and abs(abs(y[0]) - 1) < 1e-5


def test_tuning_symbols_are_exported_and_bound(L):
    from habdec_amd import capi
    for name in ("hd_stream_set_tune", "hd_stream_set_auto_afc", "hd_stream_tune"):
        assert hasattr(L, name) and name in capi.ENGINE_API
    for name in ("hd_host_tune_step", "hd_host_tune_tables", "hd_host_tune_rotate"):
        assert hasattr(L, name) and name in capi.HOST_API
    assert C.sizeof(capi.hd_tune_info) == 40
