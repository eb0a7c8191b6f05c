"""The scenario of tests/test_gpu_spectrum_tail.py, and the recorder of its golden bytes (tests/golden/spectrum_tail_<group>.npz).

    python3 tools/record_spectrum_tail.py [--lib PATH/TO/libhabdec_amd.so]      # needs the GPU

The in-wave spectrum (kernels/spectrum_wave.h) is compared with nothing but itself: its bins, its power values, its statistics and its `valid` flag
must stay the bytes they were when the fixtures were recorded -- from the library of the commit BEFORE the tail's transform was changed (twiddles
from a lane-major table, the division by the rate as a guarded product, `valid` from the sum), given with --lib.  A later change that is meant to
alter these bytes records them again from its own parent and says so.

Scenario: 64 streams (16 at /16), 2.048 MS/s, pushes of 65536 samples.  /64: 1024 decimated samples per call, so the 4096-sample spectrum buffer
completes in calls 4 and 8; nine calls are two completed buffers per stream and one call beyond.  /16: every call's 4096-sample chunk fills the buffer
alone (StreamCall::fft_run == 2).  Streams are a tone plus noise (two signals, even and odd streams), except: stream 3 all zeros; 5 with a NaN sample
and 7 with an Inf sample in the middle of every call; 9 at amplitude 1e-20 (its powers underflow: the division's slow path); 11 at amplitude 1e15
(they overflow).  None of those five may ever deliver valid statistics.

A snapshot holds, per stream, the spectrum, the power and the seven AFC fields.  The files keep each distinct row once, with an index per stream."""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"

FS, C, BAUD = 2.048e6, 65536, 50
NCALLS = 9
ZERO, NAN, INF, TINY, HUGE = 3, 5, 7, 9, 11
INVALID = (ZERO, NAN, INF, TINY, HUGE)
AFC_FIELDS = ("correction", "shift_hz", "noise_floor", "noise_var", "peak_l", "peak_r", "spectra")

# name: (golden group, streams, decimation, pipeline, arith, environment, DC blocker, calls, snapshots behind calls, (path, step_variant or None) from call 2, or None)
CASES = {
    "batch":     ("main", 64, 64, 2, 0, {},                          False, 9, (4, 8, 9), (3, 1)),
    "eager":     ("main", 64, 64, 2, 0, {"HD_EAGER_SPECTRA": "1"},   False, 9, (4, 8, 9), (3, 1)),
    "k_step":    ("main", 64, 64, 2, 0, {"HD_NO_CU_STEP": "1"},      False, 9, (4, 8, 9), (3, 0)),
    "sync":      ("main", 64, 64, 0, 0, {},                          False, 9, (4, 8, 9), (2, None)),
    "dc":        ("dc",   64, 64, 2, 0, {},                          True,  9, (4, 8, 9), (0, None)),
    "d16":       ("d16",  16, 16, 2, 0, {},                          False, 2, (1, 2),    None),
}


def signals():
    """[7][NCALLS * C] complex64: the two tone + noise signals and the five special streams."""
    n = NCALLS * C
    t = np.arange(n, dtype=np.float64) / FS
    base = []
    for j, (f, seed) in enumerate(((3100.0, 71), (-5300.0, 72))):
        rng = np.random.default_rng(seed)
        x = 0.5 * np.exp(2j * np.pi * f * t + 0.4j * j) + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        base.append(x.astype(np.complex64))
    mid = np.arange(NCALLS) * C + C // 2
    nan, inf = base[1].copy(), base[1].copy()
    nan[mid] = np.float32("nan")
    inf[mid] = np.float32("inf")
    out = np.stack([base[0], base[1], np.zeros(n, np.complex64), nan, inf, (base[1] * np.float32(1e-20)).astype(np.complex64),
                    (base[1] * np.float32(1e15)).astype(np.complex64)])
    out.setflags(write=False)
    return out


def stream_signal(S):
    """Row of signals() that stream s carries."""
    m = np.arange(S) % 2
    for s, row in ((ZERO, 2), (NAN, 3), (INF, 4), (TINY, 5), (HUGE, 6)):
        m[s] = row
    return m


def make_slab(torch, S=64):
    """[NCALLS][S][C][2] float32 on the device."""
    sig = signals()
    base = torch.from_numpy(sig.view(np.float32).reshape(sig.shape[0], NCALLS, C, 2).copy()).cuda()
    out = base[torch.from_numpy(stream_signal(S)).cuda()].permute(1, 0, 2, 3).contiguous()
    torch.cuda.synchronize()
    return out


def snapshot(eng, S):
    """(power first on the odd streams, the spectrum first on the even ones: either getter brings both up to date)"""
    spec, power, afc = np.zeros((S, 4096), np.complex64), np.zeros((S, 4096), np.float32), np.zeros((S, len(AFC_FIELDS)), np.float64)
    for s in range(S):
        if s % 2:
            p = eng.power(s); x = eng.spectrum(s)
        else:
            x = eng.spectrum(s); p = eng.power(s)
        assert x.size == 4096 and p.size == 4096, (s, x.size, p.size)
        spec[s], power[s] = x, p
        a = eng.afc(s)
        afc[s] = [a[k] for k in AFC_FIELDS]
    return {"spec": spec, "power": power, "afc": afc}


def run_case(hd, slab64, name, setenv=os.environ.__setitem__, delenv=os.environ.pop):
    """{call: snapshot} of one engine; the route is asserted as the case says."""
    _, S, D, pipeline, arith, env, dc, ncalls, snaps, route = CASES[name]
    for k, v in env.items():
        setenv(k, v)
    try:
        eng = hd.Engine(n_streams=S, max_chunk=C, sampling_rate=FS, decimation=D, baud=BAUD, pipeline=pipeline, arith=arith)
    finally:
        for k in env:
            delenv(k)
    if dc:
        for s in range(S):
            eng.set_dc_remove(s, True)
    out = {}
    for k in range(1, ncalls + 1):
        # (the slab is [call][64 streams][C]: an engine of fewer streams reads the first ones, stride C between streams)
        eng.process_device(slab64[k - 1].data_ptr(), C, C)
        t = eng.timing()
        if route is not None and k >= 2:
            assert t["path"] == route[0] and route[1] in (None, t["step_variant"]), (name, k, t)
        if k in snaps:
            eng.flush()            # (deliver: a getter answers nothing while the call that completed the buffer is undelivered)
            out[k] = snapshot(eng, S)
    eng.close()
    return out


def pack(snaps):
    """{call: snapshot} -> arrays for np.savez: the distinct rows of each kind, once, and [snapshot][stream] indices into them."""
    calls = sorted(snaps)
    out = {"calls": np.array(calls, np.int32)}
    for kind in ("spec", "power", "afc"):
        rows = np.concatenate([snaps[k][kind] for k in calls])
        raw = np.ascontiguousarray(rows).view(np.uint8).reshape(rows.shape[0], -1)
        uniq, index = np.unique(raw, axis=0, return_inverse=True)
        out[kind + "_rows"] = uniq.view(rows.dtype).reshape(uniq.shape[0], rows.shape[1])
        out[kind + "_index"] = index.reshape(len(calls), -1).astype(np.int32)
    return out


def unpack(z):
    """The inverse of pack(): {call: snapshot}."""
    return {int(k): {kind: z[kind + "_rows"][z[kind + "_index"][i]] for kind in ("spec", "power", "afc")} for i, k in enumerate(z["calls"])}


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def canonical(a):
    """`a` with every NaN replaced by the one quiet NaN of its format.  Which NaN an operation on NaNs returns -- sign and payload -- is left open by
    IEEE 754 and depends here on the operand order the compiler happens to pick (v_sub_f32 a, b against v_subrev_f32 b, a): those bits are no property of
    the arithmetic, and two builds of the same source may differ in them.  Where a value is a NaN is one, and every other value's bytes are."""
    a = np.ascontiguousarray(a)
    f = a.view(np.float32 if a.dtype in (np.complex64, np.float32) else np.float64).copy()
    f[np.isnan(f)] = np.nan
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="the library to record from (default: the tree's own)")
    ap.add_argument("--out", default=str(GOLDEN))
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import torch
    import habdec_amd
    from habdec_amd import capi
    if a.lib:
        capi.LIB_PATH = Path(a.lib).resolve()
    habdec_amd.lib()
    slab = make_slab(torch)
    groups = {}
    for name in CASES:
        group = CASES[name][0]
        snaps = run_case(habdec_amd, slab, name)
        if group in groups:        # the engines of a group must agree in the library recorded from, or the group is no fixture
            for k, snap in snaps.items():
                for kind in snap:
                    assert same_bytes(snap[kind], groups[group][k][kind]), (name, "differs from its group", group, k, kind)
        else:
            groups[group] = snaps
        nf = AFC_FIELDS.index("noise_floor")
        print(name, "ok; streams without a noise floor (never valid):", {k: [s for s in range(snap["afc"].shape[0]) if snap["afc"][s][nf] == 0.0] for k, snap in snaps.items()}, flush=True)
    for group, snaps in groups.items():
        path = Path(a.out) / f"spectrum_tail_{group}.npz"
        np.savez_compressed(path, **pack(snaps))
        back = unpack(np.load(path))
        assert all(same_bytes(back[k][kind], snaps[k][kind]) for k in snaps for kind in snaps[k])
        print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
