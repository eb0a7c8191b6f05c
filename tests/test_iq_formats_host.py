"""Packed IQ on the host (no GPU): hd_host_iq_convert against the conversion table, code by code; packed file batches against cf32 batches of the
converted floats, round by round; and the same host code under AddressSanitizer / UBSan in a stand-alone program."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from iq_formats_util import FMTS, all_codes, convert, model

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from habdec_amd.build import build
    build()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_convert_matches_the_table_for_every_code(fmt):
    codes = all_codes(fmt)                                   # every code in I, then every code in Q
    n_codes = {"cs16": 65536, "cs8": 256, "cu8": 256}[fmt]
    assert len(np.unique(codes[:, 0])) == n_codes and len(np.unique(codes[:, 1])) == n_codes
    got = convert(fmt, codes)
    want = model(fmt, codes)                                 # float64, then cast
    assert np.array_equal(got.view(np.float32).reshape(-1, 2).view(np.uint32), want.view(np.uint32))
    # and back: every value is exact, so the table inverts without rounding
    back = {"cs16": lambda v: v * 32768.0, "cs8": lambda v: v * 128.0, "cu8": lambda v: (v * 256.0 + 255.0) / 2.0}[fmt](want.astype(np.float64))
    assert np.array_equal(back, codes.astype(np.float64))


def test_cu8_endpoints_and_sizes():
    import habdec_amd
    L = habdec_amd.lib()
    v = convert("cu8", np.array([[0, 255], [127, 128]], np.uint8)).view(np.float32)
    assert list(v) == [-255.0 / 256.0, 255.0 / 256.0, -1.0 / 256.0, 1.0 / 256.0]          # the centre is 127.5: no code is zero
    v = convert("cs16", np.array([[-32768, 32767]], np.int16)).view(np.float32)
    assert list(v) == [-1.0, 32767.0 / 32768.0]
    v = convert("cs8", np.array([[-128, 127]], np.int8)).view(np.float32)
    assert list(v) == [-1.0, 127.0 / 128.0]
    assert [L.hd_host_iq_bytes(f) for f in (0, 1, 2, 3)] == [8, 4, 2, 2]
    assert L.hd_host_iq_bytes(4) == 0 and L.hd_host_iq_bytes(-1) == 0
    # cf32 through the model is a copy; an unknown format writes nothing
    x = np.arange(10, dtype=np.float32)
    out = np.full(10, 7.0, np.float32)
    L.hd_host_iq_convert(0, x.ctypes.data, 5, out)
    assert np.array_equal(out, x)
    out[:] = 7.0
    L.hd_host_iq_convert(9, x.ctypes.data, 5, out)
    assert np.all(out == 7.0)


CHUNK, GRANULE = 256, 64
# a whole number of chunks (one empty read before the rewind) / one granule short of it / shorter than a chunk and than any stage history / ragged
LENGTHS = [3 * CHUNK, 3 * CHUNK - GRANULE, 100, 1000]


def write_pairs(tmp_path, fmt, lengths=LENGTHS, seed=5):
    """Packed files of random codes and cf32 files of the converted floats."""
    _, dt, _ = FMTS[fmt]
    info = np.iinfo(dt)
    rng = np.random.default_rng(seed)
    packed, plain, datas = [], [], []
    for i, n in enumerate(lengths):
        codes = rng.integers(info.min, info.max + 1, size=(n, 2)).astype(dt)
        p, q = tmp_path / f"s{i}.{fmt}", tmp_path / f"s{i}.cf32"
        codes.tofile(p)
        convert(fmt, codes).tofile(q)
        packed.append(p); plain.append(q); datas.append(codes)
    return packed, plain, datas


@pytest.mark.parametrize("loop", [False, True])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_packed_batches_deliver_what_cf32_batches_of_the_converted_floats_deliver(tmp_path, fmt, loop):
    import habdec_amd
    packed, plain, datas = write_pairs(tmp_path, fmt)
    a = habdec_amd.IqFiles(packed, chunk=CHUNK, granule=GRANULE, loop=loop, fmt=fmt)
    b = habdec_amd.IqFiles(plain, chunk=CHUNK, granule=GRANULE, loop=loop)
    c = habdec_amd.IqFiles(packed, chunk=CHUNK, granule=GRANULE, loop=loop, fmt=FMTS[fmt][0])
    S = len(LENGTHS)
    assert [a.count(s) for s in range(S)] == LENGTHS == [b.count(s) for s in range(S)]
    delivered = np.zeros(S, np.int64)
    for r in range(40):
        sa, na, alive_a = a.next()
        sb, nb, alive_b = b.next()
        raw, nc, alive_c = c.next_raw()
        assert alive_a == alive_b == alive_c, r
        assert list(na) == list(nb) == list(nc), r
        assert [a.rewinds(s) for s in range(S)] == [b.rewinds(s) for s in range(S)] == [c.rewinds(s) for s in range(S)], r
        assert raw.dtype == FMTS[fmt][1] and raw.shape == (S, CHUNK, 2)
        for s in range(S):
            n = int(na[s])
            assert n % GRANULE == 0
            assert np.array_equal(sa[s, :n].view(np.uint32), sb[s, :n].view(np.uint32)), (r, s)
            assert np.array_equal(convert(fmt, raw[s, :n]).view(np.uint32), sa[s, :n].view(np.uint32)), (r, s)
            if not loop:                                             # ... and it is the file, in order
                assert np.array_equal(raw[s, :n], datas[s][delivered[s]:delivered[s] + n]), (r, s)
            delivered[s] += n
    if loop:
        assert all(a.rewinds(s) > 0 for s in range(S))
    else:
        assert list(delivered) == [n - n % GRANULE for n in LENGTHS]


def test_a_cf32_batch_through_the_new_calls_is_the_old_batch(tmp_path):
    import habdec_amd
    _, plain, _ = write_pairs(tmp_path, "cs8")
    a = habdec_amd.IqFiles(plain, chunk=CHUNK, granule=GRANULE, loop=True)
    b = habdec_amd.IqFiles(plain, chunk=CHUNK, granule=GRANULE, loop=True, fmt="cf32")
    for r in range(12):
        sa, na, alive_a = a.next()
        raw, nb, alive_b = b.next_raw()
        assert alive_a == alive_b and list(na) == list(nb)
        assert np.array_equal(sa.view(np.uint32), raw.reshape(sa.shape[0], -1).view(np.uint32)), r
    with pytest.raises(habdec_amd.HabdecError):
        habdec_amd.IqFiles(plain, chunk=CHUNK, granule=GRANULE, fmt=9)


def test_host_code_under_address_and_ub_sanitizers(tmp_path):
    """The stand-alone program (its own main, no Python, no GPU): hd::iq_convert on buffers of exactly n * bps bytes, and hd::IqFileBatch in packed
    mode over the same files as above beside the cf32 batch, with the minimum take hd_ingest_run sets for /64 (347 samples)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ (the compiler the oracle is built with) is needed"
    exe = tmp_path / "iq_formats_asan"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "habdec_amd" / "csrc"),
           str(ROOT / "tests" / "cpp" / "iq_formats_asan.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for fmt in FMTS:
        d = tmp_path / fmt
        d.mkdir()
        packed, plain, _ = write_pairs(d, fmt)
        for loop in (0, 1):
            for min_take in (0, 347):
                args = [str(exe), str(FMTS[fmt][0]), str(CHUNK * 2), str(GRANULE), str(loop), str(min_take), "40"]
                for p, q in zip(packed, plain):
                    args += [str(p), str(q)]
                r = subprocess.run(args, capture_output=True, text=True, timeout=120)
                assert r.returncode == 0 and "iq_formats_asan OK" in r.stdout, (fmt, loop, min_take, r.stdout[-500:], r.stderr[-3000:])
