"""bench.py --dump-outputs and the split between a plain run and --full.

CPU: dump_outputs against a stand-in engine -- the arrays and their dtypes, the 64 MB bound, the fixed seeded sample of streams above it.
GPU: a plain run prints the headline fields and nothing of --full, and its outputs are the same run to run and the same as a --full run's."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


class _Eng:
    """Answers like habdec_amd.Engine's getters; stream s's values depend on s alone."""

    def __init__(self, m):
        self.m = m

    def demodulated(self, s): return np.arange(self.m, dtype=np.float32) + s
    def spectrum(self, s): return (np.arange(4096) + 1j * s).astype(np.complex64)
    def power(self, s): return np.full(4096, s, np.float32)
    def afc(self, s): return {"correction": 0.5 * s, "shift_hz": 1.0, "noise_floor": 2.0, "noise_var": 3.0, "peak_l": 4, "peak_r": 5, "spectra": s}
    def bits(self, s): return np.ones(s % 3, np.uint8)
    def bits_total(self, s): return 10 * s


def test_dump_outputs_writes_every_stream_within_the_bound(tmp_path):
    sys.path.insert(0, str(ROOT))
    import bench
    info = bench.dump_outputs(_Eng(1024), tmp_path, 16)
    assert info["streams"] == 16 and info["bytes"] <= bench.DUMP_BUDGET_BYTES
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(got) == {"demodulated", "spectrum", "power", "afc", "symbols", "symbols_total", "streams"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["streams"], np.arange(16))
    assert got["demodulated"].shape == (16, 1024) and got["demodulated"][5, 0] == 5
    assert got["spectrum"].shape == (16, 4096, 2) and got["spectrum"][3, 7, 1] == 3
    assert got["afc"].shape == (16, 7) and got["afc"][4, 0] == 2.0
    assert got["symbols"].shape == (16, 2) and got["symbols"][0, 0] == -1 and got["symbols"][2, 1] == 1      # shorter rows padded with -1
    assert np.array_equal(got["symbols_total"][:, 0], 10.0 * np.arange(16))


def test_dump_outputs_samples_a_fixed_subset_above_64_mb(tmp_path):
    sys.path.insert(0, str(ROOT))
    import bench
    a = bench.dump_outputs(_Eng(1 << 16), tmp_path / "a", 1024)            # 1024 streams x ~330 KB: over the bound
    b = bench.dump_outputs(_Eng(1 << 16), tmp_path / "b", 1024)
    assert 0 < a["streams"] < 1024 and a["bytes"] <= bench.DUMP_BUDGET_BYTES
    sa, sb = np.load(tmp_path / "a" / "streams.npy"), np.load(tmp_path / "b" / "streams.npy")
    assert np.array_equal(sa, sb) and np.all(np.diff(sa) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "demodulated.npy")[:, 0], sa.astype(np.float32))
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= bench.DUMP_BUDGET_BYTES + 4096


def _run(*args):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_headline_and_outputs_equal_a_full_runs(tmp_path):
    """Child processes: this one's GPU context stays as it is."""
    common = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--prewarm", "8", "--streams", "64"]
    a = _run(*common, "--dump-outputs", str(tmp_path / "a"))
    b = _run(*common, "--dump-outputs", str(tmp_path / "b"))
    f = _run(*common, "--dump-outputs", str(tmp_path / "f"), "--full", "--arith", "exact", "--no-cpu-baseline", "--no-also")
    for line in (a, b):
        assert line["steps"] == 6 and line["value"] > 0 and line["unit"] == "MS/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["ms_per_step"] == pytest.approx(line["timed_region_ms"] / 6, rel=1e-2)
        assert line["full"] is False and not {"cold", "roofline", "box", "cpu_baseline", "fast", "also"} & set(line)
    assert f["full"] is True and f["cold"]["steps"] == 6 and f["roofline"]["kernel"] and f["cpu_baseline"]["gpu_matches_oracle_on_sample"] is True
    names = sorted(p.name for p in (tmp_path / "a").glob("*.npy"))
    assert "demodulated.npy" in names and a["outputs"]["streams"] == 64
    for n in names:
        x = np.load(tmp_path / "a" / n)
        assert x.dtype in (np.float32, np.float64)
        for other in ("b", "f"):
            assert np.array_equal(x, np.load(tmp_path / other / n), equal_nan=True), (n, other)
    assert np.load(tmp_path / "a" / "demodulated.npy").shape == (64, 1024)
