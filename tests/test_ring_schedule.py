"""The tile schedule of the /32 worker waves (habdec_amd/csrc/host/ring_schedule.hpp) is a pure host header: tests/ring_schedule_main.cpp checks its
properties (every output covered, a chained tile's predecessor 64 rows before it in the same run and stream, no run across a stream boundary, no row
loaded past the push, the same tile count for every stream of a mode), the ticket space the kernel walks, and -- with a float32 emulation of the
systolic tap loop -- that sums carried across a tile boundary equal plain left-to-right sums bit for bit.  Compiled with the address and
undefined-behaviour sanitizers and run as a program of its own; no GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_ring_schedule_properties_and_handover_emulation(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ring_schedule_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    str(ROOT / "tests" / "ring_schedule_main.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
