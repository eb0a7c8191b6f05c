"""The per-bin division of the in-wave spectrum as a guarded multiplication (kernels/spectrum_math.h: spec_div), against the division it replaces,
`(float)((double)q / rate)`, bit for bit -- on the CPU: the header is plain C++ and tests/cpp/spectrum_div_check.cpp is a program of its own.

Rates 32000, 156250, 39062.5, 512000 and 8000.  Inputs per rate: every float bit pattern at a stride of 1021 (4.2e6 patterns, both signs, NaNs and
infinities among them); every subnormal input of both signs and the normal floats next to them, +-0, +-Inf, a NaN, the largest float, the inputs whose
quotient lies at the ends of the subnormal floats with 2^16 consecutive inputs across the quotient 2^-126; and, for 1e6 random float results f, the float
nearest to (f + ulp/2) * rate with its two neighbours on each side -- quotients next to a float rounding midpoint, which is what the guard is about.

Those rates have few significant bits, and a 24-bit input over such a rate never comes within the guard's reach of a midpoint.  So the program also
makes rates for it: for 1e6 random pairs of an input and a midpoint, q / midpoint rounded to double and its two neighbours on each side -- quotients
within a few units of the last place of a midpoint, where the product alone rounds to the wrong float.  They must reach the guard and agree.

The division must stay rare: of the strided inputs that are positive normal floats with a normal float quotient (the range the spectrum's powers
live in) fewer than 1 in 1e4 may take it.  The guard's width predicts 9 in 2^29."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
RATES = (32000.0, 156250.0, 39062.5, 512000.0, 8000.0)


def test_spec_div_equals_the_division_bit_for_bit(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "spectrum_div_check"
    # (-ffp-contract=off: the product and the division are each rounded once, as on the device)
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "habdec_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "spectrum_div_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = re.findall(r"rate (\S+) checked (\d+) mismatches (\d+) normal (\d+) slow (\d+)", r.stdout)
    assert [float(x[0]) for x in rows] == list(RATES), r.stdout
    for rate, checked, mismatches, normal, slow in rows:
        checked, mismatches, normal, slow = int(checked), int(mismatches), int(normal), int(slow)
        print(f"rate {rate}: {checked} inputs, {mismatches} mismatches; strided normal range {normal}, of them through the division {slow}")
        assert checked >= 4_000_000 + 2 * (1 << 23) + 5_000_000, (rate, checked)
        assert mismatches == 0, (rate, mismatches, r.stderr)
        assert normal >= 1_000_000 and slow * 10_000 < normal, (rate, normal, slow)
    m = re.search(r"constructed checked (\d+) mismatches (\d+) slow (\d+)", r.stdout)
    assert m, r.stdout
    checked, mismatches, slow = map(int, m.groups())
    print(f"constructed rates: {checked} quotients next to a midpoint, {mismatches} mismatches, {slow} through the division")
    assert checked == 6_000_000 and mismatches == 0, (checked, mismatches, r.stderr)
    assert slow >= checked // 2, slow                              # (the guard is what these inputs are about: most of them must reach it)
