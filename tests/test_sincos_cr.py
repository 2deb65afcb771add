"""csrc/sincos_cr.hpp, the sin and cos of PTG_FLAG_REFERENCE_F64's plain
estimator, on the host (tests/sincos_check.cpp, built without FMA contraction
as the device code is): correctly rounded on every fifth of the angles
2 pi m 2^-24 a draw can give and on those next to the multiples of pi/2.  The
reference is the long double sinl / cosl, whose own error is below one unit
of its 64-bit mantissa, 2^-11 ulp of the double: a correctly rounded double is
within 1/2 + 2^-10 ulp of it.  How often the result differs from libm's double
sin / cos is printed and bounded by a tenth of the arguments (glibc's are
within 0.55 ulp, so they give anything but the correctly rounded value only
within 0.05 ulp of a rounding boundary): measured 25,128 and 24,782 of all
16,777,216 angles, 0.15 % each.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sincos_is_correctly_rounded(tmp_path):
    exe = tmp_path / "sincos_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "sincos_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe), "5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    w = r.stdout.split()
    max_ulp, ds, dc, n = float(w[1]), int(w[3]), int(w[5]), int(w[7])
    assert n == -(-(1 << 24) // 5) + 17
    assert max_ulp <= 0.5 + 2.0 ** -10
    assert ds <= n // 10 and dc <= n // 10
