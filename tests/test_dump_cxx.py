"""examples/dump_cxx.cpp: a drizzling 2-D box through the C++ host mirror with the particle dump (include/lcx_dump.h) -- the droplets above
25 um in the lowest two levels are handed over with n, x, z, rw2 and cell, and the example prints their count and the sum of n r^3 over them
beside the same quantity from diag_wet_rng + diag_wet_mom(3) over the cells of those levels.

The bound of the comparison.  Both sums are of the same N non-negative terms n r^3.  The dump's side forms each in double on the host
(pow(rw2, 1.5), within an ulp or two of the device's) and adds them in storage order; the moment is an ordered device sum per cell, scaled
by 1 / (dv rhod) and scaled back by the example, and the cells are added on the host.  A sum of N terms in any order is within
(N - 1) eps of the exact sum relative to the sum of the magnitudes, each term's own rounding and the scalings add a few eps more: the two
agree to (N + 8) eps of the sum of the terms' magnitudes, which for non-negative terms is the sum itself."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "dump_cxx")


def test_cxx_dump_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "dump_cxx"])
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cxx_dump_example_checks_itself():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "dump_cxx"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    lines = out.strip().splitlines()
    assert len(lines) == 2, out
    w = lines[0].split()
    assert w[0] == "dumped" and w[2] == "of" and w[4] == "stride" and w[6] == "in_levels", out
    N, Q, stride, in_levels = int(w[1]), int(w[3]), int(w[5]), int(w[7])
    assert N > 0 and N == Q and stride == 1 and in_levels == 1, out
    v = lines[1].split()
    assert v[0] == "sum_n_r3" and v[1] == "dump" and v[3] == "diag", out
    s_dump, s_diag = float(v[2]), float(v[4])
    print(out, "difference", s_dump - s_diag, "bound", (N + 8) * np.finfo(np.float64).eps * s_dump)
    assert s_dump > 0 and abs(s_dump - s_diag) <= (N + 8) * np.finfo(np.float64).eps * s_dump, out
