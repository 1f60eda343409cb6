"""examples/relax_cxx.cpp: aerosol relaxation through the C++ host mirror (factory<double>, opts_init.rlx_switch, rlx_dry_distros, opts.rlx),
the 2 x 2 set-up of the reference's tests/python/unit/relax.py with its bars (relax.py:127-142)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "relax_cxx")


@pytest.mark.gpu
def test_cxx_relaxation_example_runs():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    v = [float(x) for x in out.split()]
    assert len(v) == 6, out
    assert 1424 <= v[0] <= 1624 and 1424 <= v[2] <= 1624 and v[1] == 1024 and v[3] == 1024, out
    assert abs(v[4] - 1.5) <= 0.01 and abs(v[5] - 1.5) <= 0.01, out
