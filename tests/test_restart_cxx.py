"""examples/restart_cxx.cpp: stop a run and continue it through the C++ host mirror (snapshot() / restore(), include/lcx_state.h) -- the
parcel of parcel_cxx.cpp, 20 steps, the blob through a file into a new object, 20 more steps, beside an uninterrupted 40."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "restart_cxx")


@pytest.mark.gpu
def test_cxx_restart_example_prints_the_same_line_twice(tmp_path):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    out = subprocess.check_output([EXE, str(tmp_path / "parcel.snapshot")],
                                  env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    lines = out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("final rv ") and " wet_mom3 " in lines[0], out
    assert lines[0] == lines[1], out
    rv, m3 = float(lines[0].split()[2]), float(lines[0].split()[4])
    assert 0 < rv < 0.02 and m3 > 0, out          # (the parcel did condense: rv fell from its initial 0.02)
