"""examples/source_cxx.cpp: the aerosol source through the C++ host mirror (factory<double>, opts_init.src_type, opts.src_dry_distros),
the 2 x 2 set-up of the reference's tests/python/unit/source.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "source_cxx")


@pytest.mark.gpu
def test_cxx_source_example_runs():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    assert out.split() == ["2048", "1024", "2048", "1024"], out
