"""examples/diag_batch_cxx.cpp: the reference driver's loop over spectrum bins (diag_*_rng, diag_*_mom, outbuf() per bin and moment)
beside one diag_batch() call of the C++ host mirror (include/lcx_diag.h) -- the example prints how many values agree bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "diag_batch_cxx")


def test_cxx_diag_batch_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "diag_batch_cxx"])
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cxx_diag_batch_example_reports_agreement():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "diag_batch_cxx"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    w = out.split()
    assert w[0] == "diag_batch", out
    v = {w[i]: int(w[i + 1]) for i in range(1, len(w) - 1, 2)}
    assert v["requests"] == 72 and v["cells"] == 30 and v["per_pass"] == 32, out
    assert v["values"] == 72 * 30 and v["identical"] == v["values"], out
    assert v["nonzero"] > 30 * 10, out                     # (the spectra are not empty: more than the sd_conc row and a few bins)
