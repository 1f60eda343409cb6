"""examples/coal_log_cxx.cpp: a drizzling 2-D box through the C++ host mirror with the collision log (include/lcx_coal_log.h) and the
collision rates on at 25 um -- the example prints the events of every step and the autoconversion counts from both."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "coal_log_cxx")


def test_cxx_coal_log_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "coal_log_cxx"])
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cxx_coal_log_example_counts_autoconversion_as_the_rates_do():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "coal_log_cxx"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    lines = out.strip().splitlines()
    assert len(lines) == 9 and lines[-1].split() == ["launches", "8", "held_after_reset", "0"], out
    steps = []
    for i, ln in enumerate(lines[:-1]):
        w = ln.split()
        assert w[0] == "step" and int(w[1]) == i + 1, out
        steps.append({w[k]: float(w[k + 1]) for k in range(2, len(w) - 1, 2)})
    for s in steps:
        assert set(s) == {"events", "seen", "acnv_nr_log", "acnv_nr_rates", "acnv_nc_log", "acnv_nc_rates", "largest_product_um"}, out
        assert s["events"] == s["seen"] <= 64 * 30 / 2, out
        assert s["acnv_nr_log"] == s["acnv_nr_rates"] and s["acnv_nc_log"] == s["acnv_nc_rates"], out
        assert (s["events"] > 0) == (s["largest_product_um"] > 0), out
    assert sum(s["events"] for s in steps) > 0, out                     # (the box does collide)
