"""examples/coal_rates_cxx.cpp: a drizzling 2-D box through the C++ host mirror with the collision rates on (include/lcx_coal_rates.h) --
the example prints the domain's autoconversion and accretion mass rates per step."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "coal_rates_cxx")


def test_cxx_coal_rates_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "coal_rates_cxx"])
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cxx_coal_rates_example_prints_the_rates():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "coal_rates_cxx"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    lines = out.strip().splitlines()
    assert len(lines) == 9 and lines[-1].split() == ["outbuf_after_reset", "0.0"], out
    steps = []
    for i, ln in enumerate(lines[:-1]):
        w = ln.split()
        assert w[0] == "step" and int(w[1]) == i + 1, out
        steps.append({w[k]: float(w[k + 1]) for k in range(2, len(w) - 1, 2)})
    for s in steps:
        assert set(s) == {"acnv_kg_per_s", "accr_kg_per_s", "acnv_droplets", "accr_droplets", "self_cloud", "self_rain"}, out
        assert all(v >= 0 for v in s.values()), out
        assert (s["acnv_kg_per_s"] > 0) == (s["acnv_droplets"] > 0) and (s["accr_kg_per_s"] > 0) == (s["accr_droplets"] > 0), out
    assert sum(s["self_cloud"] + s["acnv_droplets"] + s["accr_droplets"] for s in steps) > 0, out      # (the box does collide)
