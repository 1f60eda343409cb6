"""examples/cond_rates_cxx.cpp: a drizzling 2-D box through the C++ host mirror with the condensation rates and the collision rates on
(include/lcx_cond_rates.h, include/lcx_coal_rates.h) -- the example prints one cell's rain-water budget per step, term by term, beside the
change that diag_wet_rng + diag_wet_mom see."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "cond_rates_cxx")
KEYS = {"growth_kg", "up_kg", "down_kg", "acnv_kg", "accr_kg", "sum_kg", "seen_kg", "drops_tallied", "drops_seen"}


def test_cxx_cond_rates_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "cond_rates_cxx"])
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cxx_cond_rates_example_prints_a_budget_that_closes():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "cond_rates_cxx"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    lines = out.strip().splitlines()
    assert len(lines) == 9 and lines[-1].split() == ["outbuf_after_reset", "0.0"], out
    steps = []
    for i, ln in enumerate(lines[:-1]):
        w = ln.split()
        assert w[0] == "step" and int(w[1]) == i + 1, out
        steps.append({w[k]: float(w[k + 1]) for k in range(2, len(w) - 1, 2)})
    rain = 0.
    for s in steps:
        assert set(s) == KEYS, out
        assert all(s[k] >= 0 for k in ("up_kg", "down_kg", "acnv_kg", "accr_kg")), out
        # the classic moments are sums in double of 64 droplets' n r^3 / (dv rhod): the budget closes to their rounding
        rain += s["seen_kg"]
        assert abs(s["sum_kg"] - s["seen_kg"]) <= 1e-12 * max(abs(rain), abs(s["seen_kg"])) + 1e-30, out
        assert abs(s["drops_tallied"] - s["drops_seen"]) <= .5 + 1e-12 * abs(s["drops_seen"]), out
    assert rain > 0 and any(s["growth_kg"] != 0 for s in steps), out                                        # (the box does make rain)
