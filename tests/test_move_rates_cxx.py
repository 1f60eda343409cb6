"""examples/move_rates_cxx.cpp: a drizzling 2-D box in a sinking, drifting flow through the C++ host mirror with the move rates on
(include/lcx_move_rates.h) beside the condensation and collision rates -- the example prints per step the precipitation map's sum beside
the puddle's increase, and one cell's change of the number of rain drops beside the sum of the three tallies' terms."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "move_rates_cxx")
KEYS = {"precip_n", "puddle_n", "precip_vol", "puddle_vol", "rain_in", "rain_out", "drops_tallied", "drops_seen"}


def test_cxx_move_rates_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "move_rates_cxx"])
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cxx_move_rates_example_prints_closures_that_close():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "move_rates_cxx"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    lines = out.strip().splitlines()
    assert len(lines) == 9 and lines[-1].split() == ["moves_tallied_since_reset", "0"], out
    steps = []
    for i, ln in enumerate(lines[:-1]):
        w = ln.split()
        assert w[0] == "step" and int(w[1]) == i + 1, out
        steps.append({w[k]: float(w[k + 1]) for k in range(2, len(w) - 1, 2)})
    fallen = 0.
    for s in steps:
        assert set(s) == KEYS, out
        assert s["precip_n"] == s["puddle_n"], out                      # integers below 2^53 on both sides
        # the puddle's volume is a running total in double whose increase is taken here; its terms are pow(rw2, 3/2), the tally's x sqrt(x)
        fallen += s["puddle_vol"]
        assert abs(s["precip_vol"] - s["puddle_vol"]) <= 1e-12 * fallen + 1e-30, out
        # the classic moment is a sum in double of up to 64 droplets' n / (dv rhod), scaled back: integers to its rounding
        assert abs(s["drops_tallied"] - s["drops_seen"]) <= .5 + 1e-12 * abs(s["drops_seen"]), out
    assert sum(s["precip_n"] for s in steps) > 0, out                   # (the box does rain onto the ground)
    assert sum(s["rain_in"] for s in steps) > 0 and sum(s["rain_out"] for s in steps) > 0, out          # (and rain crosses the cell's faces)
