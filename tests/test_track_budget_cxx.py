"""examples/track_budget_cxx.cpp: the drizzling 2-D box of track_cxx.cpp through the C++ host mirror with the budget of tracked droplets
(include/lcx_track_budget.h) -- after six steps the example prints, for the first marked droplet that is still alive, its radius, the
shares of its r^3 growth that came from condensation and from collection, and its number of collisions."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "track_budget_cxx")


def test_cxx_track_budget_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "track_budget_cxx"])
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cxx_track_budget_example_prints_where_the_water_came_from():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "track_budget_cxx"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    lines = [ln.split() for ln in out.strip().splitlines()]
    assert len(lines) == 5, out
    assert lines[0][0] == "selected" and 1 <= int(lines[0][1]) <= 32, out
    assert lines[1] == ["samples", "6", "cond_passes", "6", "coal_passes", "6"], out
    assert lines[2][0::2] == ["index", "r_um", "r_um_from_budget"] and 0 <= int(lines[2][1]) < int(lines[0][1]), out
    r, r_closed = float(lines[2][3]), float(lines[2][5])
    assert r >= 10. and abs(r - r_closed) <= 1e-9 * r + 1e-9, "the radius of the last sample, and the first sample's plus the budget's growth: " + out
    assert lines[3][0::2] == ["dr3_um3", "from_condensation", "collected"], out
    dr3, cond, coal = (float(v) for v in lines[3][1::2])
    assert all(math.isfinite(v) for v in (dr3, cond, coal)) and dr3 != 0 and abs(cond + coal - 1) <= 1e-9, out
    assert lines[4][0::2] == ["collisions", "gains", "gives"], out
    events, gains, gives = (float(v) for v in lines[4][1::2])
    assert events == int(events) >= 0 and events == gains + gives <= 6, out
