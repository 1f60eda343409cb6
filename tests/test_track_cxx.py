"""examples/track_cxx.cpp: a drizzling 2-D box through the C++ host mirror with tracked droplets (include/lcx_track.h) -- drizzle-sized
droplets near cloud base are marked after a spin-up, eight steps end in a sample each, and the example prints the first marked droplet's
radius, height and relative humidity per step until it reaches the ground."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "track_cxx")


def test_cxx_track_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "track_cxx"])
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cxx_track_example_prints_one_droplets_history():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s", "track_cxx"])
    out = subprocess.check_output([EXE], env=dict(os.environ, LCX_DATA_DIR=os.path.join(ROOT, "libcloudphxx_amd", "data"))).decode()
    lines = out.strip().splitlines()
    assert len(lines) == 10, out
    assert lines[0].split()[0] == "selected" and 1 <= int(lines[0].split()[1]) <= 8, out
    assert lines[-1].split() == ["samples", "8", "dropped", "0", "scans", lines[-1].split()[-1]] and int(lines[-1].split()[-1]) >= 1, out
    alive, z_before = True, None
    for i, ln in enumerate(lines[1:-1]):
        w = ln.split()
        assert w[0] == "step" and int(w[1]) == i + 1 and w[2] == "time" and float(w[3]) == 2. * (i + 1), out      # dt = 2, counted from enable
        if w[4] == "gone":
            assert i > 0, out                                               # (it was alive when it was selected, and one step does not take it to the ground)
            alive = False
            continue
        assert alive, "a droplet that has gone does not come back: " + out
        v = {w[k]: float(w[k + 1]) for k in range(4, len(w) - 1, 2)}
        assert set(v) == {"n", "r_um", "z", "cell", "RH"}, out
        assert v["n"] >= 1 and v["r_um"] >= 10. and 0. <= v["z"] < 40. and 0 <= v["cell"] < 16 and int(v["cell"]) % 4 == int(v["z"] // 10), out
        assert .9 < v["RH"] < 1.5, out
        if z_before is not None:
            assert v["z"] < z_before, "the air sinks and the droplet falls: " + out
        z_before = v["z"]
