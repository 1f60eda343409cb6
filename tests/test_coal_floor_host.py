"""The floor under the cell maxima of the coalescence bound (csrc/lcx_coal_prevote.hpp coal_cmax_floor) where it needs no device: a program
of its own under the host sanitizers (tools/coal_floor_check.cpp)."""
import os
import subprocess

import _harness as h  # noqa: F401  (as in every test module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_floor_header_alone_under_the_host_sanitizers(tmp_path):
    """Over time steps 0.01 .. 30 s, largest multiplicities 1 .. 1e19, cell volumes 1 .. 1e6 m^3, scale factors 1 .. 255 and eps 2^-16, 2^-13 and
    2^-6, float and double: coal_bound at the floor is <= eps, one grid step above it > eps, the floor never grows with n_max or dt, and
    (CMAX_FLOOR, CMAX_FLOOR) comes back where no radius qualifies, without a table and with eps = 0.  The vote's sub-lists: random length
    vectors with zeros, one sub-list holding everything, totals of 0, 1, 2 and 2^16 -- every index below the total maps to exactly one
    (sub-list, offset) with the offset below that sub-list's length, and over every grid of coal_cells_grid one wave takes it.  Compiled for the host only,
    -fsanitize=address,undefined.  Host code, a child process."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "coal_floor_check")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "coal_floor_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
