"""The cells' vote ahead of the coalescence launch (csrc/lcx_coal_prevote.hpp) where it needs no device: the pieces that the host and both
kernels share -- a cell's smallest draw, the tiles a cell's stretch overlaps, the bound's NaN cases -- in a program of their own under the
host sanitizers (tools/coal_prevote_check.cpp)."""
import os
import subprocess

import _harness as h  # noqa: F401  (as in every test module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prevote_header_alone_under_the_host_sanitizers(tmp_path):
    """coal_cell_umin against a brute-force minimum of philox::u01 over the cell's pair positions, float and double, cells of 0, 1, 2, 3, 63,
    64, 65, 255 and 256 droplets at even and odd offsets, below, across and above 2^32 (the position travels as 64 bits); coal_cell_tiles for a
    cell inside a tile, ending on a boundary, straddling one, with its only pair at the odd position 512 k - 1, and empty.  The header
    includes lcx_math.hpp, which needs the HIP headers: compiled for the host only, -fsanitize=address,undefined.  Host code, a child process."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "coal_prevote_check")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "coal_prevote_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
