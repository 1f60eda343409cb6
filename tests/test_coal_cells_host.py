"""One wave per kept cell (k_coal_cells) where it needs no device: what the kernel shares with the host through csrc/lcx_coal_prevote.hpp --
how the vote's list is shared out among the waves of a fixed grid, the grid's size, a cell's pairs and their positions -- in a program of its
own under the host sanitizers (tools/coal_cells_check.cpp)."""
import os
import subprocess

import _harness as h  # noqa: F401  (as in every test module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_shares_and_pairs_under_the_host_sanitizers(tmp_path):
    """coal_list_share_of: every entry below the count is taken by exactly one wave for lists of 0 to 36 000 entries on grids of 1 to 2048
    workgroups of one and four waves; coal_cells_grid: at least one workgroup, at most the cap; coal_cell_pairs / coal_pair_pos: cells of 0, 1,
    2, 3, 63, 64, 65, 129, 255, 256, 257 and 600 droplets at even and odd offsets below, across and above 2^32, every pair visited once by the
    kernel's windows, at an even in-cell offset, and the smallest of their draws the one coal_cell_umin gave the vote.  Compiled for the host
    only, -fsanitize=address,undefined.  Host code, a child process."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "coal_cells_check")
    b = subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tools", "coal_cells_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
