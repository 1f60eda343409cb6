"""The host side of the condensation's launches (csrc/lcx_cond_plan.hpp) where it needs no device: the kernel of a per-substep launch, the
route of a step_cond and who carries the scatter, dbg_cond_budget's five meanings, the launch sizes and the form of the per-cell finish,
in a program of their own under the host sanitizers (tools/cond_plan_check.cpp)."""
import os
import subprocess

import _harness as h  # noqa: F401  (as in every test module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cond_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """cond_kernel_of over every combination of the switches, strict, solver, turb_cond and kpa_uniform against the precedence rules, each on
    its own, exactly one form each; the rows of tests/test_hip_cond.py (what its objects must report); cond_route_of and carries_scatter
    over every combination of their inputs; cond_budget at 0, a negative value, 1, 2, 255, 256, 256 + 3, (4 << 8) | 3 and above FOLD_CAP;
    the launch sizes by hand at 0 .. 2^25 droplets; cond_finish_of with 4096 cells and 192 per cell from both sides.  The header has no
    HIP include: the host compiler alone, -fsanitize=address,undefined.  Host code, a child process."""
    cxx = os.environ.get("CXX", "c++")
    exe = str(tmp_path / "cond_plan_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "cond_plan_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
