"""The integer rules of tracked super-droplets (csrc/lcx_track_plan.hpp) where they need no device: the stride rule of a selection, the
sample buffer's offsets and the validation of a selection's arguments, in a program of their own under the host sanitizers
(tools/track_plan_check.cpp).  The kernels k_track_assign and k_track_sample apply the very same functions per lane."""
import os
import subprocess

import _harness as h  # noqa: F401  (as in every test module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_track_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """stride and count for Q in {0, 1, room - 1, room, room + 1, 2 room + 1, 2^32 - 1} at rooms from 1 to LCX_TRK_MAX, each against a walk
    over the ranks (the ranks taken get consecutive indices, never more than room of them, and one stride less would take too many); the
    buffer's offsets against a plain [capacity][12][max_tracked] array, every element hit once; every text of the validation.  The header
    has no HIP include: the host compiler alone, -fsanitize=address,undefined.  Host code, a child process."""
    cxx = os.environ.get("CXX", "c++")
    exe = str(tmp_path / "track_plan_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "track_plan_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
