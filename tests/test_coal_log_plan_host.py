"""The host side of the collision log (csrc/lcx_coal_log_plan.hpp) where it needs no device: the validation that lcx_coal_log_check and
lcx_coal_log_enable share, the layout of the list and the rule of how many events are held and written, in a program of their own under
the host sanitizers (tools/coal_log_plan_check.cpp)."""
import os
import subprocess

import _harness as h  # noqa: F401  (as in every test module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_coal_log_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """every text of the validation, the rows and bytes of a capacity up to the largest that size_t holds, held = min(seen, capacity) and
    the room of a read around their edges.  The header has no HIP include: the host compiler alone, -fsanitize=address,undefined.  Host
    code, a child process."""
    cxx = os.environ.get("CXX", "c++")
    exe = str(tmp_path / "coal_log_plan_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "coal_log_plan_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
