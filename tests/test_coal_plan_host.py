"""The host side of the coalescence's launch (csrc/lcx_coal_plan.hpp) where it needs no device: which form the launch takes, the two pause
rules and their countdowns, the list's threshold and the key of the draws made ahead, in a program of their own under the host sanitizers
(tools/coal_plan_check.cpp)."""
import os
import subprocess

import _harness as h  # noqa: F401  (as in every test module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_coal_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """coal_form_of over every combination of its inputs against the rules of DESIGN.md 4.2, each on its own; what every debug toggle
    forces; COAL_SKIP_PAUSE paused steps and COAL_EXIT_PAUSE launches out of the EXIT form behind counters just under their thresholds,
    none behind counters exactly on them; the list at 6 % and one cell above; each member of the prevote's key differing alone.  The header
    has no HIP include: the host compiler alone, -fsanitize=address,undefined.  Host code, a child process."""
    cxx = os.environ.get("CXX", "c++")
    exe = str(tmp_path / "coal_plan_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "coal_plan_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
