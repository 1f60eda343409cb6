"""The budget of tracked super-droplets (include/lcx_track_budget.h) where no device is needed: the exported symbols, where they are
declared, the enumerators on the three sides, and the Python mirror's refusal of a bad `out` before any call."""
import os
import re
import subprocess

import pytest

import _harness as h  # noqa: F401  (as in every test module)
import _track_budget_reference as B
from libcloudphxx_amd import _lib, lgrngn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("enable", "disable", "info", "read")


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_library_exports_exactly_the_four_symbols():
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, "lcx_track_budget_" + s), s
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib._name]).decode()
    exported = sorted(w for ln in out.splitlines() for w in ln.split()[-1:] if w.startswith("lcx_track_budget"))
    assert exported == sorted("lcx_track_budget_" + s for s in SYMBOLS)


def test_the_header_of_its_own_declares_them():
    declared = re.findall(r"^int (lcx_track_budget_\w+)\(", header("lcx_track_budget.h"), re.M)
    assert declared == ["lcx_track_budget_" + s for s in SYMBOLS]
    assert "lcx_track_budget_" not in header("lcx.h") and "lcx_track" not in header("lcx.h")
    assert not re.findall(r"^int (lcx_track_budget_\w+)\(", header("lcx_track.h"), re.M) and "LCX_TRB_" not in header("lcx_track.h")
    assert "lcx_track_budget.h" in header("lcx_track.h"), "lcx_track.h points to the companion"


def test_the_enumerators_agree_on_the_three_sides():
    text = header("lcx_track_budget.h")
    enum = re.search(r"enum \{ (LCX_TRB_COND_DR3,.*?) \};", text, re.S).group(1)
    names = [w.strip() for w in enum.replace("\n", " ").split(",")]
    assert names == ["LCX_TRB_COND_DR3", "LCX_TRB_COAL_DR3", "LCX_TRB_COAL_DRD3", "LCX_TRB_CHEM_DRD3", "LCX_TRB_COAL_DN", "LCX_TRB_COAL_GAINS",
                     "LCX_TRB_COAL_GIVES", "LCX_TRB_FIELDS"]
    assert [n[len("LCX_TRB_"):].lower() for n in names[:-1]] == list(lgrngn.TRACK_BUDGET_FIELDS) == list(B.FIELDS)
    cxx = open(os.path.join(ROOT, "include", "libcloudph++", "lgrngn", "particles.hpp")).read()
    m = re.search(r"enum track_budget_field_t\s*\{(.*?)\};", cxx, re.S)
    pairs = [tuple(p.strip() for p in w.split("=")) for w in m.group(1).split(",") if w.strip()]
    assert [a for a, _ in pairs] == ["trb_" + f for f in lgrngn.TRACK_BUDGET_FIELDS] + ["trb_fields"]
    assert all(b == "LCX_TRB_" + a[len("trb_"):].upper() for a, b in pairs), "each enumerator is its C twin"


class _NoCalls:
    """stands in for a particles_t whose library must not be reached"""
    _h = None

    def _f(self, name):
        raise AssertionError("the wrapper called lcx_%s with arguments it should have refused" % name)

    _chk = None

    def track_info(self):
        return {"n_samples": 3, "n_tracked": 5}


@pytest.mark.parametrize("out, text", [
    (object(), r"out must be a DeviceArray of shape \(n_samples, 7, n_tracked\) = \(3, 7, 5\)"),
    (lgrngn.DeviceArray(0, (3, 7)), "out must be a DeviceArray of shape"),
    (lgrngn.DeviceArray(0, (3, 7, 6)), "out must be a DeviceArray of shape"),
    (lgrngn.DeviceArray(0, (3, 12, 5)), "out must be a DeviceArray of shape"),
    (lgrngn.DeviceArray(0, (3, 7, 5), (70, 10, 2)), "out must have unit stride along the droplets"),
])
def test_the_wrapper_refuses_a_bad_out_before_any_call(out, text):
    with pytest.raises(ValueError, match=r"libcloudph\+\+: track budget: " + text):
        lgrngn.particles_t.track_budget(_NoCalls(), out=out)
