"""The surface of the collision rates (include/lcx_coal_rates.h) without a GPU: the header's entries and enumerators, that lcx.h and
lcx_opts_init_t stay the surface the oracle mirrors, which libraries export the entries, and the Python mirror's argument checks."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lcx_coal_rates_disable", "lcx_coal_rates_enable", "lcx_coal_rates_info", "lcx_coal_rates_read", "lcx_diag_coal_rate"]


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def hip_lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def test_the_header_declares_the_five_entries_and_lcx_h_none_of_them():
    assert sorted(set(re.findall(r"\b(lcx_[a-z0-9_A-Z]+)\s*\(", header("lcx_coal_rates.h")))) == ENTRIES
    for other in ("lcx.h", "lcx_state.h", "lcx_diag.h"):
        assert "coal_rate" not in header(other), other
    assert "coal_rate" not in open(os.path.join(ROOT, "include", "lcx.h")).read()


def test_the_python_names_follow_the_headers_enumerators():
    enum = re.search(r"enum\s*\{([^}]*LCX_CR_COUNT[^}]*)\}", header("lcx_coal_rates.h")).group(1)
    names = [e.strip() for e in enum.split(",")]
    assert names[-1] == "LCX_CR_COUNT" and len(names) == 8
    assert tuple(n[len("LCX_CR_"):].lower() for n in names[:-1]) == lgrngn.COAL_RATES
    mirror = open(os.path.join(ROOT, "include", "libcloudph++", "lgrngn", "particles.hpp")).read()
    for n in names[:-1]:
        assert "%s = %s" % (n[len("LCX_CR_"):].lower(), n) in mirror, n


def test_the_hip_library_exports_them_and_no_oracle_build_does():
    lib = hip_lib()
    assert not [s for s in ENTRIES if not hasattr(lib, s)]
    h.oracle_lib()
    builds = sorted(glob.glob(os.path.join(h.ORACLE_DIR, "liblcx_oracle*.so")))
    assert len(builds) >= 4, builds
    for so in builds:
        orc = C.CDLL(so)
        for s in ENTRIES:
            assert not hasattr(orc, s) and not hasattr(orc, "orc_" + s[4:]), (so, s)


def test_accumulator_names_and_numbers():
    assert [lgrngn.coal_rate_index(nm) for nm in lgrngn.COAL_RATES] == list(range(7))
    assert lgrngn.coal_rate_index("ACCR_M3") == 3 and lgrngn.coal_rate_index(6) == 6 and lgrngn.coal_rate_index(np.int64(0)) == 0
    for bad in ("acnv", "", "accr_m3 "):
        with pytest.raises(ValueError, match="unknown accumulator"):
            lgrngn.coal_rate_index(bad)
    for bad in (-1, 7):
        with pytest.raises(ValueError, match="which = %d is outside 0 .. 6" % bad):
            lgrngn.coal_rate_index(bad)


def test_the_threshold_must_be_positive_and_finite():
    assert lgrngn.coal_rates_threshold(25e-6) == 25e-6 and lgrngn.coal_rates_threshold(np.float32(1)) == 1.
    for bad in (0, -25e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="r_thr must be positive and finite"):
            lgrngn.coal_rates_threshold(bad)


def test_output_arrays_are_checked_before_the_library_sees_them():
    ok = np.zeros((7, 30))
    assert lgrngn.coal_rates_out(ok, 30) == (ok.ctypes.data, 30, False)
    wide = np.zeros((7, 40))
    assert lgrngn.coal_rates_out(wide[:, :30], 30) == (wide.ctypes.data, 40, False)
    dev = lgrngn.DeviceArray(4096, (7, 30), (64, 1))
    assert lgrngn.coal_rates_out(dev, 30) == (4096, 64, True)
    for bad, text in ((np.zeros((6, 30)), "must be 2-D"), (np.zeros((7, 31)), "must be 2-D"), (np.zeros(210), "must be 2-D"),
                      (np.zeros((7, 30), dtype=np.float32), "float64"), (np.zeros((30, 7)).T, "unit stride along cells"),
                      (np.zeros((7, 60))[:, ::2], "unit stride along cells"), (lgrngn.DeviceArray(4096, (7, 30), (16, 1)), "row stride")):
        with pytest.raises(ValueError, match=text):
            lgrngn.coal_rates_out(bad, 30)
    frozen = np.zeros((7, 30))
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="unsupported strides"):
        lgrngn.coal_rates_out(frozen, 30)
