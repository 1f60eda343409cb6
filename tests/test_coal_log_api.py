"""The surface of the collision log (include/lcx_coal_log.h) without a GPU: the header's entries and enumerators, that lcx.h stays the
surface the oracle mirrors, which libraries export the entries, the texts of lcx_coal_log_check, and the Python mirror's refusals
before any call."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lcx_coal_log_check", "lcx_coal_log_disable", "lcx_coal_log_enable", "lcx_coal_log_info", "lcx_coal_log_read"]
MAX_CAPACITY = (2 ** 64 - 1) // (8 * 14)


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def hip_lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def test_the_header_declares_the_five_entries_and_lcx_h_none_of_them():
    assert sorted(set(re.findall(r"\b(lcx_[a-z0-9_A-Z]+)\s*\(", header("lcx_coal_log.h")))) == ENTRIES
    for other in ("lcx.h", "lcx_state.h", "lcx_diag.h", "lcx_coal_rates.h", "lcx_dump.h"):
        assert "coal_log" not in open(os.path.join(ROOT, "include", other)).read(), other


def test_the_python_names_follow_the_headers_enumerators():
    enum = re.search(r"enum\s*\{([^}]*LCX_CLG_FIELDS[^}]*)\}", header("lcx_coal_log.h")).group(1)
    names = [e.strip() for e in enum.split(",")]
    assert names[-1] == "LCX_CLG_FIELDS" and len(names) == 15
    assert tuple(n[len("LCX_CLG_"):].lower() for n in names[:-1]) == lgrngn.COAL_LOG_FIELDS
    assert lgrngn.COAL_LOG_FIELDS == ("launch", "cell", "slot_d", "slot_r", "col_no", "n_d", "n_r", "rw2_d", "rw2_r", "rw2_new", "rd3_d", "rd3_r",
                                      "vt_d", "vt_r")
    mirror = open(os.path.join(ROOT, "include", "libcloudph++", "lgrngn", "particles.hpp")).read()
    for n in names[:-1]:
        assert "%s = %s" % (n[len("LCX_CLG_"):].lower(), n) in mirror, n


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


def test_every_text_of_the_check_function():
    lib = hip_lib()
    for cap, r in ((1, 0.), (5, 25e-6), (2 ** 40, 1e-3), (MAX_CAPACITY, 0.)):
        lgrngn.coal_log_check(cap, r, lib=lib)
    with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: coal_log: capacity == 0$"):
        lgrngn.coal_log_check(0, 0., lib=lib)
    for cap in (MAX_CAPACITY + 1, 2 ** 64 - 1):
        with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: coal_log: capacity = %d: a list of 14 rows has more bytes than size_t holds$" % cap):
            lgrngn.coal_log_check(cap, 0., lib=lib)
    for r in (-1e-300, -25e-6, float("-inf"), float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: coal_log: r_min must be non-negative and finite$"):
            lgrngn.coal_log_check(8, r, lib=lib)


def test_the_wrapper_refuses_bad_arguments_before_any_call():
    assert lgrngn.coal_log_args(5) == (5, 0.) and lgrngn.coal_log_args(np.int64(7), np.float32(1)) == (7, 1.)
    assert lgrngn.coal_log_args(MAX_CAPACITY, 25e-6) == (MAX_CAPACITY, 25e-6)
    with pytest.raises(ValueError, match="coal_log: capacity == 0"):
        lgrngn.coal_log_args(0)
    for bad in (1.5, 2., True, -1, MAX_CAPACITY + 1):
        with pytest.raises(ValueError, match="coal_log: capacity"):
            lgrngn.coal_log_args(bad)
    for bad in (-25e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="coal_log: r_min must be non-negative and finite"):
            lgrngn.coal_log_args(8, bad)

    class NoCalls:                                                      # (a particles_t whose library must not be reached)
        _h = None

        def _f(self, name):
            raise AssertionError("the library was called: " + name)
    prt = NoCalls()
    for bad in ((0, 0.), (8, -1.), (1.5, 0.)):
        with pytest.raises(ValueError, match="coal_log"):
            lgrngn.particles_t.coal_log_enable(prt, *bad)
    for bad in (np.zeros((14, 8)), lgrngn.DeviceArray(4096, (13, 8), (8, 1)), lgrngn.DeviceArray(4096, (14, 8), (4, 1)),
                lgrngn.DeviceArray(4096, (14, 8), (16, 2)), lgrngn.DeviceArray(4096, (112,), (1,))):
        with pytest.raises(ValueError, match="coal_log: out"):
            lgrngn.particles_t.coal_log(prt, out=bad)
    assert lgrngn.coal_log_check_out(lgrngn.DeviceArray(4096, (14, 8), (16, 1))) == (8, 16)
