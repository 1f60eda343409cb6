"""The surface of the condensation rates (include/lcx_cond_rates.h) without a GPU: the header's entries and enumerators, that lcx.h and the
other companion headers stay what they were, which libraries export the entries, the Python mirror's argument checks, and the long-double
reference of the GPU tests (tests/_cond_rates_reference.py) on a case worked by hand."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import _harness as h
import _cond_rates_reference as CD
from libcloudphxx_amd import lgrngn, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lcx_cond_rates_disable", "lcx_cond_rates_enable", "lcx_cond_rates_info", "lcx_cond_rates_read", "lcx_diag_cond_rate"]
LD = np.longdouble


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def hip_lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def test_the_header_declares_the_five_entries_and_the_other_headers_none_of_them():
    assert sorted(set(re.findall(r"\b(lcx_[a-z0-9_A-Z]+)\s*\(", header("lcx_cond_rates.h")))) == ENTRIES
    for other in ("lcx.h", "lcx_state.h", "lcx_diag.h", "lcx_coal_rates.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "cond_rate" not in text and "LCX_CDR" not in text, other


def test_the_python_names_follow_the_headers_enumerators():
    enum = re.search(r"enum\s*\{([^}]*LCX_CDR_PER_THR[^}]*)\}", header("lcx_cond_rates.h")).group(1)
    names = [e.strip() for e in enum.split(",")]
    assert names[-1] == "LCX_CDR_PER_THR" and len(names) == 6
    assert tuple(n[len("LCX_CDR_"):].lower() for n in names[:-1]) == lgrngn.COND_RATES == CD.NAMES
    assert int(re.search(r"LCX_CDR_MAX_THR\s*=\s*(\d+)", header("lcx_cond_rates.h")).group(1)) == lgrngn.COND_RATES_MAX_THR == 4
    mirror = open(os.path.join(ROOT, "include", "libcloudph++", "lgrngn", "particles.hpp")).read()
    for n in names:
        assert "%s = %s" % (n[len("LCX_CDR_"):].lower(), n) in mirror, n


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


def test_thresholds_from_a_scalar_or_a_sequence():
    assert lgrngn.cond_rates_thresholds(25e-6) == [25e-6]
    assert lgrngn.cond_rates_thresholds(np.float32(1)) == [1.]
    assert lgrngn.cond_rates_thresholds((1e-6, 1.5e-6, 25e-6)) == [1e-6, 1.5e-6, 25e-6]
    assert lgrngn.cond_rates_thresholds(np.array([1., 2., 3., 4.])) == [1., 2., 3., 4.]
    for bad in ([], [1., 2., 3., 4., 5.]):
        with pytest.raises(ValueError, match=r"cond_rates: n_thr = %d is outside 1 \.\. 4" % len(bad)):
            lgrngn.cond_rates_thresholds(bad)
    for bad in (0, -25e-6, float("nan"), float("inf"), [1e-6, float("inf")], [0., 1.]):
        with pytest.raises(ValueError, match="cond_rates: every threshold must be positive and finite"):
            lgrngn.cond_rates_thresholds(bad)
    for bad in ([2e-6, 1e-6], [1e-6, 1e-6], [1e-6, 2e-6, 2e-6]):
        with pytest.raises(ValueError, match="cond_rates: the thresholds must be strictly increasing"):
            lgrngn.cond_rates_thresholds(bad)


def test_row_names_and_numbers():
    for k in (1, 3, 4):
        assert [lgrngn.cond_rate_index(nm, t, k) for t in range(k) for nm in lgrngn.COND_RATES] == list(range(5 * k))
        assert lgrngn.cond_rate_index("total_dm3", 0, k) == lgrngn.cond_rate_index("TOTAL_DM3", 2, k) == 5 * k
        assert lgrngn.cond_rate_index(5 * k, 0, k) == 5 * k and lgrngn.cond_rate_index(np.int64(0), 0, k) == 0
        for bad in (-1, 5 * k + 1):
            with pytest.raises(ValueError, match=r"cond_rates: row = %d is outside 0 \.\. %d" % (bad, 5 * k)):
                lgrngn.cond_rate_index(bad, 0, k)
        for bad in (-1, k):
            with pytest.raises(ValueError, match=r"cond_rates: t = %d is outside 0 \.\. %d" % (bad, k - 1)):
                lgrngn.cond_rate_index("up_n", bad, k)
    assert lgrngn.cond_rate_index("UP_M3", 1, 3) == 7
    for bad in ("up", "", "up_n "):
        with pytest.raises(ValueError, match="cond_rates: unknown row"):
            lgrngn.cond_rate_index(bad)


def test_output_arrays_are_checked_before_the_library_sees_them():
    ok = np.zeros((16, 30))
    assert lgrngn.cond_rates_out(ok, 3, 30) == (ok.ctypes.data, 30, False)
    wide = np.zeros((6, 40))
    assert lgrngn.cond_rates_out(wide[:, :30], 1, 30) == (wide.ctypes.data, 40, False)
    dev = lgrngn.DeviceArray(4096, (21, 30), (64, 1))
    assert lgrngn.cond_rates_out(dev, 4, 30) == (4096, 64, True)
    for bad, text in ((np.zeros((15, 30)), "must be 2-D"), (np.zeros((16, 31)), "must be 2-D"), (np.zeros(480), "must be 2-D"),
                      (np.zeros((16, 30), dtype=np.float32), "float64"), (np.zeros((30, 16)).T, "unit stride along cells"),
                      (np.zeros((16, 60))[:, ::2], "unit stride along cells"), (lgrngn.DeviceArray(4096, (16, 30), (16, 1)), "row stride")):
        with pytest.raises(ValueError, match=text):
            lgrngn.cond_rates_out(bad, 3, 30)
    frozen = np.zeros((16, 30))
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="unsupported strides"):
        lgrngn.cond_rates_out(frozen, 3, 30)


def test_the_reference_on_a_case_worked_by_hand():
    """three droplets of one cell (cell 1 of 2), two thresholds at r = 2 and r = 4 (lo = 4 and 16): radii 1 -> 3 (up through the first),
    5 -> 3 (down through the second, staying above the first), 5 -> 6 (staying above both); a dead slot and a below -> below droplet add
    nothing to the thresholds' rows"""
    n = np.array([10, 3, 2, 0, 7], dtype=np.uint64)
    ijk = np.array([1, 1, 1, 1, 0])
    rw2_0 = np.array([1., 25., 25., 1., .25])
    rw2_1 = np.array([9., 9., 36., 100., 1.])
    rows = CD.tally(n, ijk, rw2_0, rw2_1, CD.bounds([2., 4.], np.float64), 2)
    want = {0: {CD.ABOVE_DM3: 3 * (27 - 125) + 2 * (216 - 125), CD.UP_N: 10, CD.UP_M3: 10 * 27, CD.DOWN_N: 0, CD.DOWN_M3: 0},
            1: {CD.ABOVE_DM3: 2 * (216 - 125), CD.UP_N: 0, CD.UP_M3: 0, CD.DOWN_N: 3, CD.DOWN_M3: 3 * 125}}
    for t in (0, 1):
        for w, v in want[t].items():
            assert rows.value(5 * t + w, 1) == v, (t, w)
            assert rows.value(5 * t + w, 0) == 0, (t, w)
            assert isinstance(rows.value(5 * t + w, 1), int) == (w in CD.NUMBER)
    assert rows.value(10, 1) == 10 * 26 + 3 * (27 - 125) + 2 * (216 - 125) and rows.value(10, 0) == LD(7) * (1 - LD(.125))
    assert rows.count(10, 1) == 3 and rows.weight(10, 1) == 10 * 28 + 3 * 152 + 2 * 341
    assert rows.count(0, 1) == 2 and rows.count(2, 1) == 1 and rows.count(9, 1) == 1 and rows.weight(9, 1) == 3 * 152
    assert rows.up.tolist() == [[0, 1], [0, 0]] and rows.down.tolist() == [[0, 0], [0, 1]]
    assert CD.m3_bar(rows, 10, 1) == 11 * LD(2.) ** -52 * 1418
    # budgets of the header: N and M3 of "above t" from the state itself
    for t, lo in enumerate((4., 16.)):
        live = (n > 0) & (ijk == 1)
        N = lambda x: int(n[live & (x >= lo)].sum())
        M = lambda x: float((n * x ** 1.5)[live & (x >= lo)].sum())
        assert N(rw2_1) - N(rw2_0) == rows.value(5 * t + CD.UP_N, 1) - rows.value(5 * t + CD.DOWN_N, 1)
        assert M(rw2_1) - M(rw2_0) == rows.value(5 * t, 1) + rows.value(5 * t + CD.UP_M3, 1) - rows.value(5 * t + CD.DOWN_M3, 1)
