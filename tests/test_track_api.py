"""Tracked super-droplets (include/lcx_track.h) where no device is needed: the exported symbols, the enumerators, lcx_track_check, and the
Python mirror's translation of clauses and refusal of bad arguments before any call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _harness as h  # noqa: F401  (as in every test module)
from libcloudphxx_amd import _lib, lgrngn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("check", "enable", "disable", "select", "select_slots", "sample", "info", "read")


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_library_exports_the_eight_symbols_and_lcx_h_does_not_declare_them():
    lib = _lib.load()
    for s in SYMBOLS:
        assert hasattr(lib, "lcx_track_" + s), s
    text = header("lcx_track.h")
    declared = re.findall(r"^int (lcx_track_\w+)\(", text, re.M)
    assert declared == ["lcx_track_" + s for s in SYMBOLS]
    assert "lcx_track" not in header("lcx.h"), "lcx.h is the surface that the CPU oracle mirrors entry for entry"


def test_the_enumerators_follow_the_header():
    text = header("lcx_track.h")
    enum = re.search(r"enum \{ (LCX_TRK_N,.*?) \};", text, re.S).group(1)
    names = [w.strip() for w in enum.replace("\n", " ").split(",")]
    assert names[-1] == "LCX_TRK_FIELDS" and len(names) == 13
    assert [n[len("LCX_TRK_"):].lower() for n in names[:-1]] == [f.lower() for f in lgrngn.TRACK_FIELDS]
    assert lgrngn.TRACK_FIELDS == ("n", "x", "y", "z", "rw2", "rd3", "kappa", "vt", "cell", "T", "RH", "rv")
    assert re.search(r"LCX_TRK_MAX = 1 << 20", text) and lgrngn.TRACK_MAX == 1 << 20
    assert np.float32(lgrngn.TRACK_MAX) == lgrngn.TRACK_MAX and np.float32(lgrngn.TRACK_MAX - 1) == lgrngn.TRACK_MAX - 1, "marks are exact in float"
    cxx = open(os.path.join(ROOT, "include", "libcloudph++", "lgrngn", "particles.hpp")).read()
    m = re.search(r"enum track_field_t\s*\{(.*?)\};", cxx, re.S)
    pairs = [tuple(p.strip() for p in w.split("=")) for w in m.group(1).split(",") if w.strip()]
    assert [a for a, _ in pairs] == ["trk_" + f for f in lgrngn.TRACK_FIELDS] + ["trk_fields"]
    assert all(b == "LCX_TRK_" + a[len("trk_"):].upper() for a, b in pairs), "each enumerator is its C twin"


def test_lcx_track_check_accepts_and_refuses_what_the_header_says():
    lib = _lib.load()
    lib.lcx_last_error.restype = C.c_char_p
    clauses = (lgrngn._diag_clause_c * 5)()
    for i, sel in enumerate((0, 1, 2, 3, 4)):
        clauses[i].sel, clauses[i].lo, clauses[i].hi = sel, 1e-6, 2e-6
    box = lambda *v: (C.c_double * 6)(*v)
    ok = lambda *a: lib.lcx_track_check(*a)
    assert ok(clauses, C.c_int(1), None, C.c_size_t(1)) == 0
    assert ok(clauses, C.c_int(4), box(0, 1, 0, 1, 0, 1), C.c_size_t(1 << 40)) == 0
    assert ok(clauses, C.c_int(1), box(0, 0, 5, 5, -1, -1), C.c_size_t(1)) == 0, "lo == hi is an empty box, not a fault"
    refusals = [
        ((clauses, C.c_int(0), None, C.c_size_t(1)), "libcloudph++: track: n_clauses = 0 is outside 1 .. 4"),
        ((clauses, C.c_int(5), None, C.c_size_t(1)), "libcloudph++: track: n_clauses = 5 is outside 1 .. 4"),
        ((None, C.c_int(1), None, C.c_size_t(1)), "libcloudph++: track: clause == NULL"),
        ((clauses, C.c_int(1), None, C.c_size_t(0)), "libcloudph++: track: max_count == 0"),
        ((clauses, C.c_int(1), box(0, 1, 2, 1, 0, 1), C.c_size_t(1)), "libcloudph++: track: box: lo > hi in pair 1"),
        ((clauses, C.c_int(1), box(0, 1, 0, 1, 0, float("inf")), C.c_size_t(1)), "libcloudph++: track: box: bound 5 is not finite"),
        ((clauses, C.c_int(1), box(float("nan"), 1, 0, 1, 0, 1), C.c_size_t(1)), "libcloudph++: track: box: bound 0 is not finite"),
    ]
    for args, text in refusals:
        assert ok(*args) == 1 and lib.lcx_last_error().decode() == text, text
    for bad in (-1, 5, 99):
        clauses[1].sel = bad
        assert ok(clauses, C.c_int(2), None, C.c_size_t(1)) == 1
        assert lib.lcx_last_error().decode() == "libcloudph++: track: clause 1: unknown sel %d" % bad
    # the Python door to it
    lgrngn.track_check([("all",)])
    lgrngn.track_check([("rng", "wet", 1e-6, 2e-6), ("water",)], box=(0, 1, 0, 1, 0, 1), max_count=3)
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: track: max_count == 0"):
        lgrngn.track_check([("all",)], max_count=0)
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: track: box: lo > hi in pair 2"):
        lgrngn.track_check([("all",)], box=(0, 1, 0, 1, 3, 1))


def test_the_wrapper_translates_the_clause_notation():
    arr, n = lgrngn.track_clauses([("all",), ("rng", "wet", 1e-6, 2e-6), ("rng", "dry", 3e-8, 4e-8, True), ("water",)])
    assert n == 4 and [arr[i].sel for i in range(4)] == [0, 2, 1, 4]
    assert (arr[1].lo, arr[1].hi, arr[2].lo, arr[2].hi) == (1e-6, 2e-6, 3e-8, 4e-8)
    arr, n = lgrngn.track_clauses([("rng", "kappa", .1, .7), ("water", True)])
    assert n == 2 and (arr[0].sel, arr[0].lo, arr[0].hi, arr[1].sel) == (3, .1, .7, 4)
    for bad in ([], [("all",)] * 5):
        with pytest.raises(ValueError, match=r"libcloudph\+\+: track: n_clauses = \d is outside 1 \.\. 4"):
            lgrngn.track_clauses(bad)
    for bad in ([("rng", "wet", 1e-6)], [("rng", "ice", 1e-6, 2e-6)], [("all", 1)], [("RH_ge_Sc",)], [()], [("water", 1, 2)]):
        with pytest.raises(ValueError, match=r"libcloudph\+\+: track: cannot express clause 0"):
            lgrngn.track_clauses(bad)
    assert lgrngn.track_box(None) is None
    assert list(lgrngn.track_box((0, 1, 2, 3, 4, 5))) == [0., 1., 2., 3., 4., 5.]
    assert list(lgrngn.track_box(np.array([[0, 1], [2, 3], [4, 5]]))) == [0., 1., 2., 3., 4., 5.]
    with pytest.raises(ValueError, match="six bounds"):
        lgrngn.track_box((0, 1, 2, 3))
    with pytest.raises(ValueError, match="must be finite"):
        lgrngn.track_box((0, 1, 2, 3, 4, float("nan")))
    with pytest.raises(ValueError, match="lo > hi"):
        lgrngn.track_box((1, 0, 2, 3, 4, 5))


class _NoCalls:
    """stands in for a particles_t whose library must not be reached"""
    _h = None

    def _f(self, name):
        raise AssertionError("the wrapper called lcx_%s with arguments it should have refused" % name)

    _chk = None
    track_info = None


@pytest.mark.parametrize("call, text", [
    (lambda p: lgrngn.particles_t.track_enable(p, 0), r"max_tracked = 0 is outside 1 \.\. 1048576"),
    (lambda p: lgrngn.particles_t.track_enable(p, (1 << 20) + 1), r"max_tracked = 1048577 is outside"),
    (lambda p: lgrngn.particles_t.track_enable(p, 8, capacity=0), "capacity must be at least 1"),
    (lambda p: lgrngn.particles_t.track_enable(p, 8, every=-1), r"every = -1 < 0"),
    (lambda p: lgrngn.particles_t.track_select(p, []), "n_clauses = 0"),
    (lambda p: lgrngn.particles_t.track_select(p, [("rng", "wet", 1.)]), "cannot express clause 0"),
    (lambda p: lgrngn.particles_t.track_select(p, box=(0, 1)), "six bounds"),
    (lambda p: lgrngn.particles_t.track_select(p, max_count=0), "max_count must be at least 1"),
    (lambda p: lgrngn.particles_t.track_select_slots(p, [0, -1]), "non-negative integers"),
    (lambda p: lgrngn.particles_t.track_select_slots(p, [0.5]), "non-negative integers"),
])
def test_the_wrapper_refuses_bad_arguments_before_any_call(call, text):
    with pytest.raises(ValueError, match=r"libcloudph\+\+: track: .*" + text):
        call(_NoCalls())
