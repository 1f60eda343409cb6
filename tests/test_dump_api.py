"""The particle dump (include/lcx_dump.h) where no device is needed: the exported symbols, the enumerators, lcx_dump_check, and the Python
mirror's refusal of bad arguments before any call."""
import ctypes as C
import glob
import os
import re

import pytest

import _harness as h
from libcloudphxx_amd import _lib, lgrngn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_declares_the_two_entries_and_no_other_header_names_them():
    text = header("lcx_dump.h")
    assert re.findall(r"^int (lcx_dump\w*)\(", text, re.M) == ["lcx_dump_check", "lcx_dump"]
    assert sorted(set(re.findall(r"\blcx_dump\w*(?=\()", text))) == ["lcx_dump", "lcx_dump_check"], "declared exactly the two"
    others = [p for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "lcx_dump.h"]
    assert len(others) >= 10 and os.path.join(ROOT, "include", "lcx.h") in others
    for p in others:
        assert "lcx_dump" not in open(p).read(), os.path.basename(p) + ": lcx.h is the surface that the CPU oracle mirrors, the companions keep to their own"


def test_the_library_exports_both_and_the_oracle_neither():
    lib = _lib.load()
    assert hasattr(lib, "lcx_dump") and hasattr(lib, "lcx_dump_check")
    orc = h.oracle_lib()
    for pre in ("lcx_", "orc_"):
        for s in ("dump", "dump_check"):
            assert not hasattr(orc, pre + s), pre + s


def test_the_field_names_follow_the_enumerators():
    text = header("lcx_dump.h")
    enum = re.search(r"enum \{ (LCX_DMP_N,.*?) \};", text, re.S).group(1)
    enum = re.sub(r"/\*.*?\*/", " ", enum, flags=re.S)
    names = [w.strip() for w in enum.replace("\n", " ").split(",")]
    assert names[-1] == "LCX_DMP_FIELDS" and len(names) == 24
    assert tuple(n[len("LCX_DMP_"):].lower() for n in names[:-1]) == tuple(f.lower() for f in lgrngn.DUMP_FIELDS)
    assert lgrngn.DUMP_FIELDS[:12] == lgrngn.TRACK_FIELDS and len(set(f.lower() for f in lgrngn.DUMP_FIELDS)) == 23
    trk = re.search(r"enum \{ (LCX_TRK_N,.*?) \};", header("lcx_track.h"), re.S).group(1)
    trk = [w.strip()[len("LCX_TRK_"):] for w in trk.replace("\n", " ").split(",")][:-1]
    assert [n[len("LCX_DMP_"):] for n in names[:12]] == trk, "the twelve of LCX_TRK_*, in their order"
    assert lgrngn.DUMP_FIELDS[12:] == ("slot", "track", "incloud_time", "chem_hno3", "chem_nh3", "chem_co2", "chem_so2", "chem_h2o2", "chem_o3",
                                       "chem_s_vi", "chem_h")
    cxx = open(os.path.join(ROOT, "include", "libcloudph++", "lgrngn", "particles.hpp")).read()
    m = re.search(r"enum dump_field_t\s*\{(.*?)\};", cxx, re.S)
    pairs = [tuple(p.strip() for p in w.split("=")) for w in m.group(1).split(",") if w.strip()]
    assert [a.lower() for a, _ in pairs] == ["dmp_" + f.lower() for f in lgrngn.DUMP_FIELDS] + ["dmp_fields"]
    assert all(b == "LCX_DMP_" + a[len("dmp_"):].upper() for a, b in pairs), "each enumerator is its C twin"


def test_lcx_dump_check_accepts_and_refuses_what_the_header_says():
    lib = _lib.load()
    lib.lcx_last_error.restype = C.c_char_p
    clauses = (lgrngn._diag_clause_c * 5)()
    for i, sel in enumerate((0, 1, 2, 3, 4)):
        clauses[i].sel, clauses[i].lo, clauses[i].hi = sel, 1e-6, 2e-6
    box = lambda *v: (C.c_double * 6)(*v)
    ints = lambda *v: (C.c_int * len(v))(*v)
    i32 = C.c_int
    every = ints(*range(23))
    ok = lambda *a: lib.lcx_dump_check(*a)
    assert ok(clauses, i32(1), None, ints(0), i32(1)) == 0
    assert ok(clauses, i32(4), box(0, 1, 0, 1, 0, 1), every, i32(23)) == 0, "without an object the optional fields are taken as given"
    assert ok(clauses, i32(1), box(0, 0, 5, 5, -1, -1), ints(22, 3, 12), i32(3)) == 0, "lo == hi is an empty box, not a fault; any order of fields"
    refusals = [
        ((clauses, i32(0), None, every, i32(1)), "libcloudph++: dump: n_clauses = 0 is outside 1 .. 4"),
        ((clauses, i32(5), None, every, i32(1)), "libcloudph++: dump: n_clauses = 5 is outside 1 .. 4"),
        ((None, i32(1), None, every, i32(1)), "libcloudph++: dump: clause == NULL"),
        ((clauses, i32(1), box(0, 1, 2, 1, 0, 1), every, i32(1)), "libcloudph++: dump: box: lo > hi in pair 1"),
        ((clauses, i32(1), box(0, 1, 0, 1, 0, float("inf")), every, i32(1)), "libcloudph++: dump: box: bound 5 is not finite"),
        ((clauses, i32(1), box(float("nan"), 1, 0, 1, 0, 1), every, i32(1)), "libcloudph++: dump: box: bound 0 is not finite"),
        ((clauses, i32(1), None, every, i32(0)), "libcloudph++: dump: n_fields = 0 is outside 1 .. 23"),
        ((clauses, i32(1), None, every, i32(24)), "libcloudph++: dump: n_fields = 24 is outside 1 .. 23"),
        ((clauses, i32(1), None, None, i32(2)), "libcloudph++: dump: field == NULL"),
        ((clauses, i32(1), None, ints(0, 23), i32(2)), "libcloudph++: dump: field 1: unknown field 23"),
        ((clauses, i32(1), None, ints(-1), i32(1)), "libcloudph++: dump: field 0: unknown field -1"),
        ((clauses, i32(1), None, ints(4, 0, 4), i32(3)), "libcloudph++: dump: field 2: field 4 is given twice"),
    ]
    for args, text in refusals:
        assert ok(*args) == 1 and lib.lcx_last_error().decode() == text, text
    for bad in (-1, 5, 99):
        clauses[1].sel = bad
        assert ok(clauses, i32(2), None, every, i32(1)) == 1
        assert lib.lcx_last_error().decode() == "libcloudph++: dump: clause 1: unknown sel %d" % bad
    # the Python door to it
    lgrngn.dump_check()
    lgrngn.dump_check([("rng", "wet", 1e-6, 2e-6), ("water",)], box=(0, 1, 0, 1, 0, 1), fields=lgrngn.DUMP_FIELDS)
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: dump: box: lo > hi in pair 2"):
        lgrngn.dump_check([("all",)], box=(0, 1, 0, 1, 3, 1))
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: dump: field 1: field 0 is given twice"):
        lgrngn.dump_check(fields=("n", 0))
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: dump: field 0: unknown field 40"):
        lgrngn.dump_check(fields=(40,))


def test_the_wrapper_translates_the_field_names():
    arr, n, names = lgrngn.dump_fields(("n", "RW2", "chem_S_VI", "slot"))
    assert n == 4 and list(arr) == [0, 4, 21, 12] and names == ["n", "rw2", "chem_s_vi", "slot"]
    arr, n, names = lgrngn.dump_fields(("t", "rh", "RV"))
    assert list(arr) == [9, 10, 11] and names == ["T", "RH", "rv"], "the names of a track record as TRACK_FIELDS spells them"
    arr, n, names = lgrngn.dump_fields("track")
    assert n == 1 and list(arr) == [13]
    arr, n, names = lgrngn.dump_fields(lgrngn.DUMP_FIELDS)
    assert n == 23 and list(arr) == list(range(23))
    assert lgrngn.DUMP_DEFAULT_FIELDS == ("n", "x", "y", "z", "rw2", "rd3", "kappa")


class _NoCalls:
    """stands in for a particles_t whose library must not be reached"""
    _h = None

    def _f(self, name):
        raise AssertionError("the wrapper called lcx_%s with arguments it should have refused" % name)

    _chk = None
    _dump_call = None


DA = lgrngn.DeviceArray


@pytest.mark.parametrize("call, text", [
    (lambda p: lgrngn.particles_t.dump(p, fields=()), r"n_fields = 0 is outside 1 \.\. 23"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "radius")), "unknown field 'radius'"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "x", "N")), "field 'n' is given twice"),
    (lambda p: lgrngn.particles_t.dump(p, max_count=0), "max_count must be at least 1"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "x"), max_count=8, out=DA(0, (3, 8))), r"out must be a DeviceArray of shape \(n_fields, max_count\) = \(2, 8\)"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "x"), max_count=9, out=DA(0, (2, 8))), r"out must be a DeviceArray of shape \(n_fields, max_count\) = \(2, 9\)"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "x"), max_count=8, out=DA(0, (16,))), "out must be a DeviceArray of shape"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "x"), max_count=8, out=__import__("numpy").zeros((2, 8), dtype="float32")), "out must be a DeviceArray of shape"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "x"), max_count=8, out=__import__("numpy").zeros((2, 8))), "out must be a DeviceArray of shape"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "x"), max_count=8, out=DA(0, (2, 8), (8, 2))), "unit stride along the droplets"),
    (lambda p: lgrngn.particles_t.dump(p, fields=("n", "x"), max_count=8, out=DA(0, (2, 8), (4, 1))), "row stride is below max_count"),
    (lambda p: lgrngn.particles_t.dump(p, []), "track: n_clauses = 0"),
    (lambda p: lgrngn.particles_t.dump(p, [("rng", "wet", 1.)]), "track: cannot express clause 0"),
    (lambda p: lgrngn.particles_t.dump(p, box=(0, 1)), "track: box must hold six bounds"),
    (lambda p: lgrngn.particles_t.dump_count(p, box=(0, 1, 1, 0, 0, 1)), "track: box: lo > hi"),
])
def test_the_wrapper_refuses_bad_arguments_before_any_call(call, text):
    with pytest.raises(ValueError, match=r"libcloudph\+\+: (dump: )?.*" + text):
        call(_NoCalls())
