"""The surface of the batched diagnostics (include/lcx_diag.h) without a GPU: which libraries export it, that lcx.h stays the surface
the oracle mirrors, the ctypes structs against the header's layout, lcx_diag_batch_check on the translated lists of
tests/test_oracle_diagnostics.py and on malformed ones, the translation of the `calls` notation there and back, and
libcloudphxx_amd/csrc/lcx_diag_plan.hpp alone under the host sanitizers."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _harness as h
import test_oracle_diagnostics as D
from libcloudphxx_amd import lgrngn, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["lcx_diag_batch", "lcx_diag_batch_check", "lcx_diag_batch_info"]


def header_entries(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lcx_[a-z0-9_A-Z]+)\s*\(", src)))


def hip_lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def expressible(calls):
    return [c for c in calls if lgrngn.diag_batch_expressible(c)]


def test_the_header_declares_the_three_entries_and_lcx_h_none_of_them():
    assert header_entries("lcx_diag.h") == ENTRIES
    assert not [s for s in header_entries("lcx.h") if s.startswith("lcx_diag_batch")]
    assert "diag_batch" not in open(os.path.join(ROOT, "include", "lcx.h")).read()


def test_the_hip_library_exports_them_and_no_oracle_build_does():
    lib = hip_lib()
    assert not [s for s in ENTRIES if not hasattr(lib, s)]
    h.oracle_lib()                                         # (builds every flavour)
    builds = sorted(glob.glob(os.path.join(h.ORACLE_DIR, "liblcx_oracle*.so")))
    assert len(builds) >= 4, builds
    for so in builds:
        orc = C.CDLL(so)
        for s in ENTRIES:
            assert not hasattr(orc, s) and not hasattr(orc, "orc_" + s[4:]), (so, s)


def test_ctypes_structs_have_the_headers_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lcx_diag.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(lcx_diag_clause_t), offsetof(lcx_diag_clause_t, sel),\n'
                   '  offsetof(lcx_diag_clause_t, lo), offsetof(lcx_diag_clause_t, hi), sizeof(lcx_diag_req_t), offsetof(lcx_diag_req_t, n_clauses),\n'
                   '  offsetof(lcx_diag_req_t, clause), offsetof(lcx_diag_req_t, count), offsetof(lcx_diag_req_t, k), LCX_DIAG_MAX_CLAUSES,\n'
                   '  LCX_DIAG_SEL_WATER, LCX_DIAG_KAPPA_MOM); return 0; }\n')
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True, capture_output=True, text=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    cl, rq = lgrngn._diag_clause_c, lgrngn._diag_req_c
    want = [C.sizeof(cl), cl.sel.offset, cl.lo.offset, cl.hi.offset, C.sizeof(rq), rq.n_clauses.offset, rq.clause.offset, rq.count.offset,
            rq.k.offset, lgrngn.DIAG_MAX_CLAUSES, lgrngn._DIAG_SEL["water"], lgrngn._DIAG_MOM["kappa"]]
    assert got == want, (got, want)
    assert sorted(lgrngn._DIAG_SEL.values()) == [0, 1, 2, 3, 4] and sorted(lgrngn._DIAG_MOM.values()) == [1, 2, 3]


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
def test_the_expressible_part_of_the_standard_calls(real_t):
    sub = expressible(D.standard_calls(real_t))
    assert len(sub) == (26 if real_t is np.float64 else 25)
    for z in (False, True):
        left = [c for c in D.standard_calls(real_t, z) if c not in expressible(D.standard_calls(real_t, z))]
        assert {c[1][0] for c in left} <= {"mom", "sd_conc", "precip_rate", "wet_mass_dens", "max_rw", "pressure", "temperature", "RH", "vel_div"}
        assert all(c[1][0] not in ("mom", "sd_conc") or c[0][0][0] in ("RH_ge_Sc", "rw_ge_rc") for c in left), left
    case_c = D.case_C(real_t)
    assert expressible(case_c.calls) == case_c.calls and len(case_c.calls) == 14


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
def test_check_accepts_the_translated_standard_calls_and_the_translation_round_trips(real_t):
    hip_lib()
    sub = expressible(D.standard_calls(real_t)) + D.case_C(real_t).calls
    lgrngn.diag_batch_check(sub)
    arr = lgrngn.diag_batch_requests(sub)
    back = lgrngn.diag_batch_calls(arr, len(sub))
    norm = lambda calls: [([tuple(s) for s in sel], tuple(cnt)) for sel, cnt in calls]
    assert norm(back) == norm(sub)
    # what the classic notation can say and the batch cannot is refused by the translation, each by its index
    for bad in [([("rng", "wet", 0., 1., True)], ("sd_conc",)),                                    # a chain that starts with _cons
                ([("all",), ("rng", "wet", 0., 1., False)], ("sd_conc",)),                         # a second selection that starts anew
                ([("all",), ("all",)], ("sd_conc",)), ([], ("sd_conc",)), ([("all",)] * 5, ("sd_conc",)),
                ([("RH_ge_Sc",)], ("sd_conc",)), ([("all",)], ("precip_rate",)), ([("all",)], ("mom", "incloud_time", 1))]:
        assert not lgrngn.diag_batch_expressible(bad)
        with pytest.raises(ValueError, match="request 1"):
            lgrngn.diag_batch_requests([sub[0], bad])


def test_check_names_each_malformed_request():
    lib = hip_lib()
    lib.lcx_last_error.restype = C.c_char_p
    good = expressible(D.standard_calls(np.float64))

    def refused(mutate, n=None):
        arr = lgrngn.diag_batch_requests(good)
        mutate(arr)
        assert lib.lcx_diag_batch_check(arr, C.c_int(len(good) if n is None else n)) == 1
        text = lib.lcx_last_error().decode()
        assert text.startswith("libcloudph++: diag_batch: "), text
        return text

    def setter(i, field, v, clause=None):
        def f(arr):
            setattr(arr[i] if clause is None else arr[i].clause[clause], field, v)
        return f

    assert "request 3: n_clauses = 0" in refused(setter(3, "n_clauses", 0))
    assert "request 7: n_clauses = 5" in refused(setter(7, "n_clauses", 5))
    assert "request 0: clause 0: unknown sel 5" in refused(setter(0, "sel", 5, 0))
    assert "request 2: clause 0: unknown sel -1" in refused(setter(2, "sel", -1, 0))
    # (request 13 is the first with three clauses; a bad enumerator behind n_clauses is not looked at)
    assert len(good[13][0]) == 3
    assert "request 13: clause 2: unknown sel 9" in refused(setter(13, "sel", 9, 2))
    arr = lgrngn.diag_batch_requests(good)
    arr[0].clause[3].sel = 9
    assert len(good[0][0]) == 1 and lib.lcx_diag_batch_check(arr, C.c_int(len(good))) == 0
    assert "request 5: unknown count 4" in refused(setter(5, "count", 4))       # (the classic counts beyond the moments: by enumerator range)
    assert "request 5: unknown count -1" in refused(setter(5, "count", -1))
    assert "n_req < 0" in refused(lambda arr: None, n=-1)
    assert lib.lcx_diag_batch_check(None, C.c_int(0)) == 0
    assert lib.lcx_diag_batch_check(None, C.c_int(2)) == 1 and "req == NULL" in lib.lcx_last_error().decode()
    with pytest.raises(RuntimeError, match="unknown count 4"):
        arr = lgrngn.diag_batch_requests(good)
        arr[1].count = 4
        lgrngn.diag_batch_check((arr, len(good)))


def test_the_plan_header_alone_under_the_host_sanitizers(tmp_path):
    """tools/diag_batch_plan_check.cpp: validation over malformed lists, the pass size over cell counts up to 2^58 and the planner over
    lists of up to 20000 random requests, built with -fsanitize=address,undefined.  Host code, run as a child process."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "diag_batch_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tools", "diag_batch_plan_check.cpp")], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr


def test_the_plan_header_has_no_hip_include():
    src = open(os.path.join(ROOT, "libcloudphxx_amd", "csrc", "lcx_diag_plan.hpp")).read()
    assert "#include <hip" not in src and "__global__" not in src and "__device__" not in src
