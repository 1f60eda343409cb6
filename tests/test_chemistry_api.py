"""CPU-side checks of the chemistry interface (no GPU): the entries of include/lcx_chem.h are exported with their declared signatures, the
species enums of the three mirrors agree with the header, the option struct carries chem_rho, and the one-process-per-GPU path refuses
chemistry like the reference's MPI build."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcx_chem.h")
ORDER = ["HNO3", "NH3", "CO2", "SO2", "H2O2", "O3", "S_VI", "H"]


def header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def declared():
    """name -> number of parameters, of every function the header declares"""
    out = {}
    for m in re.finditer(r"\bint\s+(lcx_[a-z_]+)\s*\(([^;]*?)\)\s*;", header(), flags=re.S):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    return out


def test_header_declares_the_chemistry_entries():
    d = declared()
    assert d == {"lcx_init_chem": 9, "lcx_sync_in_chem": 9, "lcx_step_cond_chem": 5, "lcx_step_sync_chem": 10, "lcx_diag_chem": 2}, d
    # each is the plain entry of lcx.h plus the six ambient arrays
    plain = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcx.h")).read(), flags=re.S)
    for name in ("init", "sync_in", "step_cond", "step_sync"):
        m = re.search(r"\bint\s+lcx_%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S)
        assert d["lcx_%s_chem" % name] == len(m.group(1).split(",")) + 1
        assert re.search(r"lcx_%s_chem\s*\([^;]*const\s+lcx_arrinfo_t\s*\*\s*ambient_chem\s*\[6\]\s*\)" % name, header(), flags=re.S)


def test_library_exports_the_chemistry_entries():
    from libcloudphxx_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in declared() if not hasattr(lib, s)]
    assert not missing, missing


def test_species_enums_equal_the_header():
    from libcloudphxx_amd import lgrngn
    m = re.search(r"enum\s+lcx_chem_species\s*\{(.*?)\}", header(), flags=re.S)
    names = [x.strip().split("=")[0].strip() for x in m.group(1).split(",")]
    assert names[:8] == ["LCX_CHEM_" + n for n in ORDER]
    for i, n in enumerate(ORDER):
        assert int(lgrngn.chem_species_t[n]) == i
    assert lgrngn.chem_gas_n == 6 and len(lgrngn.chem_species_t) == 8
    # the C++ mirror's enum and the puddle slots of lcx.h list the same order
    cxx = open(os.path.join(ROOT, "include", "libcloudph++", "common", "output.hpp")).read()
    assert re.search(r"enum chem_species_t \{ " + ", ".join(ORDER) + ",", cxx)
    lcx = open(os.path.join(ROOT, "include", "lcx.h")).read()
    assert re.search(r"LCX_OUT_HNO3 = 0, " + ", ".join("LCX_OUT_" + n for n in ORDER[1:]) + ",", re.sub(r"\s+", " ", lcx))
    assert lgrngn.output_names[:8] == ORDER


def test_option_struct_carries_chem_rho():
    from libcloudphxx_amd import lgrngn, _lib
    assert lgrngn._opts_init_c._fields_[-1] == ("chem_rho", ctypes.c_double)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcx.h")).read(), flags=re.S)
    assert re.search(r"double\s+chem_rho\s*;\s*\}\s*lcx_opts_init_t", hdr)
    oi = lgrngn.opts_init_t()
    oi.chem_switch, oi.chem_rho, oi.sstp_chem = True, 1.8e3, 3
    c = oi._to_c([])
    assert (c.chem_switch, c.chem_rho, c.sstp_chem) == (1, 1.8e3, 3)
    d = lgrngn._opts_init_c()
    f = _lib.load().lcx_opts_init_default
    f.restype = None
    f(ctypes.byref(d))
    assert (d.chem_switch, d.chem_rho, d.sstp_chem) == (0, 0., 1)


def test_python_mirror_takes_ambient_chem():
    import inspect
    from libcloudphxx_amd import lgrngn
    for name in ("init", "sync_in", "step_cond", "step_sync"):
        assert "ambient_chem" in inspect.signature(getattr(lgrngn.particles_t, name)).parameters
    assert callable(lgrngn.particles_t.diag_chem)


def test_one_process_per_gpu_path_refuses_chemistry():
    from libcloudphxx_amd import lgrngn, multi
    oi = lgrngn.opts_init_t()
    oi.nx, oi.x1, oi.dt, oi.sd_conc, oi.n_sd_max = 4, 4., 1, 8, 100
    multi.distmem_opts(oi, 0, 2)
    oi.chem_switch, oi.chem_rho = True, 1.8e3
    with pytest.raises(RuntimeError, match="chemistry is not compatible with MPI"):
        multi.distmem_opts(oi, 0, 2)
