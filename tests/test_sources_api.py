"""CPU-side checks of how the aerosol source travels through the interfaces (no device needed): the two option structs of
include/lcx.h as the Python mirror fills them, lcx_opts_default, the C++ example's build, and that the CPU oracle -- which has no
source and is not the checker of this feature -- goes on refusing it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the struct prefix that lcx_opts_t had before the source fields were added behind it: 15 ints, padding, two doubles
_PREFIX_FIELDS = [(k, C.c_int) for k in ("adve", "sedi", "subs", "cond", "coal", "src", "rlx", "rcyc", "turb_adve", "turb_cond", "turb_coal",
                                         "ice_nucl", "chem_dsl", "chem_dsc", "chem_rct")] + [("RH_max", C.c_double), ("dt", C.c_double)]


class _opts_prefix_c(C.Structure):
    _fields_ = _PREFIX_FIELDS


def _prefix_bytes(c):
    return bytes((C.c_char * C.sizeof(_opts_prefix_c)).from_buffer_copy(bytes(c)[:C.sizeof(_opts_prefix_c)]))


def test_empty_source_dictionaries_give_null_pointers_and_the_old_prefix():
    o = lgrngn.opts_t()
    o.sedi, o.rcyc, o.RH_max, o.dt = False, True, 1.01, 0.5
    c = o._to_c()
    assert not c.src_dry_distros and not c.src_dry_sizes
    assert c.n_src_dry_distros == 0 and c.n_src_dry_sizes == 0
    # the leading bytes are what a struct without the new fields holds for the same settings
    old = _opts_prefix_c()
    for name, ctype in _PREFIX_FIELDS:
        v = getattr(o, name)
        setattr(old, name, float(v) if ctype is C.c_double else int(bool(v)))
    assert _prefix_bytes(c) == bytes(old)
    assert [f[0] for f in lgrngn._opts_c._fields_[:len(_PREFIX_FIELDS)]] == [f[0] for f in _PREFIX_FIELDS]
    assert C.sizeof(lgrngn._opts_c) == C.sizeof(_opts_prefix_c) + 2 * (C.sizeof(C.c_void_p) + 8)


def test_source_dictionaries_are_marshalled_sorted():
    """the reference's Python shapes (tests/python/unit/source.py:104,158)"""
    o = lgrngn.opts_t()
    o.src = True
    fn = h.lognormal_fn(.05e-6, 1.4, 60e4)
    o.src_dry_distros = {(.61, 0.): (fn, 512, 50)}
    o.src_dry_sizes = {(.8, 0.): {2e-6: [.2, 3, 7]}, (.61, 0.): {15e-6: [.1, 5, 50], 1e-6: [.3, 10, 40]}}
    c = o._to_c()
    assert c.src == 1 and c.n_src_dry_distros == 1 and c.n_src_dry_sizes == 3
    d = c.src_dry_distros[0]
    assert (d.distro.kappa, d.distro.rd_insol, d.sd_conc, d.supstp) == (.61, 0., 512, 50)
    assert d.distro.fn(-16., None) == fn(-16.)                 # the callback is alive and is the user's function
    got = [(s.kappa, s.rd_insol, s.radius, s.conc_per_s, s.sd_count, s.supstp) for s in (c.src_dry_sizes[i] for i in range(3))]
    assert got == [(.61, 0., 1e-6, .3, 10, 40), (.61, 0., 15e-6, .1, 5, 50), (.8, 0., 2e-6, .2, 3, 7)]
    # a built-in lognormal goes natively (no callback)
    o.src_dry_distros = {(.61, 0.): (lgrngn.lognormal(.05e-6, 1.4, 60e4), 64, 2)}
    c = o._to_c()
    d = c.src_dry_distros[0]
    assert not d.distro.fn and d.distro.n_modes == 1 and d.distro.mean_rd[0] == .05e-6 and d.distro.n_stp[0] == 60e4
    assert (d.sd_conc, d.supstp) == (64, 2)


def test_source_box_round_trips_through_opts_init():
    oi = lgrngn.opts_init_t()
    oi.src_type = lgrngn.src_t.matching
    oi.src_x0, oi.src_y0, oi.src_z0, oi.src_x1, oi.src_y1, oi.src_z1 = 1., 2., 3., 4., 5., 6.
    keep = []
    c = oi._to_c(keep)
    assert c.src_type == 2
    assert (c.src_x0, c.src_y0, c.src_z0, c.src_x1, c.src_y1, c.src_z1) == (1., 2., 3., 4., 5., 6.)
    c0 = lgrngn.opts_init_t()._to_c(keep)
    assert (c0.src_x0, c0.src_y0, c0.src_z0, c0.src_x1, c0.src_y1, c0.src_z1) == (0.,) * 6 and c0.src_type == 0


def _product_lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def test_opts_default_nulls_the_source_fields():
    lib = _product_lib()
    c = lgrngn._opts_c()
    C.memset(C.byref(c), 0xff, C.sizeof(c))
    lib.lcx_opts_default(C.byref(c))
    assert not c.src_dry_distros and not c.src_dry_sizes and c.n_src_dry_distros == 0 and c.n_src_dry_sizes == 0
    assert c.src == 0 and c.adve == 1 and c.dt == -1
    ci = lgrngn._opts_init_c()
    C.memset(C.byref(ci), 0xff, C.sizeof(ci))
    lib.lcx_opts_init_default(C.byref(ci))
    assert (ci.src_x0, ci.src_y0, ci.src_z0, ci.src_x1, ci.src_y1, ci.src_z1) == (0.,) * 6 and ci.src_type == 0


def test_python_structs_have_the_size_the_library_was_compiled_with():
    """lcx_opts_init_default clears sizeof(lcx_opts_init_t) bytes: a guard page of 0xff behind the mirror's struct must survive, and the
    mirror's last field must be cleared (so the two layouts end at the same place)"""
    lib = _product_lib()
    for ctype, fn in ((lgrngn._opts_init_c, lib.lcx_opts_init_default), (lgrngn._opts_c, lib.lcx_opts_default)):
        n = C.sizeof(ctype)
        buf = (C.c_ubyte * (n + 64))(*([0xff] * (n + 64)))
        fn(C.byref(buf))
        assert all(b == 0xff for b in buf[n:]), ctype
        assert all(b == 0 for b in buf[n - 4:n]), ctype


def test_source_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    assert os.path.exists(os.path.join(ROOT, "examples", "source_cxx"))


def test_the_oracle_still_refuses_sources():
    """the oracle has no source: it must say so instead of running without one"""
    for src_type in (lgrngn.src_t.simple, lgrngn.src_t.matching):
        oi = lgrngn.opts_init_t()
        oi.nx = oi.nz = 2
        oi.x1 = oi.z1 = 2.
        oi.dt, oi.sd_conc, oi.n_sd_max = 1., 8, 64
        oi.dry_distros = {(.61, 0.): h.lognormal_fn(.02e-6, 1.4, 60e6)}
        oi.src_type = src_type
        with pytest.raises(RuntimeError):
            h.oracle_particles(oi)


def test_spmd_path_points_to_the_multi_device_object():
    from libcloudphxx_amd import multi
    oi = lgrngn.opts_init_t()
    oi.nx, oi.x1, oi.src_type = 4, 4., lgrngn.src_t.simple
    with pytest.raises(RuntimeError, match="use the multi-device object"):
        multi.distmem_opts(oi, 0, 2)
