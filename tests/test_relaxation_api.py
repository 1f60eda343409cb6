"""CPU-side checks of how aerosol relaxation travels through the interfaces (no device needed): the relaxation fields of
lcx_opts_init_t as the Python mirror fills them, lcx_opts_init_default, the host-only layout entry lcx_rlx_layout against a numpy
restatement of the reference's expressions (src/impl/sources_and_relaxation_of_SDs/particles_impl_rlx_dry_distros.ipp:100-147,186-187)
written here, the C++ example's build, and that the CPU oracle -- which has no relaxation and is not the checker of this feature --
goes on refusing it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT = (.02e-6, 1.4, 60e6)          # the reference's tests/python/unit/relax.py:17-31
RLX = (.02e-6, 1.4, 120e6)


def _product_lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(_lib.LIB_PATH)


def relax_py_opts(spectrum):
    """relax.py:41-63,104-112"""
    oi = lgrngn.opts_init_t()
    oi.nx = oi.nz = 2
    oi.dx = oi.dz = 1.
    oi.x1 = oi.z1 = 2.
    oi.dt = 1.
    oi.aerosol_independent_of_rhod = True
    oi.coal_switch = oi.sedi_switch = False
    oi.rlx_switch = True
    oi.dry_distros = {(.61, 0.): h.lognormal_fn(*INIT)}
    oi.rlx_dry_distros = {.61: [spectrum, [0, 2], [0, oi.dz]]}
    oi.sd_conc = 1024
    oi.rlx_bins, oi.rlx_timescale, oi.rlx_sd_per_bin, oi.supstp_rlx = 1024, 4, 1, 2
    oi.n_sd_max = 8192
    return oi


# ------------------------------------------------------------------ restatement of the reference's expressions (double)
def dist_analysis(fn, sd_conc, vol):
    """init_dist_analysis_sd_conc (initialization/particles_impl_init_dist_analysis.ipp:17-77): (ln rd_min, ln rd_max)"""
    rd_min, rd_max = 1e-14, 1e-3
    while True:
        mult = math.log(rd_max / rd_min) / sd_conc * 1. * vol
        lo, hi = math.log(rd_min), math.log(rd_max)
        n_min, n_max = int(fn(lo) * mult), int(fn(hi) * mult)
        if n_min == 0:
            rd_min *= 1.01
        elif n_max == 0:
            rd_max /= 1.01
        else:
            return lo, hi


def layout(fns, rlx_bins, vol):
    """rlx_dry_distros.ipp:100-138,186-187: per spectrum (edges in rd3, expected STP concentration per bin)"""
    rngs = [dist_analysis(fn, rlx_bins, vol) for fn in fns]
    tot = 0.
    for lo, hi in rngs:
        tot += hi - lo
    res = []
    for fn, (lo, hi) in zip(fns, rngs):
        n_bins = int(rlx_bins * (hi - lo) / tot)
        size = (hi - lo) / n_bins
        edges = np.array([math.exp(3 * (lo + float(b) * size)) for b in range(n_bins + 1)])
        conc = np.array([fn(lo + (b + 0.5) * size) * size for b in range(n_bins)])
        res.append((edges, conc))
    return res


# ------------------------------------------------------------------ marshalling
def test_relaxation_dictionary_is_marshalled_sorted_by_kappa():
    """the reference's Python shape {kappa: [fun, [kappa_min, kappa_max], [z_min, z_max]]} (relax.py:109, bindings/python/lgrngn.hpp:357-377)"""
    fn = h.lognormal_fn(*RLX)
    oi = relax_py_opts(fn)
    oi.rlx_dry_distros = {.8: [lgrngn.lognormal(.05e-6, 1.8, 50e6), [.7, .9], [10., 20.]], .61: [fn, [0, .7], [0, 1.5]]}
    keep = []
    c = oi._to_c(keep)
    assert c.rlx_switch == 1 and c.n_rlx_dry_distros == 2
    assert (c.rlx_bins, c.rlx_sd_per_bin, c.rlx_timescale, c.supstp_rlx) == (1024, 1., 4., 2)
    a, b = c.rlx_dry_distros[0], c.rlx_dry_distros[1]
    assert (a.distro.kappa, a.kappa_min, a.kappa_max, a.z_min, a.z_max) == (.61, 0., .7, 0., 1.5)
    assert (b.distro.kappa, b.kappa_min, b.kappa_max, b.z_min, b.z_max) == (.8, .7, .9, 10., 20.)
    assert a.distro.fn(-16., None) == fn(-16.)                  # the callback is alive and is the user's function
    # a built-in lognormal goes natively (no callback)
    assert not b.distro.fn and b.distro.n_modes == 1 and b.distro.mean_rd[0] == .05e-6 and b.distro.sdev[0] == 1.8 and b.distro.n_stp[0] == 50e6
    # nothing set: null pointer, zero count, the reference's defaults
    c0 = lgrngn.opts_init_t()._to_c(keep)
    assert not c0.rlx_dry_distros and c0.n_rlx_dry_distros == 0 and c0.rlx_switch == 0
    assert (c0.rlx_bins, c0.rlx_sd_per_bin, c0.rlx_timescale, c0.supstp_rlx) == (0, 0., 1., 1)


def test_opts_init_default_sets_the_reference_defaults():
    lib = _product_lib()
    ci = lgrngn._opts_init_c()
    C.memset(C.byref(ci), 0xff, C.sizeof(ci))
    lib.lcx_opts_init_default(C.byref(ci))
    assert (ci.rlx_bins, ci.rlx_sd_per_bin, ci.rlx_timescale, ci.supstp_rlx) == (0, 0., 1., 1)
    assert not ci.rlx_dry_distros and ci.n_rlx_dry_distros == 0 and ci.rlx_switch == 0
    # the mirror ends where the library's struct ends
    n = C.sizeof(lgrngn._opts_init_c)
    buf = (C.c_ubyte * (n + 64))(*([0xff] * (n + 64)))
    lib.lcx_opts_init_default(C.byref(buf))
    assert all(b == 0xff for b in buf[n:]) and all(b == 0 for b in buf[n - 4:n])


# ------------------------------------------------------------------ lcx_rlx_layout
def ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


@pytest.mark.parametrize("builtin", [True, False])
def test_layout_of_the_reference_test_spectrum(builtin):
    """relax.py's spectrum, rlx_bins = 1024, one spectrum: edges to the last bit (the same expression; math.exp and std::exp are the
    same libm routine), bin-centre concentrations to 1e-14 relative"""
    fn = h.lognormal_fn(*RLX)
    oi = relax_py_opts(lgrngn.lognormal(*RLX) if builtin else fn)
    edges, conc = lgrngn.rlx_layout(oi, 0, lib=_product_lib())
    (e_ref, c_ref), = layout([fn], 1024, 1.)
    assert len(conc) == len(c_ref) == 1024 and len(edges) == 1025
    print("largest edge difference in ulp:", ulps(edges, e_ref).max(), "largest relative difference of the concentrations:", np.abs(conc / c_ref - 1).max())
    assert np.array_equal(edges, e_ref)
    assert np.all(np.diff(edges) > 0)
    np.testing.assert_allclose(conc, c_ref, rtol=1e-14)
    # the bins hold the spectrum: 120e6 per unit volume at STP
    assert abs(conc.sum() / 120e6 - 1) < 1e-5


def test_layout_of_two_spectra_of_different_width():
    """the bins are shared in proportion to the ranges of ln rd: n_bins = int(rlx_bins * range / sum of ranges)"""
    f0, f1 = h.lognormal_fn(*RLX), h.lognormal_fn(.05e-6, 1.8, 50e6)
    oi = relax_py_opts(f0)
    oi.dx, oi.dz, oi.x1, oi.z1 = 50., 25., 100., 50.             # (the cell volume enters the spectrum analysis)
    oi.rlx_bins = 1000
    oi.rlx_dry_distros = {.8: [f1, [.7, 2], [0, 25.]], .61: [lgrngn.lognormal(*RLX), [0, .7], [0, 50.]]}
    ref = layout([f0, f1], 1000, 50. * 1. * 25.)
    n = []
    for s in (0, 1):
        edges, conc = lgrngn.rlx_layout(oi, s, lib=_product_lib())
        e_ref, c_ref = ref[s]
        n.append(len(conc))
        assert len(edges) == len(e_ref) and len(conc) == len(c_ref)
        assert np.array_equal(edges, e_ref)
        np.testing.assert_allclose(conc, c_ref, rtol=1e-14)
    print("bins of the two spectra:", n)
    assert n[1] > n[0] and 998 <= sum(n) <= 1000                # the wider spectrum gets more bins; int() drops at most one each


def _raises(text, make):
    with pytest.raises(RuntimeError) as e:
        make()
    assert text in str(e.value), str(e.value)


def test_layout_reports_the_option_errors():
    """the checks of the options need no device either"""
    lib = _product_lib()
    fn = lgrngn.lognormal(*RLX)

    def with_(**kw):
        oi = relax_py_opts(fn)
        for k, v in kw.items():
            setattr(oi, k, v)
        return lambda: lgrngn.rlx_layout(oi, 0, lib=lib)
    _raises("libcloudph++: rlx_bins <= 0", with_(rlx_bins=0))
    _raises("libcloudph++: rlx_sd_per_bin <= 0", with_(rlx_sd_per_bin=0.))
    _raises("libcloudph++: rlx_timescale <= 0", with_(rlx_timescale=0.))
    _raises("CCN relaxation works only in 2D and 3D", with_(nz=0))
    _raises("rlx_bins above 1024", with_(rlx_bins=1025))
    _raises("z_min > z_max", with_(rlx_dry_distros={.61: [fn, [0, 2], [1.5, 1.]]}))
    _raises("empty kappa range", with_(rlx_dry_distros={.61: [fn, [.7, .7], [0, 1.]]}))
    _raises("no such entry", lambda: lgrngn.rlx_layout(relax_py_opts(fn), 1, lib=lib))
    assert len(lgrngn.rlx_layout(relax_py_opts(fn), 0, lib=lib)[1]) == 1024


# ------------------------------------------------------------------ the neighbours of the feature
def test_the_oracle_still_refuses_relaxation():
    """the oracle has no relaxation: it must say so instead of running without it"""
    with pytest.raises(RuntimeError):
        h.oracle_particles(relax_py_opts(h.lognormal_fn(*RLX)))


def test_spmd_path_points_to_the_multi_device_object():
    from libcloudphxx_amd import multi
    oi = relax_py_opts(lgrngn.lognormal(*RLX))
    oi.nx, oi.x1 = 4, 4.
    with pytest.raises(RuntimeError, match="use the multi-device object"):
        multi.distmem_opts(oi, 0, 2)


def test_relaxation_example_builds():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    assert os.path.exists(os.path.join(ROOT, "examples", "relax_cxx"))
