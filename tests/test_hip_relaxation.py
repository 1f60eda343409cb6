"""Aerosol relaxation (opts_init.rlx_switch, rlx_dry_distros, opts.rlx) on the HIP path.

The CPU oracle has no relaxation, so the yardsticks are (a) the reference's own known answers (its tests/python/unit/relax.py),
restated here as numbers, and (b) numpy restatements of the reference's formulas
(src/impl/sources_and_relaxation_of_SDs/particles_impl_rlx_dry_distros.ipp), written in this file and fed with the state the library
reports BEFORE the firing step (state_u64 "n", "ijk", state_real "rd3", "kappa") and with the bin tables the object holds
("raw_rlx_edges", "raw_rlx_conc"; for an object in double they are lcx_rlx_layout's, which tests/test_relaxation_api.py holds to its
own restatement).  A super-droplet whose planned multiplicity rounds to zero is created and dropped by the step's post_copy like any
other super-droplet with n == 0, so the restated plan lists the entries with n > 0."""
import copy

import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

INIT = (.02e-6, 1.4, 60e6)          # relax.py:17-31
RLX = (.02e-6, 1.4, 120e6)
TOLERANCE = .1                      # src/detail/config.hpp:33


def spectrum(par, builtin):
    return lgrngn.lognormal(*par) if builtin else h.lognormal_fn(*par)


def rho_stp(real):
    r = real
    return r(101325) / r(273.15 + 15) / (r(8.3144621) / r(0.02897))          # p_stp / T_stp / R_d, each constant in real_t


def steps(p, opts, f, n, C=None):
    for _ in range(n):
        p.step_sync(opts, *f, **(C or {}))
        p.step_async(opts)


def cell_field(p, what, *a):
    p.diag_all()
    getattr(p, what)(*a)
    return p.outbuf_array().astype(np.float64)


def only_rlx():
    o = lgrngn.opts_t()
    o.adve = o.sedi = o.cond = o.coal = False
    o.rlx = True
    return o


def _raises(text, make):
    with pytest.raises(RuntimeError) as e:
        make()
    assert text in str(e.value), str(e.value)


# ------------------------------------------------------------------ restatement of the reference's formulas
def tables(p, oi):
    """per spectrum, in kappa order: the option entry and the object's own bin tables"""
    edges, conc = p.state_real("raw_rlx_edges"), p.state_real("raw_rlx_conc")
    res, e0, b0 = [], 0, 0
    for s, kappa in enumerate(sorted(oi.rlx_dry_distros)):
        nb = len(lgrngn.rlx_layout(oi, s)[1])
        _, kr, zr = oi.rlx_dry_distros[kappa]
        res.append(dict(kappa=kappa, kmin=kr[0], kmax=kr[1], zmin=zr[0], zmax=zr[1], edges=edges[e0:e0 + nb + 1], conc=conc[b0:b0 + nb]))
        e0, b0 = e0 + nb + 1, b0 + nb
    assert e0 == edges.size and b0 == conc.size
    return res


def census(oi, st, tab, real):
    """hor_sum[bin][level] of one spectrum: summed multiplicities of kappa_min <= kappa < kappa_max, edge[b] <= rd3 < edge[b+1]"""
    nb = tab["conc"].size
    hor = np.zeros((nb, oi.nz), dtype=np.uint64)
    kpa, rd3 = st["kappa"].astype(real), st["rd3"].astype(real)
    e = tab["edges"].astype(real)
    b = np.searchsorted(e, rd3, side="right") - 1                  # an rd3 ON an edge belongs to the upper bin
    sel = (kpa >= real(tab["kmin"])) & (kpa < real(tab["kmax"])) & (b >= 0) & (b < nb)
    np.add.at(hor, (b[sel], (st["ijk"][sel] % np.uint64(oi.nz)).astype(np.int64)), st["n"][sel])
    return hor


def plan_of(oi, tab, hor, real, rhod_col, dt, x_extent=None, spb=None):
    """rlx_dry_distros.ipp:186-258 for one spectrum, in real_t = real and in the reference's order of operations:
    [(kappa, level, bin, n)] of what is created (entries with n > 0), and the number created per (bin, level)"""
    r = real
    spb = r(oi.rlx_sd_per_bin if spb is None else spb)
    n_per_bin = max(1, int(spb + r(0.5)))
    dz, z0, z1 = r(oi.dz), r(oi.z0), r(oi.z1)
    xe = r(oi.x1) - r(oi.x0) if x_extent is None else r(x_extent[1]) - r(x_extent[0])
    frac = min(r(r(oi.supstp_rlx) * r(dt)) / r(oi.rlx_timescale), r(1))
    k_lo, k_hi = int(r(tab["zmin"]) / dz), min(int(r(tab["zmax"]) / dz), oi.nz)
    out, created = [], np.zeros(hor.shape, dtype=np.int64)
    for b in range(hor.shape[0]):
        conc = r(tab["conc"][b])
        for k in range(oi.nz):
            vol = max(r(0), xe * (r(oi.y1) - r(oi.y0)) * (min(r(k + 1) * dz, z1) - max(r(k) * dz, z0)))
            expected = conc * vol
            if not oi.aerosol_independent_of_rhod:
                expected = expected * r(rhod_col[k]) / rho_stp(r)
            if k < k_lo or k >= k_hi:
                expected = r(0)
            missing = max(expected - r(hor[b, k]), r(0))
            if expected > 0 and missing / expected > r(TOLERANCE):
                n = int(missing / spb * frac + r(0.5))
                created[b, k] = n_per_bin
                if n > 0:
                    out += [(tab["kappa"], k, b, n)] * n_per_bin
    return out, created


def whole_plan(p, oi, st, real, rhod_col, dt=None, **kw):
    out = []
    for tab in tables(p, oi):
        out += plan_of(oi, tab, census(oi, st, tab, real), real, rhod_col, oi.dt if dt is None else dt, **kw)[0]
    return sorted(out)


def state_of(p, names=("rd3", "kappa")):
    st = {k: p.state_real(k) for k in names}
    st.update(n=p.state_u64("n"), ijk=p.state_u64("ijk"))
    return st


def newcomers_as_plan(p, oi, new):
    """(kappa, level, bin, n) of every newcomer; its rd3 must lie inside a bin of the spectrum that carries its kappa"""
    by_kappa = {t["kappa"]: t for t in tables(p, oi)}
    out = []
    for kappa, ijk, rd3, n in zip(new["kappa"], new["ijk"], new["rd3"], new["n"]):
        t = by_kappa[[k for k in by_kappa if np.float32(k) == np.float32(kappa)][0]]
        b = int(np.searchsorted(t["edges"], rd3, side="right")) - 1
        assert 0 <= b < t["conc"].size and t["edges"][b] <= rd3 < t["edges"][b + 1]
        out.append((t["kappa"], int(ijk % oi.nz), b, int(n)))
    return sorted(out)


def float_layout(fns, rlx_bins, vol):
    """the layout (init_dist_analysis.ipp:17-77, rlx_dry_distros.ipp:100-138,186-187) restated in np.float32: per spectrum (edges, conc)"""
    import math
    r = np.float32
    rngs = []
    for fn in fns:
        rd_min, rd_max = r(1e-14), r(1e-3)
        while True:
            mult = r(r(math.log(rd_max / rd_min)) / r(rlx_bins) * r(1) * r(vol))
            lo, hi = r(math.log(rd_min)), r(math.log(rd_max))
            n_min, n_max = int(r(fn(float(lo))) * mult), int(r(fn(float(hi))) * mult)
            if n_min == 0:
                rd_min = r(rd_min * r(1.01))
            elif n_max == 0:
                rd_max = r(rd_max / r(1.01))
            else:
                break
        rngs.append((lo, r(hi - lo)))
    tot = r(0)
    for _, rng in rngs:
        tot = r(tot + rng)
    res = []
    for fn, (lo, rng) in zip(fns, rngs):
        n_bins = int(r(r(rlx_bins) * rng) / tot)
        size = r(rng / r(n_bins))
        edges = np.array([r(math.exp(r(3) * r(lo + r(r(b) * size)))) for b in range(n_bins + 1)], dtype=np.float64)
        conc = np.array([r(r(fn(float(r(float(lo) + (b + 0.5) * float(size))))) * size) for b in range(n_bins)], dtype=np.float64)
        res.append((edges, conc))
    return res


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["double", "float"])
def test_the_objects_tables_are_the_layouts(real_t):
    """The restatements above take edges and bin-centre concentrations from the object.  In double they must be lcx_rlx_layout's to the
    last bit (which tests/test_relaxation_api.py holds to its own restatement).  In float they are held to the same expressions
    restated in np.float32 (float_layout).  That restatement takes logarithms and exponentials in double and rounds them, the library
    calls logf / expf, each within one float ulp of the true value: ln rd_min (about -18, where a float ulp is 1.9e-6) may differ by one
    ulp, the sum ln rd_min + b * bin by one more rounding (0.95e-6), rd3 = exp(3 ...) carries three times that plus two ulps of its own
    (1.2e-7): 3 x 2.9e-6 + 1.2e-7 < 1e-5 relative for the edges.  The spectrum's logarithmic slope (ln rd - ln mean) / ln^2 sigma reaches
    about 10 at the ends of the range, so a centre that is 2.9e-6 off moves the concentration by 3e-5; with the bin width's ulp: 4e-5."""
    oi, f = plan_box(False, False, real_t)
    p = h.hip_particles(oi, real_t)
    tabs = tables(p, oi)
    assert len(tabs) == 2
    if real_t is np.float32:
        fns = [h.lognormal_fn(A_INIT[0], A_INIT[1], 2.5 * A_INIT[2]), h.lognormal_fn(.1e-6, 1.5, 3 * B_INIT[2])]       # plan_box's two spectra
        ref = float_layout(fns, oi.rlx_bins, oi.dx * oi.dy * oi.dz)
    for s, t in enumerate(tabs):
        edges, conc = lgrngn.rlx_layout(oi, s)
        if real_t is np.float64:
            assert np.array_equal(t["edges"], edges) and np.array_equal(t["conc"], conc)
        else:
            edges, conc = ref[s]
            assert t["edges"].size == edges.size and t["conc"].size == conc.size
            assert np.array_equal(t["edges"], t["edges"].astype(np.float32)) and np.all(np.diff(t["edges"]) > 0)
            print("float tables against the float restatement: edges", np.abs(t["edges"] / edges - 1).max(), "concentrations", np.abs(t["conc"] / conc - 1).max())
            np.testing.assert_allclose(t["edges"], edges, rtol=1e-5)
            np.testing.assert_allclose(t["conc"], conc, rtol=4e-5)


# ------------------------------------------------------------------ 1: relax.py's known answers
def relax_py_opts(builtin, spb, seed):
    """relax.py:41-63,104-120"""
    oi = lgrngn.opts_init_t()
    oi.nx = oi.nz = 2
    oi.dx = oi.dz = 1.
    oi.x1 = oi.z1 = 2.
    oi.dt = 1.
    oi.aerosol_independent_of_rhod = True
    oi.coal_switch = oi.sedi_switch = False
    oi.rlx_switch = True
    oi.rng_seed = seed
    oi.dry_distros = {(.61, 0.): spectrum(INIT, builtin)}
    oi.rlx_dry_distros = {.61: [spectrum(RLX, builtin), [0, 2], [0, oi.dz]]}
    oi.sd_conc = 1024
    oi.rlx_bins, oi.rlx_timescale, oi.rlx_sd_per_bin, oi.supstp_rlx = 1024, 4, spb, 2
    oi.n_sd_max = int((oi.sd_conc * 2 + oi.rlx_bins * spb * 2) * 2)
    return oi


def fields_2x2(real_t=np.float64):
    return np.full((2, 2), 300., real_t), np.full((2, 2), .01, real_t), np.full((2, 2), 1., real_t)


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("builtin", [True, False], ids=["lognormal", "callable"])
@pytest.mark.parametrize("spb", [1, 10])
def test_reference_known_answers(spb, builtin, real_t):
    """relax.py:117-172: two steps, one firing, relaxation time scale twice the run: half of what is missing is added"""
    for seed in (44, 7, 12345, 1, 2):
        p = h.hip_particles(relax_py_opts(builtin, spb, seed), real_t)
        f = fields_2x2(real_t)
        p.init(*f)
        steps(p, only_rlx(), f, 2)
        sd = cell_field(p, "diag_sd_conc")
        m0, m1 = cell_field(p, "diag_wet_mom", 0), cell_field(p, "diag_wet_mom", 1)
        r0, r1 = (m0[0] + m0[2]) / (m0[1] + m0[3]), (m1[0] + m1[2]) / (m1[1] + m1[3])
        print("seed", seed, "sd_conc", sd, "moment ratios", r0, r1)
        assert 1024 + 400 * spb <= sd[0] <= 1024 + 600 * spb and 1024 + 400 * spb <= sd[2] <= 1024 + 600 * spb
        assert sd[1] == 1024 and sd[3] == 1024
        assert abs(r0 - 1.5) <= 0.01 and abs(r1 - 1.5) <= 0.01


# ------------------------------------------------------------------ 2: the plan, exactly
A_INIT, B_INIT = (.03e-6, 1.5, 80e6), (.08e-6, 1.3, 30e6)
K_A, K_B = .3, .9


def plan_box(three_d, indep, real_t, seed=3, **kw):
    oi = lgrngn.opts_init_t()
    if three_d:
        oi.nx, oi.ny, oi.nz = 4, 3, 5
        oi.dx, oi.dy, oi.dz = 2., 1.5, 1.
        oi.x0, oi.y0, oi.z0 = .4, .3, .25
        oi.x1, oi.y1, oi.z1 = 7.5, 4.2, 4.6
    else:
        oi.nx, oi.nz = 6, 5
        oi.dx, oi.dz = 2., 1.
        oi.x0, oi.z0 = .4, .25
        oi.x1, oi.z1 = 11.5, 4.6
    oi.dt = .5
    oi.coal_switch = oi.sedi_switch = False
    oi.aerosol_independent_of_rhod = indep
    oi.diag_incloud_time = True
    oi.reorder_every = -1
    oi.dbg_flags = int(lgrngn.dbg.TAG)
    oi.rng_seed = seed
    oi.sd_conc = 48
    oi.dry_distros = {(K_A, 0.): spectrum(A_INIT, True), (K_B, 0.): spectrum(B_INIT, False)}
    oi.rlx_switch = True
    oi.rlx_bins, oi.rlx_sd_per_bin, oi.rlx_timescale, oi.supstp_rlx = 60, 2, 3., 2
    # two spectra, disjoint kappa ranges, different altitude ranges (the second one's reaches past the top: clamped to nz)
    oi.rlx_dry_distros = {K_A: [spectrum((A_INIT[0], A_INIT[1], 2.5 * A_INIT[2]), True), [0, .5], [1., 3.5]],
                          K_B: [spectrum((.1e-6, 1.5, 3 * B_INIT[2]), False), [.5, 1.5], [2.2, 7.]]}
    ncell = oi.nx * max(oi.ny, 1) * oi.nz
    oi.n_sd_max = 2 * 48 * ncell + 2 * 60 * 5 + 64
    for k, v in kw.items():
        setattr(oi, k, v)
    shp = (oi.nx, oi.ny, oi.nz) if three_d else (oi.nx, oi.nz)
    rhod = np.broadcast_to(1.15 - .03 * np.arange(oi.nz), shp).astype(real_t).copy()
    f = (np.full(shp, 300., real_t), np.full(shp, .01, real_t), rhod)
    return oi, f


NAMES = ("rd3", "rw2", "x", "y", "z", "kappa", "incloud_time", "tag")


def full_state(p, three_d):
    st = {k: p.state_real(k) for k in NAMES if three_d or k != "y"}
    st.update(n=p.state_u64("n"), ijk=p.state_u64("ijk"))
    return st


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("indep", [False, True], ids=["rhod", "indep_rhod"])
@pytest.mark.parametrize("three_d", [False, True], ids=["2d", "3d"])
def test_the_plan_exactly(three_d, indep, real_t):
    oi, f = plan_box(three_d, indep, real_t)
    p, q = h.hip_particles(oi, real_t), h.hip_particles(oi, real_t)          # q: the same run without opts.rlx
    p.init(*f)
    q.init(*f)
    before = full_state(p, three_d)
    n_old = p.n_part
    assert set(np.unique(before["kappa"]).astype(np.float32).tolist()) == {np.float32(K_A), np.float32(K_B)}
    expect = whole_plan(p, oi, before, real_t, f[2].reshape(-1, oi.nz)[0])
    off = only_rlx()
    off.rlx = False
    steps(p, only_rlx(), f, 1)
    steps(q, off, f, 1)
    after, twin = full_state(p, three_d), full_state(q, three_d)
    assert q.n_part == n_old and p.n_part > n_old
    # the old super-droplets: first (reorder_every = -1), bit for bit what the run without relaxation holds
    for k in twin:
        assert np.array_equal(after[k][:n_old], twin[k]), k
    new = {k: v[n_old:] for k, v in after.items()}
    assert np.all(new["tag"] >= n_old) and np.unique(new["tag"]).size == new["tag"].size
    got = newcomers_as_plan(p, oi, new)
    print("newcomers", len(got), "planned", len(expect))
    if real_t is np.float64:
        assert got == expect
    else:
        # the same plan restated in float: counts per (kappa, level, bin) exact, a multiplicity off by one in at most 1 % of the newcomers
        assert [g[:3] for g in got] == [e[:3] for e in expect]
        d = np.abs(np.array([g[3] for g in got], dtype=np.int64) - np.array([e[3] for e in expect], dtype=np.int64))
        print("float: multiplicities that differ from the restatement:", int((d > 0).sum()), "of", d.size, "largest difference", int(d.max()))
        assert d.max() <= 1 and (d > 0).sum() <= .01 * d.size
    # both spectra and only their levels
    lev = {K_A: set(), K_B: set()}
    for kappa, k, _, _ in got:
        lev[kappa].add(k)
    assert lev[K_A] == {1, 2} and lev[K_B] == {2, 3, 4}
    # where they are: inside their cell and inside the domain; wet radius above the dry one; the extension attributes of a newcomer
    nyz = max(oi.ny, 1) * oi.nz
    ci, cj, ck = new["ijk"] // nyz, (new["ijk"] // oi.nz) % max(oi.ny, 1), new["ijk"] % oi.nz
    dims = [("x", ci, oi.dx, oi.x0, oi.x1), ("z", ck, oi.dz, oi.z0, oi.z1)] + ([("y", cj, oi.dy, oi.y0, oi.y1)] if three_d else [])
    for name, idx, d, lo, hi in dims:
        pos = new[name]
        assert np.all(pos >= idx * d) and np.all(pos < (idx + 1) * d) and np.all(pos >= real_t(lo)) and np.all(pos < real_t(hi)), name
    assert set(ci.tolist()) == set(range(oi.nx))                   # i (and j) are drawn over the whole level
    assert np.all(new["rw2"] ** 1.5 > new["rd3"])
    assert np.all(new["incloud_time"] == 0)
    assert np.all(new["n"] > 0)
    assert cell_field(p, "diag_sd_conc").sum() == p.n_part


# ------------------------------------------------------------------ 3: the cells of the start of the step
def test_census_sees_the_cells_of_the_step_start():
    """Euler advection with an upward Courant number that carries droplets across levels in the firing step: the reference's ijk is not
    refreshed between its advection and its relaxation, so the plan is the one of the levels BEFORE the step"""
    oi, f = plan_box(False, True, np.float64, adve_scheme=lgrngn.as_t.euler, periodic_topbot_walls=True, z0=0., z1=5.)
    C = dict(Cx=np.zeros((oi.nx + 1, oi.nz)), Cz=np.full((oi.nx, oi.nz + 1), .6))
    p, q = h.hip_particles(oi), h.hip_particles(oi)
    p.init(*f, **C)
    q.init(*f, **C)
    before = state_of(p)
    n_old = p.n_part
    on, off = only_rlx(), only_rlx()
    on.adve, off.adve, off.rlx = True, True, False
    steps(p, on, f, 1, C)
    steps(q, off, f, 1, C)
    moved = state_of(q)
    crossed = (moved["ijk"] % oi.nz != before["ijk"] % oi.nz).mean()
    print("fraction of the droplets that changed level in the step:", crossed)
    assert crossed > .4
    after = state_of(p)
    got = newcomers_as_plan(p, oi, {k: v[n_old:] for k, v in after.items()})
    col = f[2].reshape(-1, oi.nz)[0]
    assert got == whole_plan(p, oi, before, np.float64, col)
    assert got != whole_plan(p, oi, moved, np.float64, col)


# ------------------------------------------------------------------ 4: census edge cases
def census_box(rlx_bins=64, dbg=0):
    oi = lgrngn.opts_init_t()
    oi.nx, oi.nz = 2, 3
    oi.dx = oi.dz = 1.
    oi.x1, oi.z1 = 2., 3.
    oi.dt = 1.
    oi.coal_switch = oi.sedi_switch = False
    oi.aerosol_independent_of_rhod = True
    oi.reorder_every = -1
    oi.dbg_flags = int(dbg)
    oi.sd_conc = 8
    oi.dry_distros = {(.61, 0.): spectrum(INIT, True)}
    oi.rlx_switch = True
    oi.rlx_bins, oi.rlx_sd_per_bin, oi.rlx_timescale, oi.supstp_rlx = rlx_bins, 1, 1., 1
    oi.rlx_dry_distros = {.61: [spectrum(RLX, True), [.5, .7], [0, 3.]]}
    oi.n_sd_max = 48 + 3 * rlx_bins + 64
    return oi


@pytest.mark.parametrize("global_atomics", [False, True], ids=["lds_table", "global_atomics"])
def test_census_edge_cases(global_atomics):
    oi = census_box(dbg=lgrngn.dbg.RLX_GLOBAL_ATOMICS if global_atomics else 0)
    p = h.hip_particles(oi)
    f = tuple(np.full((2, 3), v) for v in (300., .01, 1.))
    p.init(*f)
    e = tables(p, oi)[0]["edges"]
    below = lambda v: np.nextafter(v, 0.)
    # (rd3, kappa, n, z): level 2 stays empty
    drops = [(e[10], .61, 5, .5),                 # ON an edge: the upper bin (10)
             (below(e[10]), .61, 7, .5),          # just below it: bin 9
             (e[10], .61, 11, 1.5),               # the same size one level up
             (e[0], .61, 13, .5),                 # the first edge: bin 0
             (below(e[0]), .61, 17, .5),          # below the first edge: not counted
             (e[-1], .61, 19, .5),                # the last edge: not counted
             (below(e[-1]), .61, 23, .5),         # just below it: the last bin
             (e[20], .7, 29, .5),                 # kappa == kappa_max: not counted
             (e[20], .5, 31, .5),                 # kappa == kappa_min: counted
             (e[20], below(.7), 37, 1.5),
             (e[30], .61, 0, .5),                 # dead: adds nothing
             (e[31] * 1.001, .61, 2 ** 40, 1.5)]  # a multiplicity beyond 32 bits
    rd3, kpa, n, z = (np.array(c) for c in zip(*drops))
    x = np.linspace(.1, 1.9, len(drops))
    p.set_particles(n.astype(np.uint64), rd3, (1.2 * rd3 ** (1 / 3.)) ** 2, kpa, np.zeros(len(drops)), x=x, z=z)
    steps(p, only_rlx(), f, 1)
    cnt = p.state_u64("raw_rlx_count").reshape(64, 3)
    want = np.zeros((64, 3), dtype=np.uint64)
    want[10, 0], want[9, 0], want[10, 1], want[0, 0], want[63, 0], want[20, 0], want[20, 1], want[31, 1] = 5, 7, 11, 13, 23, 31, 37, 2 ** 40
    assert np.array_equal(cnt, want)
    assert not cnt[:, 2].any()
    # the empty level gets every bin's super-droplet, the others miss those that the census found filled
    lev = p.state_u64("ijk")[len(drops) - 1:] % 3              # (the dead one is gone)
    assert (lev == 2).sum() == 64


def test_rlx_bins_at_the_cap_and_above():
    oi = census_box(rlx_bins=1024)
    p = h.hip_particles(oi)
    f = tuple(np.full((2, 3), v) for v in (300., .01, 1.))
    p.init(*f)
    before = state_of(p)
    steps(p, only_rlx(), f, 1)
    tab = tables(p, oi)[0]
    assert tab["conc"].size == 1024
    assert np.array_equal(p.state_u64("raw_rlx_count").reshape(1024, 3), census(oi, before, tab, np.float64))
    got = newcomers_as_plan(p, oi, {k: v[48:] for k, v in state_of(p).items()})
    assert got == whole_plan(p, oi, before, np.float64, np.ones(3))
    _raises("rlx_bins above 1024", lambda: h.hip_particles(census_box(rlx_bins=1025)))


# ------------------------------------------------------------------ 5: counter semantics
def small_run(**kw):
    oi = relax_py_opts(True, 1, 44)
    oi.sd_conc, oi.rlx_bins, oi.n_sd_max = 16, 32, 4000
    for k, v in kw.items():
        setattr(oi, k, v)
    p = h.hip_particles(oi)
    f = fields_2x2()
    p.init(*f)
    return p, only_rlx(), f


def test_counter_semantics():
    p, opts, f = small_run(supstp_rlx=3, rlx_timescale=300.)
    seen = []
    for _ in range(8):
        steps(p, opts, f, 1)
        seen.append(p.n_part)
    grow = [b - a for a, b in zip([64] + seen[:-1], seen)]
    print("growth per step", grow)
    assert all((g > 0) == (i % 3 == 0) for i, g in enumerate(grow))            # fires at steps 0, 3, 6
    opts.rlx = False
    steps(p, opts, f, 1)                                            # ... resets the counter
    assert p.n_part == seen[-1]
    opts.rlx = True
    steps(p, opts, f, 1)
    assert p.n_part > seen[-1]


def test_a_relaxed_state_gets_less_and_a_full_one_nothing():
    # time scale = the firing's interval: the first firing adds all that is missing, the second finds the bins (nearly) full
    p, opts, f = small_run(supstp_rlx=1, rlx_timescale=1., sd_conc=256, rlx_bins=128, rlx_dry_distros={.61: [spectrum(RLX, True), [0, 2], [0, 2.]]})
    n0 = p.n_part
    steps(p, opts, f, 1)
    first = p.n_part - n0
    steps(p, opts, f, 1)
    second = p.n_part - n0 - first
    print("created by the first firing", first, "by the second", second)
    assert 0 <= second < first / 4
    # a target far below what is there (1 / 32 of the initial spectrum in 16 bins: its range of ln rd lies inside that of the 256 initial
    # super-droplets per cell, so no bin is empty): nothing is created, nothing is appended to the storage
    p, opts, f = small_run(supstp_rlx=1, sd_conc=256, rlx_bins=16, rlx_dry_distros={.61: [spectrum((INIT[0], INIT[1], INIT[2] / 32), True), [0, 2], [0, 2.]]})
    n0, extent = p.n_part, p.state_u64("raw_n").size
    steps(p, opts, f, 2)
    assert p.n_part == n0 and p.state_u64("raw_n").size == extent


# ------------------------------------------------------------------ 6: nothing changes when nothing fires
def full_physics_box(seed=5, **kw):
    oi = h.api_default_opts(h.box_opts(8, 8, 8, 64, rng_seed=seed))
    oi.n_sd_max = 64 * 512 * 2
    oi.rlx_switch = True
    oi.rlx_bins, oi.rlx_sd_per_bin, oi.rlx_timescale, oi.supstp_rlx = 64, 1, 100., 1000
    oi.rlx_dry_distros = {.61: [lgrngn.lognormal(.02e-6, 1.4, 120e6), [0, 2], [0, 80.]]}
    for k, v in kw.items():
        setattr(oi, k, v)
    return oi


def run_counted(oi, rlx_in_step, n_steps):
    fields = h.box_fields(oi)
    th, rv, rhod, C = fields
    p = h.hip_particles(oi)
    p.init(th.copy(), rv.copy(), rhod.copy(), **C)
    th, rv = th.copy(), rv.copy()
    per_step, modes = [], []
    for s in range(n_steps):
        opts = lgrngn.opts_t()
        opts.rlx = rlx_in_step(s)
        l0 = p.state_u64("raw_launches").astype(np.int64)
        p.step_sync(opts, th, rv, rhod, **C)
        p.step_async(opts)
        per_step.append(tuple((p.state_u64("raw_launches").astype(np.int64) - l0).tolist()))
        modes.append(p.mode())
    state = {k: p.state_real(k) for k in ("rd3", "rw2", "x", "y", "z")}
    state.update(n=p.state_u64("n"), th=th.copy(), rv=rv.copy())
    return per_step, modes, state, p.n_part


def test_nothing_changes_when_nothing_fires():
    """both runs fire in step 0 (the counter starts at 0); from then on A keeps opts.rlx without firing (supstp_rlx = 1000), B drops it"""
    a_steps, a_modes, a_state, a_n = run_counted(full_physics_box(), lambda s: True, 6)
    b_steps, b_modes, b_state, b_n = run_counted(full_physics_box(), lambda s: s == 0, 6)
    print("launches, waits per step: A", a_steps, "B", b_steps)
    assert a_steps == b_steps and a_modes == b_modes and a_n == b_n
    for k in a_state:
        assert np.array_equal(a_state[k], b_state[k]), k
    # (an object without the switch, for the record: step 0 did create something)
    c_steps, _, _, c_n = run_counted(full_physics_box(rlx_switch=False), lambda s: False, 6)
    print("without rlx_switch", c_steps, "n_part", c_n, "against", a_n)
    assert a_n > c_n


def test_launches_of_a_firing_do_not_depend_on_rlx_bins():
    few, _, _, n_few = run_counted(full_physics_box(rlx_bins=64), lambda s: True, 1)
    many, _, _, n_many = run_counted(full_physics_box(rlx_bins=1024), lambda s: True, 1)
    print("launches, waits of the firing step: 64 bins", few, "1024 bins (the cap)", many, "n_part", n_few, n_many)
    assert few == many and n_many > n_few


# ------------------------------------------------------------------ 7: a run that goes on
def census_by_tag(oi, before, after, tag_hi, tab):
    """The census of a step that also coalesces, restated from outside: coalescence runs first and changes n and rd3 of the old
    super-droplets (one of a pair may end with n == 0 and is gone afterwards), the census counts what it left, in the cells of the
    step's START; nothing behind the census touches n, rd3 or kappa of an old super-droplet.  So its input is (n, rd3, kappa) read AFTER
    the step for the old tags, joined by tag with the level read BEFORE it.  A super-droplet that the move takes out of the domain is
    gone afterwards as well, but it started in the lowest or the highest level; the caller relaxes neither."""
    old = after["tag"] < tag_hi
    order = np.argsort(before["tag"])
    pos = order[np.searchsorted(before["tag"][order], after["tag"][old])]
    assert np.array_equal(before["tag"][pos], after["tag"][old])
    st = {k: after[k][old] for k in ("n", "rd3", "kappa")}
    st["ijk"] = before["ijk"][pos]
    return census(oi, st, tab, np.float64), before["tag"].size - int(old.sum())


def test_long_run_with_everything_on():
    """8 x 8 x 8 x 64, condensation, coalescence (Hall), sedimentation, advection, 200 steps, a firing every 10, coalescence in the
    firing steps too.  At every firing: the census table the object holds is the one restated from outside (census_by_tag), the
    newcomers are the plan restated from it, and a second object whose census is the global-atomic kernel holds the same table (the
    two runs are the same run as long as the tables agree).  The lowest and the highest level are not relaxed: what rains out or
    leaves through the top in a firing step was not counted in a relaxed level."""
    def make(dbg):
        oi = h.box_opts(8, 8, 8, 64, rng_seed=21, kernel=lgrngn.kernel_t.hall, dbg_flags=int(lgrngn.dbg.TAG | dbg))
        oi.rlx_switch = True
        oi.rlx_bins, oi.rlx_sd_per_bin, oi.rlx_timescale, oi.supstp_rlx = 48, 1, 40., 10
        bimodal = h.lgrngn_bimodal()
        oi.rlx_dry_distros = {.61: [lambda lnrd: 2 * bimodal(lnrd), [0, 2], [40., 280.]]}          # twice the initial spectrum, levels 1 .. 6
        oi.n_sd_max = 64 * 512 + 20 * 48 * 6 + 64
        th, rv, rhod, C = h.box_fields(oi)
        p = h.hip_particles(oi)
        p.init(th.copy(), rv.copy(), rhod.copy(), **C)
        return oi, p, th.copy(), rv.copy(), rhod, C
    oi, p, th, rv, rhod, C = make(0)
    _, q, thq, rvq, _, _ = make(lgrngn.dbg.RLX_GLOBAL_ATOMICS)
    col = rhod.reshape(-1, 8)[0]
    opts = lgrngn.opts_t()
    opts.rlx = True
    created, gone = [], []
    names = ("rd3", "kappa", "tag")
    for step in range(200):
        fires = step % 10 == 0
        if fires:                                                  # (condensation, all that step_sync does, changes none of these)
            before = state_of(p, names)
            tag_hi = before["tag"].max() + 1
            state_of(q, names)                                     # (a getter may compact the storage: the twin gets the same calls)
        p.step_sync(opts, th, rv, rhod, **C)
        p.step_async(opts)
        q.step_sync(opts, thq, rvq, rhod, **C)
        q.step_async(opts)
        assert p.n_part <= oi.n_sd_max
        if fires:
            after = state_of(p, names)
            after_q = state_of(q, names)
            assert all(np.array_equal(after[k], after_q[k]) for k in after)
            tab, = tables(p, oi)
            hor, n_gone = census_by_tag(oi, before, after, tag_hi, tab)
            hor[:, [0, 7]] = 0                                     # (not relaxed: not visited)
            table = p.state_u64("raw_rlx_count").reshape(48, 8)
            assert np.array_equal(table, hor), step
            assert np.array_equal(q.state_u64("raw_rlx_count").reshape(48, 8), table), step
            expect = sorted(plan_of(oi, tab, hor, np.float64, col, oi.dt)[0])
            sel = after["tag"] >= tag_hi
            got = newcomers_as_plan(p, oi, {k: v[sel] for k, v in after.items()})
            created.append(len(got))
            gone.append(n_gone)
            assert got == expect, step
            assert cell_field(p, "diag_sd_conc").sum() == p.n_part
            assert cell_field(q, "diag_sd_conc").sum() == q.n_part
    print("created per firing", created, "old super-droplets gone in the firing steps (coalescence, rain)", gone, "n_part at the end", p.n_part)
    assert p.n_part == q.n_part
    assert created[0] > 0 and sum(c > 0 for c in created) >= 3
    assert sum(gone) > 0                                           # the firing steps did use super-droplets up


def test_levels_outside_the_altitude_range_are_left_alone():
    """adve = sedi = False, condensation on: the levels that no spectrum relaxes hold what a run without relaxation holds, to the last
    bit.  (Without coalescence: its random numbers go by position in the cell-sorted order, which newcomers in other cells shift.)"""
    res = []
    for rlx in (True, False):
        oi = h.box_opts(8, 8, 8, 64, rng_seed=22, coal_switch=False)
        oi.rlx_switch = True
        oi.rlx_bins, oi.rlx_sd_per_bin, oi.rlx_timescale, oi.supstp_rlx = 48, 1, 10., 5
        bimodal = h.lgrngn_bimodal()
        oi.rlx_dry_distros = {.61: [lambda lnrd: 2 * bimodal(lnrd), [0, 2], [80., 160.]]}
        oi.n_sd_max = 64 * 512 + 8 * 48 * 2 + 64
        th, rv, rhod, C = h.box_fields(oi)
        p = h.hip_particles(oi)
        p.init(th.copy(), rv.copy(), rhod.copy(), **C)
        opts = lgrngn.opts_t()
        opts.adve = opts.sedi = opts.coal = False
        opts.rlx = rlx
        th, rv = th.copy(), rv.copy()
        for _ in range(30):
            p.step_sync(opts, th, rv, rhod, **C)
            p.step_async(opts)
        res.append([cell_field(p, "diag_sd_conc").reshape(8, 8, 8)] + [cell_field(p, "diag_wet_mom", k).reshape(8, 8, 8) for k in range(4)]
                   + [th.copy(), rv.copy()])
    outside = [0, 1, 4, 5, 6, 7]
    for a, b in zip(*res):
        assert np.array_equal(a[:, :, outside], b[:, :, outside])
    assert res[0][0][:, :, 2:4].sum() > res[1][0][:, :, 2:4].sum()


# ------------------------------------------------------------------ 8: errors
def test_errors():
    f = fields_2x2()
    _raises("libcloudph++: rlx_bins <= 0", lambda: small_run(rlx_bins=0))
    _raises("libcloudph++: rlx_sd_per_bin <= 0", lambda: small_run(rlx_sd_per_bin=0))
    _raises("libcloudph++: rlx_timescale <= 0", lambda: small_run(rlx_timescale=0.))
    _raises("z_min > z_max", lambda: small_run(rlx_dry_distros={.61: [spectrum(RLX, True), [0, 2], [1.5, 1.]]}))
    _raises("empty kappa range", lambda: small_run(rlx_dry_distros={.61: [spectrum(RLX, True), [1, 1], [0, 1.]]}))
    # opts.rlx while the switch is off
    p, opts, _ = small_run(rlx_switch=False)
    _raises("aerosol relaxation was switched off in opts_init", lambda: steps(p, opts, f, 1))

    def one_d():
        oi = relax_py_opts(True, 1, 44)
        oi.nz, oi.sd_conc, oi.n_sd_max = 0, 8, 64
        h.hip_particles(oi)
    _raises("CCN relaxation works only in 2D and 3D, set rlx_switch to false", one_d)
    # relaxation together with a source stays refused, before the values are looked at
    _raises("option outside the accelerated hot path", lambda: small_run(src_type=lgrngn.src_t.simple, rlx_bins=0))
    # an altitude range above the domain is clamped to it, not an error
    p, opts, _ = small_run(rlx_dry_distros={.61: [spectrum(RLX, True), [0, 2], [1., 50.]]})
    steps(p, opts, f, 1)
    sd = cell_field(p, "diag_sd_conc")
    assert sd[0] == 16 and sd[2] == 16 and sd[1] > 16 and sd[3] > 16


# ------------------------------------------------------------------ 9: the multi-device object
def test_multi_device_object(monkeypatch):
    """two slabs on one device: each relaxes on its own horizontal sums over its own x0 .. x1 with rlx_sd_per_bin / 2
    (distmem_opts.hpp:49), so each slab's newcomers are the plan restated per slab"""
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi, f = plan_box(False, False, np.float64, dev_count=2, rlx_sd_per_bin=4, dbg_flags=0)      # x0 = .4, x1 = 11.5: partial outer cells
    p = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert p.dev_count == 2
    p.init(*f)
    slabs = [p.slab(i) for i in range(2)]
    before = [state_of(s) for s in slabs]
    expect = []
    for i, s in enumerate(slabs):
        so = copy.copy(oi)
        so.nx = 3                                                  # (cells are numbered inside the slab)
        # the slab's own frame: the first one keeps x0 and ends at its last plane, the second begins at 0 and ends at x1 - 6
        expect.append(whole_plan(s, so, before[i], np.float64, f[2][0], x_extent=((.4, 6.), (0., 5.5))[i], spb=2))
    steps(p, only_rlx(), f, 1)
    for i, s in enumerate(slabs):
        n_old = before[i]["n"].size
        after = state_of(s)
        got = newcomers_as_plan(s, oi, {k: v[n_old:] for k, v in after.items()})
        print("slab", i, "newcomers", len(got))
        assert got == expect[i] and len(got) > 0
    assert cell_field(p, "diag_sd_conc").sum() == p.n_part
