"""The aerosol source (opts_init.src_type simple / matching, opts.src_dry_distros / src_dry_sizes) on the HIP path.

The CPU oracle has no source, so the yardsticks are (a) the reference's own known answers (its tests/python/unit/source.py),
restated here, (b) numpy restatements of the reference's formulas, written in this file and fed with the state the library reports,
and (c) the oracle's init(), which shares every formula a source uses."""
import math

import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

KEY = (.61, 0.)
RHO_STP = 101325. / (273.15 + 15) / (8.3144621 / 0.02897)          # p_stp / T_stp / R_d
INIT = (.02e-6, 1.4, 60e6)                                          # source.py:35-80
SRC = (.05e-6, 1.4, 60e4)                                           # per second


def spectrum(par, builtin):
    return lgrngn.lognormal(*par) if builtin else h.lognormal_fn(*par)


# ------------------------------------------------------------------ restatements of the reference's formulas
def dist_analysis(fn, sd_conc, dt, vol, real=np.float64):
    """init_dist_analysis_sd_conc (initialization/particles_impl_init_dist_analysis.ipp:17-77): (ln rd_min, ln rd_max, multiplier)"""
    r = real
    rd_min, rd_max = r(1e-14), r(1e-3)
    while True:
        mult = r(math.log(rd_max / rd_min) / sd_conc * r(dt) * r(vol))
        lo, hi = r(math.log(rd_min)), r(math.log(rd_max))
        n_min, n_max = int(r(fn(lo)) * mult), int(r(fn(hi)) * mult)
        if n_min == 0:
            rd_min = r(rd_min * r(1.01))
        elif n_max == 0:
            rd_max = r(rd_max / r(1.01))
        else:
            return float(lo), float(hi), float(mult)


def src_cells(oi):
    """init_count_num_src (initialization/particles_impl_init_count_num.ipp:120-175), cells as the flat index (i * ny + j) * nz + k"""
    e = lambda v, d: int(v / d + 0.5)
    i0, i1, k0, k1 = e(oi.src_x0, oi.dx), e(oi.src_x1, oi.dx), e(oi.src_z0, oi.dz), e(oi.src_z1, oi.dz)
    j0, j1 = (e(oi.src_y0, oi.dy), e(oi.src_y1, oi.dy)) if oi.ny else (0, 1)
    ny = max(oi.ny, 1)
    return sorted((i * ny + j) * oi.nz + k for i in range(oi.nx) for j in range(ny) for k in range(oi.nz)
                  if i0 <= i < i1 and j0 <= j < j1 and k0 <= k < k1)


# ------------------------------------------------------------------ the set-up of source.py:35-80
def opts_2x2(src_type, seed, n_sd_max=6144):
    oi = lgrngn.opts_init_t()
    oi.nx = oi.nz = 2
    oi.dx = oi.dz = 1.
    oi.x1 = oi.z1 = 2.
    oi.dt = 1.
    oi.coal_switch = oi.sedi_switch = False
    oi.rng_seed = seed
    oi.src_type = src_type
    oi.src_x0, oi.src_x1, oi.src_z0, oi.src_z1 = 0., 2., 0., 1.     # the lower row
    oi.n_sd_max = n_sd_max
    return oi


def only_src():
    o = lgrngn.opts_t()
    o.adve = o.sedi = o.cond = o.coal = False
    o.src = True
    return o


def fields_2x2(real_t=np.float64):
    return np.full((2, 2), 300., real_t), np.full((2, 2), .01, real_t), np.full((2, 2), 1., real_t)


def make_distro_run(src_type, builtin, seed, real_t=np.float64, n_sd_max=6144):
    oi = opts_2x2(src_type, seed, n_sd_max)
    oi.dry_distros = {KEY: spectrum(INIT, builtin)}
    oi.sd_conc = 1024
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, builtin), 512, 50)}
    p = h.hip_particles(oi, real_t)
    f = fields_2x2(real_t)
    p.init(*f)
    return p, opts, f


def steps(p, opts, f, n):
    for _ in range(n):
        p.step_sync(opts, *f)
        p.step_async(opts)


def cell_field(p, what, *a):
    p.diag_all()
    getattr(p, what)(*a)
    return p.outbuf_array().astype(np.float64)


def lower_over_upper(v):
    return (v[0] + v[2]) / (v[1] + v[3])                            # 2-D: cell = i * nz + k, k = 0 the lower row


_proxy = {}


def oracle_proxy():
    """1 + sum M_k(source spectrum) / sum M_k(initial spectrum), k = 0 and 1, from the ORACLE's init() with each spectrum at equal total number
    (two firings of 50 s at 60e4 per second = 60e6; 512 and 1024 super-droplets per cell), for 8 seeds: what the lower-over-upper ratio of
    the wet moments is if the source samples its spectrum the way init() samples the initial one"""
    if "v" in _proxy:
        return _proxy["v"]
    res = []
    for seed in (44, 7, 12345, 1, 2, 3, 4, 5):
        m = {}
        for name, par, sd in (("init", INIT, 1024), ("src", (SRC[0], SRC[1], SRC[2] * 100), 512)):
            oi = opts_2x2(lgrngn.src_t.off, seed)
            oi.dry_distros = {KEY: h.lognormal_fn(*par)}
            oi.sd_conc = sd
            o = h.oracle_particles(oi)
            o.init(*fields_2x2())
            m[name] = [cell_field(o, "diag_wet_mom", k).sum() for k in (0, 1)]
        res.append([1 + m["src"][k] / m["init"][k] for k in (0, 1)])
    res = np.array(res)
    print("oracle proxy moment 0:", res[:, 0], "moment 1:", res[:, 1])
    _proxy["v"] = res
    return res


def check_moments(p, tag=""):
    m0 = lower_over_upper(cell_field(p, "diag_wet_mom", 0))
    m1 = lower_over_upper(cell_field(p, "diag_wet_mom", 1))
    proxy = oracle_proxy()
    mean, sd = proxy.mean(axis=0), proxy.std(axis=0, ddof=1)
    print(tag, "moment-0 ratio", m0, "moment-1 ratio", m1, "proxy mean", mean, "proxy sample sd", sd)
    assert abs(m0 - 2.) <= 0.015                                    # source.py:117
    assert abs(m1 - 7.84 / 2.12) <= 0.015                           # source.py:121
    assert abs(m1 - mean[1]) <= 5 * sd[1], (m1, mean[1], sd[1])     # the tighter bar against the oracle


# ------------------------------------------------------------------ 1-3: simple
@pytest.mark.parametrize("seed", [44, 7])
@pytest.mark.parametrize("builtin", [False, True], ids=["callable", "lognormal"])
def test_simple_known_answers(seed, builtin):
    p, opts, f = make_distro_run(lgrngn.src_t.simple, builtin, seed)
    steps(p, opts, f, 100)                                          # fires at counter 0 and 50
    sd = cell_field(p, "diag_sd_conc")
    assert sd.tolist() == [2048., 1024., 2048., 1024.]              # source.py:111-114
    assert p.n_part == 6144                                         # n_sd_max exactly filled
    check_moments(p, tag="simple seed %d" % seed)
    with pytest.raises(RuntimeError, match=r"n_sd_max \(6144\) < n_part \(7168\)"):
        steps(p, opts, f, 1)                                        # the third firing, counter 100


# ------------------------------------------------------------------ 4: matching
def matching_geometry():
    """source bins wholly outside the initial spectrum's analysed range, and bins that straddle one of its ends"""
    i_lo, i_hi, _ = dist_analysis(h.lognormal_fn(*INIT), 1024, 1., 1.)
    s_lo, s_hi, _ = dist_analysis(h.lognormal_fn(*SRC), 512, 50., 1.)
    w = (s_hi - s_lo) / 512
    assert (i_hi - i_lo) / 1024 < w / 1.5                           # every source bin inside the initial range holds a whole stratum
    outside = straddle = 0
    for b in range(512):
        lo, hi = s_lo + b * w, s_lo + (b + 1) * w
        if hi <= i_lo or lo >= i_hi:
            outside += 1
        elif lo < i_lo or hi > i_hi:
            straddle += 1
    print("initial ln r range", i_lo, i_hi, "source", s_lo, s_hi, "bins outside", outside, "straddling", straddle)
    return outside, straddle


@pytest.mark.parametrize("seed", [44, 7])
@pytest.mark.parametrize("builtin", [False, True], ids=["callable", "lognormal"])
def test_matching_known_answers(seed, builtin):
    outside, straddle = matching_geometry()
    allowed = {1024 + outside + k for k in range(straddle + 1)}
    assert allowed == {1164, 1165}                                  # source.py:139-142
    p, opts, f = make_distro_run(lgrngn.src_t.matching, builtin, seed)
    steps(p, opts, f, 50)
    lower = lambda: p.state_u64("ijk") % 2 == 0
    n_part_50, sum_n_50 = p.n_part, int(p.state_u64("n")[lower()].sum())
    sd = cell_field(p, "diag_sd_conc")
    assert sd[1] == sd[3] == 1024 and sd[0] in allowed and sd[2] in allowed, sd
    steps(p, opts, f, 1)                                            # the second firing finds every bin occupied:
    assert p.n_part == n_part_50                                    # ... matching moves number, not count
    assert int(p.state_u64("n")[lower()].sum()) > sum_n_50
    steps(p, opts, f, 49)
    assert np.array_equal(cell_field(p, "diag_sd_conc"), sd)
    check_moments(p, tag="matching seed %d" % seed)


def test_matching_refuses_more_bins_than_it_supports():
    oi = opts_2x2(lgrngn.src_t.matching, 44, n_sd_max=40000)
    oi.dry_distros = {KEY: spectrum(INIT, True)}
    oi.sd_conc = 16
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, True), 4096, 1)}
    p = h.hip_particles(oi)
    f = fields_2x2()
    p.init(*f)
    steps(p, opts, f, 2)                                            # 4096 bins per cell are supported
    assert p.n_part <= 64 + 2 * 4096
    opts.src_dry_distros = {KEY: (spectrum(SRC, True), 4097, 1)}
    with pytest.raises(RuntimeError, match="4096"):
        steps(p, opts, f, 1)


# ------------------------------------------------------------------ 5: dry_sizes
def make_sizes_run(seed, real_t=np.float64):
    oi = opts_2x2(lgrngn.src_t.simple, seed, n_sd_max=240)
    oi.dry_sizes = {KEY: {1e-6: [30., 20], 15e-6: [10., 10]}}       # source.py:157-173
    oi.reorder_every = -1
    opts = only_src()
    opts.src_dry_sizes = {KEY: {1e-6: [.3, 10, 50], 15e-6: [.1, 5, 50]}}
    p = h.hip_particles(oi, real_t)
    f = fields_2x2(real_t)
    p.init(*f)
    return p, opts, f


@pytest.mark.parametrize("seed", [44, 7])
def test_dry_sizes_known_answers(seed):
    p, opts, f = make_sizes_run(seed)
    n_init = p.n_part
    assert n_init == 120
    steps(p, opts, f, 100)
    assert cell_field(p, "diag_sd_conc").tolist() == [60., 30., 60., 30.]
    m0 = lower_over_upper(cell_field(p, "diag_wet_mom", 0))
    print("dry_sizes moment-0 ratio", m0)
    assert abs(m0 - 2.) <= 0.001                                    # source.py:172
    n, ijk, rd3, rw2 = p.state_u64("n"), p.state_u64("ijk"), p.state_real("rd3"), p.state_real("rw2")
    rhod, dv = p.state_real("rhod"), p.state_real("dv")
    new = np.arange(n.size) >= n_init                               # reorder_every = -1: storage order is id order, newcomers behind
    assert set(ijk[new].tolist()) == {0, 2}
    for radius, (conc, count, supstp) in opts.src_dry_sizes[KEY].items():
        sel = new & np.isclose(rd3, radius ** 3, rtol=1e-12, atol=0.)
        assert sel.sum() == 2 * 2 * count                           # two firings, two cells
        for c in (0, 2):
            v = (conc * (supstp * 1.)) * dv[c]                      # init_n_dry_sizes(conc * sup_dt, count): conc_to_number, then / count + .5
            v = rhod[c] / RHO_STP * v
            assert np.all(n[sel & (ijk == c)] == int(v / count + .5))
            old = ~new & np.isclose(rd3, radius ** 3, rtol=1e-12, atol=0.) & (ijk == c)
            assert old.any()
            # the same kernel with the same inputs (nothing else runs): bit-identical wet radii
            assert np.unique(np.concatenate([rw2[old], rw2[sel & (ijk == c)]])).size == 1


# ------------------------------------------------------------------ 6: structure of one firing in 3-D
@pytest.mark.parametrize("builtin", [False, True], ids=["callable", "lognormal"])
def test_structure_of_one_simple_firing_3d(builtin):
    oi = lgrngn.opts_init_t()
    oi.nx, oi.ny, oi.nz = 4, 3, 5
    oi.dx, oi.dy, oi.dz = 2., 1.5, 1.
    oi.x1, oi.y1, oi.z1 = 8., 4.5, 5.
    oi.dt = .5
    oi.coal_switch = oi.sedi_switch = False
    oi.sd_conc = 16
    oi.n_sd_max = 16 * 60 + 8 * 60
    oi.dry_distros = {KEY: spectrum(INIT, builtin)}
    oi.aerosol_independent_of_rhod = True
    oi.aerosol_conc_factor = np.array([1., .9, .8, .7, .6])
    oi.diag_incloud_time = True
    oi.reorder_every = -1
    oi.src_type = lgrngn.src_t.simple
    oi.src_x0, oi.src_x1, oi.src_y0, oi.src_y1, oi.src_z0, oi.src_z1 = 1.7, 6.3, .8, 2.9, .6, 3.4
    cells = src_cells(oi)
    assert cells == sorted((i * 3 + j) * 5 + k for i in (1, 2) for j in (1,) for k in (1, 2))
    sd_conc, supstp = 8, 3
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, builtin), sd_conc, supstp)}
    p = h.hip_particles(oi)
    shp = (4, 3, 5)
    f = (np.full(shp, 300.), np.full(shp, .01), 1. + .01 * np.arange(60.).reshape(shp))
    p.init(*f)
    names = ("rd3", "rw2", "x", "y", "z", "kappa", "incloud_time")
    before = {k: p.state_real(k) for k in names}
    before.update(n=p.state_u64("n"), ijk=p.state_u64("ijk"))
    n_old = p.n_part
    steps(p, opts, f, 1)
    after = {k: p.state_real(k) for k in names}
    after.update(n=p.state_u64("n"), ijk=p.state_u64("ijk"))
    assert p.n_part == n_old + sd_conc * len(cells)
    # The old super-droplets: first, and bit for bit as they were.  x and y pass the periodic boundary rule in every step, source or
    # not, and that rule rounds (bcnd.ipp: x0 + fmod(x - x0 + 10 (x1 - x0), x1 - x0)): for them "as they were" is that formula, restated,
    # applied to the old value -- bit for bit as well.
    wrap = lambda v, a, b: a + np.fmod((v - a) + 10 * (b - a), b - a)
    before["x"], before["y"] = wrap(before["x"], oi.x0, oi.x1), wrap(before["y"], oi.y0, oi.y1)
    for k in before:
        assert np.array_equal(after[k][:n_old], before[k]), k
    new = {k: v[n_old:] for k, v in after.items()}
    assert sorted(set(new["ijk"].tolist())) == cells
    assert all((new["ijk"] == c).sum() == sd_conc for c in cells)
    fn = h.lognormal_fn(*SRC)
    lo, hi, mult = dist_analysis(fn, sd_conc, supstp * oi.dt, oi.dx * oi.dy * oi.dz)
    lnrd = np.array([math.log(v) / 3. for v in new["rd3"]])
    stratum = np.floor((lnrd - lo) / (hi - lo) * sd_conc).astype(int)
    for c in cells:
        assert sorted(stratum[new["ijk"] == c].tolist()) == list(range(sd_conc))
    ci, cj, ck = new["ijk"] // 15, (new["ijk"] // 5) % 3, new["ijk"] % 5
    for pos, idx, d in ((new["x"], ci, oi.dx), (new["y"], cj, oi.dy), (new["z"], ck, oi.dz)):
        assert np.all(pos >= idx * d) and np.all(pos < (idx + 1) * d)
    dv = p.state_real("dv")
    expect = []
    for l, c in zip(lnrd, new["ijk"]):
        v = mult * fn(l)                                            # init_n.ipp:48-143; aerosol_independent_of_rhod: no rhod / rho_stp
        v = v * oi.aerosol_conc_factor[c % 5]
        v = v * dv[c] / (oi.dx * oi.dy * oi.dz)
        expect.append(int(v + .5))
    diff = np.abs(new["n"].astype(np.int64) - np.array(expect, dtype=np.int64))
    assert diff.max() <= (1 if builtin else 0), diff.max()
    assert np.all(new["n"] > 0)
    assert np.all(new["rw2"] ** 1.5 > new["rd3"])
    assert np.all(new["kappa"] == KEY[0])
    assert np.all(new["incloud_time"] == 0)


def test_rhod_enters_the_multiplicity_of_a_new_super_droplet():
    """as above without aerosol_independent_of_rhod: n == int(fn(ln rd) * multiplier * rhod / rho_stp + 0.5) exactly"""
    oi = opts_2x2(lgrngn.src_t.simple, 3)
    oi.dry_distros = {KEY: spectrum(INIT, False)}
    oi.sd_conc = 32
    oi.reorder_every = -1
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, False), 16, 4)}
    p = h.hip_particles(oi)
    f = (np.full((2, 2), 300.), np.full((2, 2), .01), np.array([[1.1, 1.], [.9, .8]]))
    p.init(*f)
    n_old = p.n_part
    steps(p, opts, f, 1)
    fn = h.lognormal_fn(*SRC)
    _, _, mult = dist_analysis(fn, 16, 4., 1.)
    n, ijk, rd3, rhod = p.state_u64("n")[n_old:], p.state_u64("ijk")[n_old:], p.state_real("rd3")[n_old:], p.state_real("rhod")
    assert n.size == 32
    for ni, c, r3 in zip(n, ijk, rd3):
        v = mult * fn(math.log(r3) / 3.)
        v = v * rhod[c] / RHO_STP
        assert ni == int(v + .5)


# ------------------------------------------------------------------ 7: counter semantics and errors
def small_run(src_type=lgrngn.src_t.simple, supstp=3, **kw):
    oi = opts_2x2(src_type, 44, n_sd_max=4000)
    oi.dry_distros = {KEY: spectrum(INIT, True)}
    oi.sd_conc = 16
    for k, v in kw.items():
        setattr(oi, k, v)
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, True), 8, supstp)}
    p = h.hip_particles(oi)
    f = fields_2x2()
    p.init(*f)
    return p, opts, f


def test_counter_semantics():
    p, opts, f = small_run(supstp=3)
    seen = []
    for _ in range(8):
        steps(p, opts, f, 1)
        seen.append(p.n_part)
    grow = [b - a for a, b in zip([64] + seen[:-1], seen)]
    assert grow == [16, 0, 0, 16, 0, 0, 16, 0]                      # fires at steps 0, 3, 6
    opts.src = False
    steps(p, opts, f, 1)                                            # ... resets the counter
    assert p.n_part == seen[-1]
    opts.src = True
    steps(p, opts, f, 1)
    assert p.n_part == seen[-1] + 16


def test_box_of_zero_extent_in_x_never_fires_and_never_throws():
    p, opts, f = small_run(supstp=1, src_x0=0., src_x1=0.)
    opts.src_dry_distros = {KEY: (spectrum(SRC, True), 8, 1), (.8, 0.): (spectrum(SRC, True), 8, 1)}   # (would be an error with a box)
    steps(p, opts, f, 3)
    assert p.n_part == 64


def _raises(text, make):
    with pytest.raises(RuntimeError) as e:
        make()
    assert text in str(e.value), str(e.value)


def test_errors():
    f = fields_2x2()
    # opts.src while opts_init.src_type == off
    p, opts, _ = small_run(src_type=lgrngn.src_t.off, src_x0=0., src_x1=0.)
    _raises("aerosol source was switched off in opts_init", lambda: steps(p, opts, f, 1))
    # 0-D and 1-D
    for nx in (0, 2):
        def low_dim():
            oi = lgrngn.opts_init_t()
            oi.nx, oi.x1, oi.dt, oi.sd_conc, oi.n_sd_max = nx, max(nx, 1), 1., 8, 64
            oi.coal_switch = oi.sedi_switch = False
            oi.dry_distros = {KEY: spectrum(INIT, True)}
            oi.src_type = lgrngn.src_t.simple
            a = np.full((max(nx, 1),), 300.)
            h.hip_particles(oi).init(a, np.full_like(a, .01), np.full_like(a, 1.))
        _raises("CCN source works in 2D and 3D only.", low_dim)
    # matching with two initial kappas
    _raises("the initial aerosol distribution can only have one kappa value",
            lambda: small_run(src_type=lgrngn.src_t.matching, dry_distros={KEY: spectrum(INIT, True), (.8, 0.): spectrum(INIT, True)}))
    # matching with a source kappa that differs from the initial one
    p, opts, _ = small_run(src_type=lgrngn.src_t.matching)
    opts.src_dry_distros = {(.8, 0.): (spectrum(SRC, True), 8, 3)}
    _raises("kappa of the source has to be the same as that of the initial profile", lambda: steps(p, opts, f, 1))
    # two entries in src_dry_distros
    p, opts, _ = small_run()
    opts.src_dry_distros = {KEY: (spectrum(SRC, True), 8, 3), (.8, 0.): (spectrum(SRC, True), 8, 3)}
    _raises("src_dry_distros can only have a single kappa value.", lambda: steps(p, opts, f, 1))
    # constant multiplicity
    _raises("aerosol source and constant multiplicity option are not compatible", lambda: small_run(sd_conc=0, sd_const_multi=1000))
    # per-particle condensation substepping
    _raises("aerosol source and per-particle condensation substepping",
            lambda: small_run(exact_sstp_cond=True, sstp_cond=2))
    # relaxation stays out of scope
    _raises("option outside the accelerated hot path", lambda: small_run(rlx_switch=True))


# ------------------------------------------------------------------ 8: nothing changes when nothing fires
def full_physics_box(seed=5, **kw):
    oi = h.api_default_opts(h.box_opts(8, 8, 8, 64, rng_seed=seed))
    oi.n_sd_max = int(64 * 512 * 1.5)
    for k, v in kw.items():
        setattr(oi, k, v)
    return oi


def run_counted(oi, opts, n_steps):
    fields = h.box_fields(oi)
    th, rv, rhod, C = fields
    p = h.hip_particles(oi)
    p.init(th.copy(), rv.copy(), rhod.copy(), **C)
    th, rv = th.copy(), rv.copy()
    per_step, modes = [], []
    for _ in range(n_steps):
        l0 = p.state_u64("raw_launches").astype(np.int64)
        p.step_sync(opts, th, rv, rhod, **C)
        p.step_async(opts)
        per_step.append(tuple((p.state_u64("raw_launches").astype(np.int64) - l0).tolist()))
        modes.append(p.mode())
    state = {k: p.state_real(k) for k in ("rd3", "rw2", "x", "y", "z")}
    state.update(n=p.state_u64("n"), th=th.copy(), rv=rv.copy())
    return per_step, modes, state, p.n_part


def test_nothing_changes_when_nothing_fires():
    full = lgrngn.opts_t()
    a_steps, a_modes, a_state, a_n = run_counted(full_physics_box(), full, 6)
    src = lgrngn.opts_t()
    src.src = True
    src.src_dry_distros = {KEY: (h.lognormal_fn(*SRC), 8, 1)}
    # B: the reference's way to switch a domain's source off
    b_steps, b_modes, b_state, b_n = run_counted(full_physics_box(src_type=lgrngn.src_t.simple, src_x0=0., src_x1=0.), src, 6)
    print("launches, waits per step: A", a_steps, "B", b_steps)
    assert b_steps == a_steps and b_modes == a_modes and b_n == a_n
    for k in a_state:
        assert np.array_equal(a_state[k], b_state[k]), k
    # C: a source that fires in step 0 only
    src.src_dry_distros = {KEY: (lgrngn.lognormal(*SRC), 8, 1000)}
    oi = full_physics_box(src_type=lgrngn.src_t.simple, src_x1=8 * 40., src_y1=8 * 40., src_z1=2 * 40.)
    c_steps, c_modes, _, c_n = run_counted(oi, src, 6)
    print("C", c_steps, "n_part", c_n, "against", a_n)
    assert c_steps[1:] == a_steps[1:]
    assert c_steps[0][1] == a_steps[0][1]                           # the firing step of a built-in spectrum: no host wait of its own
    assert c_n > a_n - 200                                          # (128 source cells x 8; coalescence takes a few)
    assert c_modes == a_modes


# ------------------------------------------------------------------ 9: a run that goes on
def test_long_run_simple_counts_and_conserves():
    oi = h.box_opts(8, 8, 8, 64, rng_seed=11, reorder_every=4, periodic_topbot_walls=True, coal_switch=False)
    oi.src_type = lgrngn.src_t.simple
    oi.src_x1, oi.src_y1, oi.src_z1 = 8 * 40., 8 * 40., 2 * 40.
    per_firing = 4 * 128
    oi.n_sd_max = 64 * 512 + 20 * per_firing + 64
    opts = lgrngn.opts_t()
    opts.coal = False
    opts.src = True
    opts.src_dry_distros = {KEY: (spectrum(SRC, True), 4, 2)}
    th, rv, rhod, C = h.box_fields(oi)
    p = h.hip_particles(oi)
    p.init(th.copy(), rv.copy(), rhod.copy(), **C)
    n0 = p.n_part
    key = lambda: np.sort(p.state_u64("n").astype(np.float64) * p.state_real("rd3"))
    last = None
    for step in range(40):
        p.step_sync(opts, th, rv, rhod, **C)
        p.step_async(opts)
        assert p.n_part == n0 + (step // 2 + 1) * per_firing
        assert cell_field(p, "diag_sd_conc").sum() == p.n_part
        k = key()
        if step % 2 == 1:
            assert np.array_equal(k, last)                          # nothing dies, nothing is born between two firings
        last = k


def test_long_run_matching_with_coalescence():
    oi = h.box_opts(8, 8, 8, 64, rng_seed=12, reorder_every=4, periodic_topbot_walls=True)
    oi.dry_distros = {KEY: spectrum(INIT, True)}
    oi.src_type = lgrngn.src_t.matching
    oi.src_x1, oi.src_y1, oi.src_z1 = 8 * 40., 8 * 40., 2 * 40.
    oi.n_sd_max = 2 * 64 * 512 + 2 * 64 * 128          # (room for one firing's candidates behind what has been added)
    opts = lgrngn.opts_t()
    opts.src = True
    opts.src_dry_distros = {KEY: (spectrum(SRC, True), 64, 2)}
    th, rv, rhod, C = h.box_fields(oi)
    p = h.hip_particles(oi)
    p.init(th.copy(), rv.copy(), rhod.copy(), **C)
    dry = lambda: float((p.state_u64("n").astype(np.float64) * p.state_real("rd3")).sum())
    last = dry()
    for step in range(40):
        p.step_sync(opts, th, rv, rhod, **C)
        p.step_async(opts)
        assert cell_field(p, "diag_sd_conc").sum() == p.n_part
        now = dry()
        if step % 2 == 0:
            assert now > last                                       # a firing adds dry volume
        else:
            assert abs(now - last) <= 1e-10 * last                  # coalescence conserves it (the reference's test_coal.py:95-101)
        last = now


# ------------------------------------------------------------------ 10: the multi-device object
def multi_run(monkeypatch, multi, box):
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = lgrngn.opts_init_t()
    oi.nx, oi.nz = 4, 2
    oi.dx = oi.dz = 1.
    oi.x1, oi.z1 = 4., 2.
    oi.dt = 1.
    oi.coal_switch = oi.sedi_switch = False
    oi.dry_distros = {KEY: spectrum(INIT, True)}
    oi.sd_conc = 32
    oi.n_sd_max = 4000
    oi.dev_count = 2
    oi.src_type = lgrngn.src_t.simple
    oi.src_x0, oi.src_x1 = box
    oi.src_z0, oi.src_z1 = 0., 1.
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, True), 8, 2)}
    p = lgrngn.factory(lgrngn.backend_t.multi_HIP if multi else lgrngn.backend_t.HIP, oi)
    if multi:
        assert p.dev_count == 2
    f = (np.full((4, 2), 300.), np.full((4, 2), .01), np.full((4, 2), 1.))
    p.init(*f)
    steps(p, opts, f, 4)
    return cell_field(p, "diag_sd_conc").reshape(4, 2), p


def test_multi_device_object(monkeypatch):
    single, _ = multi_run(monkeypatch, False, (1., 3.))
    multi, _ = multi_run(monkeypatch, True, (1., 3.))
    assert np.array_equal(single[:, 0], [32, 48, 48, 32]) and np.all(single[:, 1] == 32)
    assert np.array_equal(multi, single)
    one, p = multi_run(monkeypatch, True, (2., 3.))                 # a box inside the second slab
    assert np.array_equal(one[:, 0], [32, 32, 48, 32]) and np.all(one[:, 1] == 32)
    assert p.slab(0).n_part == 2 * 2 * 32                           # the other slab's count is unchanged


# ------------------------------------------------------------------ 11: float
@pytest.mark.parametrize("seed", [44, 7])
def test_float_simple(seed):
    p, opts, f = make_distro_run(lgrngn.src_t.simple, True, seed, np.float32)
    steps(p, opts, f, 100)
    assert cell_field(p, "diag_sd_conc").tolist() == [2048., 1024., 2048., 1024.]
    assert p.n_part == 6144
    m0 = lower_over_upper(cell_field(p, "diag_wet_mom", 0))
    print("float simple seed", seed, "moment-0 ratio", m0)
    assert abs(m0 - 2.) <= 0.015
    with pytest.raises(RuntimeError, match=r"n_sd_max \(6144\) < n_part \(7168\)"):
        steps(p, opts, f, 1)


@pytest.mark.parametrize("seed", [44, 7])
def test_float_dry_sizes(seed):
    p, opts, f = make_sizes_run(seed, np.float32)
    steps(p, opts, f, 100)
    assert cell_field(p, "diag_sd_conc").tolist() == [60., 30., 60., 30.]
    m0 = lower_over_upper(cell_field(p, "diag_wet_mom", 0))
    print("float dry_sizes moment-0 ratio", m0)
    assert abs(m0 - 2.) <= 0.001
