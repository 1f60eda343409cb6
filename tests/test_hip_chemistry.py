"""Aqueous chemistry on the HIP path (opts_init.chem_switch; opts.chem_dsl / chem_dsc / chem_rct).

The CPU oracle has no chemistry, so the yardsticks are numpy restatements of the reference's formulas (src/impl/chemistry/*.ipp,
common/{henry,dissoc,react,molar_mass}.hpp), written here with their own constants and fed the state that the library reports BEFORE the
step: n, ijk, rw2, rd3, the eight masses, cell T / rhod / dv and the ambient fields (the method of tests/test_hip_relaxation.py).

Bars.  Double objects, closed forms (Henry, RK4, init, dry radius, puddle, diag): rtol 1e-12, per-cell sums relative to the sum of the
absolute terms.  Float objects: the restatement is evaluated in float32 and in float64 on the same inputs and the bar is four times their
largest relative difference, computed here.  The H+ root is not restated: the electroneutrality function's root is found by bisection to
1e-14 and the library's value must lie within 2 x 4.77e-7 of it (twice the reference's eps_tolerance<float>(32))."""
import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

SP = lgrngn.chem_species_t
NAMES = ["HNO3", "NH3", "CO2", "SO2", "H2O2", "O3", "S_VI", "H"]
HNO3, NH3, CO2, SO2, H2O2, O3, S_VI, H = range(8)
GASES = range(6)
# molar_mass.hpp, dissoc.hpp, react.hpp, henry.hpp (the constants are converted to the working precision where they are used)
M = dict(SO2=64e-3, H2O2=34e-3, O3=48e-3, NH3=17e-3, HNO3=63e-3, CO2=44e-3, H=1e-3, SO2_H2O=82e-3, NH3_H2O=35e-3, NH4=18e-3,
         CO2_H2O=62e-3, H2SO4=98e-3, HSO4=97e-3)
M_GAS = [M["HNO3"], M["NH3"], M["CO2"], M["SO2"], M["H2O2"], M["O3"]]
M_AQ = [M["HNO3"], M["NH3_H2O"], M["CO2_H2O"], M["SO2_H2O"], M["H2O2"], M["O3"]]
K_H2O = 1e-14 * 1e6
K298 = dict(SO2=(1.3e-2 * 1e3, 1960.), HSO3=(6.6e-8 * 1e3, 1500.), HSO4=(1.2e-2 * 1e3, 2720.), CO2=(4.3e-7 * 1e3, -1000.),
            HCO3=(4.68e-11 * 1e3, -1760.), NH3=(1.7e-5 * 1e3, -450.), HNO3=(15.4 * 1e3, 8700.))
R298 = dict(O3_k0=(2.4e4 * 1e-3, 0.), O3_k1=(3.7e5 * 1e-3, -5530.), O3_k2=(1.5e9 * 1e-3, -5280.), H2O2_k=(7.5e7 * 1e-6, -4430.))
R_S_H2O2_K = 13. * 1e-3
P_STP, KABONA = 101325., 8.3144621
H298 = [(2.1e5 * 1e3, 8700.), (62 * 1e3, 4100.), (3.4e-2 * 1e3, 2440.), (1.23 * 1e3, 3150.), (7.45e4 * 1e3, 7300.), (1.13e-2 * 1e3, 2540.)]
D_GAS = [.6525e-4, .1978e-4, .1381e-4, .1089e-4, .8700e-4, .1444e-4]
AC_GAS = [.05, .05, .05, .035, .018, .00053]
M_D = 0.02897
# the trace gases of the kinematic chemistry case (volume mixing ratios .1, .1 ppb, 360 ppm, .2, .4, 25 ppb) as mass mixing ratios
ICICLE_GAS = [.1e-9 * M_GAS[0] / M_D, .1e-9 * M_GAS[1] / M_D, 360e-6 * M_GAS[2] / M_D, .2e-9 * M_GAS[3] / M_D, .4e-9 * M_GAS[4] / M_D, 25e-9 * M_GAS[5] / M_D]
CHEM_RHO = 1.8e3
TOL_ROOT = 2 * 4.77e-7


# ------------------------------------------------------------------------------------------ the restatement (f: the working precision)
def arrh(T, K, dKR, f):
    return f(K) * np.exp(f(dKR) * (f(1.) / T - f(1. / 298)))


def cell_factors(T, f):
    k = {n: arrh(T, v[0], v[1], f) for n, v in K298.items()}
    k.update({n: arrh(T, v[0], v[1], f) for n, v in R298.items()})
    k["H"] = [arrh(T, f(v[0]) / f(P_STP), v[1], f) for v in H298]
    k["mv"] = [np.sqrt(f(8.) / f(np.pi) * (f(KABONA) * T / f(M_GAS[g]))) for g in GASES]
    return k


def volume(rw2, f):
    return f(4. / 3) * f(np.pi) * np.power(rw2, f(3. / 2))


def dilute(m, V, k, f):
    S4, C4, N5 = m[SO2] / f(M["SO2_H2O"]) / V, m[CO2] / f(M["CO2_H2O"]) / V, m[HNO3] / f(M["HNO3"]) / V
    N3, S6, cH = m[NH3] / f(M["NH3_H2O"]) / V, m[S_VI] / f(M["H2SO4"]) / V, m[H] / f(M["H"]) / V
    with np.errstate(divide="ignore", invalid="ignore"):
        I = f(0.5) * (cH + f(K_H2O) / cH + cH * S6 / (cH + k["HSO4"]) + f(4) * k["HSO4"] * S6 / (cH + k["HSO4"]) +
                      k["CO2"] * cH * C4 / (cH * cH + k["CO2"] * cH + k["CO2"] * k["HCO3"]) +
                      f(4) * k["CO2"] * k["HCO3"] * C4 / (cH * cH + k["CO2"] * cH + k["CO2"] * k["HCO3"]) +
                      k["SO2"] * cH * S4 / (cH * cH + k["SO2"] * cH + k["SO2"] * k["HSO3"]) +
                      f(4) * k["SO2"] * k["HSO3"] * S4 / (cH * cH + k["SO2"] * cH + k["SO2"] * k["HSO3"]) +
                      k["HNO3"] * N5 / (cH + k["HNO3"]) + k["NH3"] * cH * N3 / (f(K_H2O) + k["NH3"] * cH))
    return I < f(0.02 * 1000)


def henry(g, m_old, m_H, V, rw2, T, c, rhod, dt, k, f):
    cH = m_H / f(M["H"]) / V
    if g == SO2:
        hlp = f(1) + k["SO2"] / cH + k["SO2"] * k["HSO3"] / cH / cH
    elif g == CO2:
        hlp = f(1) + k["CO2"] / cH + k["CO2"] * k["HCO3"] / cH / cH
    elif g == HNO3:
        hlp = f(1) + k["HNO3"] / cH
    elif g == NH3:
        hlp = f(1.) + k["NH3"] / f(K_H2O) * cH
    else:
        hlp = None
    Hen = k["H"][g] if hlp is None else k["H"][g] * hlp
    mt = f(1.) / (rw2 / f(3.) / f(D_GAS[g]) + f(4. / 3.) / f(AC_GAS[g]) * np.sqrt(rw2) / k["mv"][g])
    return (m_old + f(dt) * V * mt * c * rhod * (f(M_AQ[g]) / f(M_GAS[g]))) / (f(1.) + f(dt) * mt / Hen / f(KABONA) / T)


def minfun(mH, m, V, k):
    f = np.float64
    cH = mH / M["H"] / V
    dS = f(1) + k["SO2"] / cH + k["SO2"] * k["HSO3"] / cH / cH
    dC = f(1) + k["CO2"] / cH + k["CO2"] * k["HCO3"] / cH / cH
    return -mH + M["H"] * (
        K_H2O * M["H"] * (V * V) / mH
        + m[SO2] / M["SO2_H2O"] * k["SO2"] / cH / dS + 2 * m[SO2] / M["SO2_H2O"] * k["SO2"] * k["HSO3"] / cH / cH / dS
        + cH * m[S_VI] / M["H2SO4"] / (cH + k["HSO4"]) + 2 * k["HSO4"] * m[S_VI] / M["H2SO4"] / (cH + k["HSO4"])
        + m[CO2] / M["CO2_H2O"] * k["CO2"] / cH / dC + 2 * m[CO2] / M["CO2_H2O"] * k["CO2"] * k["HCO3"] / cH / cH / dC
        + m[HNO3] / M["HNO3"] * k["HNO3"] / cH / (1. + k["HNO3"] / cH)
        - m[NH3] / M["NH3_H2O"] * k["NH3"] / K_H2O * cH / (1 + k["NH3"] / K_H2O * cH))


def root_by_bisection(m, V, k):
    """the root of the electroneutrality function between 1e-8 and 10 mol / l, to 1e-14 (in float64 whatever the object's precision)"""
    a, b = 1e-8 * 1e3 * V * M["H"], 1e1 * 1e3 * V * M["H"]
    fa = minfun(a, m, V, k)
    assert np.all(fa * minfun(b, m, V, k) < 0)
    for _ in range(200):
        c = 0.5 * (a + b)
        fc = minfun(c, m, V, k)
        left = fa * fc <= 0
        b = np.where(left, c, b)
        a = np.where(left, a, c)
        fa = np.where(left, fa, fc)
    assert np.all((b - a) <= 1e-14 * a)
    return 0.5 * (a + b)


def react_rhs(x, mH, V, dt, k, f, limited=None):
    mS4, mH2O2, mO3 = x[0], x[1], x[2]
    cH = mH / f(M["H"]) / V
    diss = f(1) + k["SO2"] / cH + k["SO2"] * k["HSO3"] / cH / cH
    o3 = V * mO3 / f(M["O3"]) / V * mS4 / f(M["SO2_H2O"]) / V / diss * (k["O3_k0"] + k["O3_k1"] * k["SO2"] / cH + k["O3_k2"] * k["SO2"] * k["HSO3"] / cH / cH)
    l1 = ~(o3 * f(dt) < mO3 / f(M["O3"]))
    o3 = np.where(l1, mO3 / f(M["O3"]) / f(dt), o3)
    l2 = ~(o3 * f(dt) < mS4 / f(M["SO2_H2O"]))
    o3 = np.where(l2, mS4 / f(M["SO2_H2O"]) / f(dt), o3)
    h2 = V * k["H2O2_k"] * k["SO2"] * mH2O2 / f(M["H2O2"]) / V * mS4 / f(M["SO2_H2O"]) / V / diss / (f(1) + f(R_S_H2O2_K) * cH)
    l3 = ~(h2 * f(dt) < mH2O2 / f(M["H2O2"]))
    h2 = np.where(l3, mH2O2 / f(M["H2O2"]) / f(dt), h2)
    l4 = ~(h2 * f(dt) < mS4 / f(M["SO2_H2O"]) - o3 * f(dt))
    h2 = np.where(l4, mS4 / f(M["SO2_H2O"]) / f(dt) - o3, h2)
    if limited is not None:
        limited |= l1 | l2 | l3 | l4
    return [-(f(M["SO2_H2O"]) * (o3 + h2)), -(f(M["H2O2"]) * h2), -(f(M["O3"]) * o3), f(M["H2SO4"]) * (o3 + h2)]


def rk4(x0, mH, V, dt, k, f, limited=None):
    d = f(dt)
    k1 = react_rhs(x0, mH, V, dt, k, f, limited)
    k2 = react_rhs([x0[i] + d * f(.5) * k1[i] for i in range(4)], mH, V, dt, k, f)
    k3 = react_rhs([x0[i] + d * f(.5) * k2[i] for i in range(4)], mH, V, dt, k, f)
    k4 = react_rhs([x0[i] + d * k3[i] for i in range(4)], mH, V, dt, k, f)
    return [x0[i] + d / f(6) * k1[i] + d / f(3) * k2[i] + d / f(3) * k3[i] + d / f(6) * k4[i] for i in range(4)]


def clean(m):
    return [np.where(x >= 0, x, x * 0) for x in m]


def substep(st, dt, dsl, dsc, rct, f, amb=None, info=None, H_after_dsc=None):
    """one chemistry substep of the state `st` (masses, rw2, rd3 ... as read from the library) in precision f; amb: the cells' ambient
    mixing ratios to use (default: the state's).  Returns (masses, rd3, ambient, V, flag); dsc takes the H+ root by bisection, or, with
    H_after_dsc, the given H+ masses (the library's own root, which a caller has held to the bisection's, so that what follows the
    dissociation can be held to the closed-form bars)."""
    ijk = st["ijk"]
    T, rhod, dv = st["T"].astype(f)[ijk], st["rhod"].astype(f)[ijk], st["dv"].astype(f)
    k = cell_factors(st["T"].astype(f), f)
    k = {n: ([a[ijk] for a in v] if isinstance(v, list) else v[ijk]) for n, v in k.items()}
    m = [x.astype(f) for x in st["m"]]
    rw2, rd3, nn = st["rw2"].astype(f), st["rd3"].astype(f), st["n"].astype(f)
    amb = [a.astype(f) for a in (st["amb"] if amb is None else amb)]
    V = volume(rw2, f)
    flag = dilute(m, V, k, f)
    if dsl:
        new_amb = []
        for g in GASES:
            m_new = np.where(flag, henry(g, m[g], m[H], V, rw2, T, amb[g][ijk], rhod, dt, k, f), m[g])
            terms = nn * (m_new - m[g])
            tot = np.bincount(ijk, weights=terms.astype(np.float64), minlength=st["T"].size).astype(f)
            cnt = np.bincount(ijk, minlength=st["T"].size)
            c_new = amb[g] - tot / f(M_AQ[g]) * f(M_GAS[g]) / dv / st["rhod"].astype(f)
            c_new = np.where(c_new > 0, c_new, c_new * 0)
            if info is not None:
                info.setdefault("abs_terms", []).append(np.bincount(ijk, weights=np.abs(terms).astype(np.float64), minlength=st["T"].size)
                                                        / M_AQ[g] * M_GAS[g] / st["dv"] / st["rhod"])
                info.setdefault("clamped", []).append((c_new == 0) & (cnt > 0))
            new_amb.append(np.where(cnt > 0, c_new, amb[g]))
            m[g] = m_new
        amb = new_amb
        m = clean(m)
    if dsc:
        k64 = cell_factors(st["T"], np.float64)
        k64 = {n: ([a[ijk] for a in v] if isinstance(v, list) else v[ijk]) for n, v in k64.items()}
        m64 = [x.astype(np.float64) for x in m]
        if H_after_dsc is None:
            m[H] = np.where(flag, root_by_bisection(m64, V.astype(np.float64), k64), m64[H]).astype(f)
        else:
            m[H] = np.where(flag, np.asarray(H_after_dsc, dtype=np.float64), m64[H]).astype(f)
        m = clean(m)
    if rct:
        lim = np.zeros(rw2.shape, dtype=bool)
        x = rk4([m[SO2], m[H2O2], m[O3], m[S_VI]], m[H], V, dt, k, f, lim)
        if info is not None:
            info["limited"] = lim & flag
        rd3 = np.where(flag, rd3 + (f(3. / 4) / f(np.pi) / f(CHEM_RHO)) * (x[3] - m[S_VI]), rd3)
        for i, s in enumerate((SO2, H2O2, O3, S_VI)):
            m[s] = np.where(flag, x[i], m[s])
        m = clean(m)
    return m, rd3, amb, V, flag


# ------------------------------------------------------------------------------------------ boxes
def rv_at(RH, th, rhod):
    """the vapour mixing ratio that gives the relative humidity RH at (th, rhod), by fixed-point iteration on the library's r_vs"""
    from libcloudphxx_amd import common
    T = h.T_of(th, rhod)
    rv = 0.006
    for _ in range(30):
        rv = RH * common.r_vs(T, h.p_of(rhod, rv, T))
    return rv


# the arithmetic of an object: the parity mode that the suite pins, the API default (fast arithmetic, the reference's iterates) and the
# mode that bench.py runs; (strict_fp, cond_solver) as h.assert_mode reads them back
MODES = {"strict": (True, 0), "toms": (False, 1), "fast": (False, 0)}


def set_mode(oi, mode):
    if mode == "toms":
        h.api_default_opts(oi)
        assert (bool(oi.strict_fp), int(oi.cond_solver)) == MODES["toms"]
    else:
        oi.strict_fp, oi.cond_solver = MODES[mode]
    return oi


class Box:
    """a chemistry object, its fields and ambient arrays; stepped with condensation at slight supersaturation first.  mode: a key of
    MODES; courant: the non-zero Courant numbers of h.box_fields instead of air at rest"""

    def __init__(self, dims, sd_conc, real_t=np.float64, gases=ICICLE_GAS, cond_steps=6, empty_cell=None, mode="strict", courant=False, **kw):
        nx, nz = dims
        oi = lgrngn.opts_init_t()
        oi.nx, oi.nz = nx, nz
        oi.dx = oi.dz = 40.
        oi.x1, oi.z1 = max(nx, 1) * 40., max(nz, 1) * 40.
        oi.dt = 1.
        oi.sd_conc = sd_conc
        oi.n_sd_max = sd_conc * max(nx, 1) * max(nz, 1) + 16
        oi.dry_distros = {(.61, 0.): h.lgrngn_bimodal()}
        oi.kernel = lgrngn.kernel_t.geometric
        oi.terminal_velocity = lgrngn.vt_t.beard77fast
        oi.adve_scheme = lgrngn.as_t.euler
        oi.coal_switch = False
        oi.sedi_switch = False
        oi.chem_switch = True
        oi.chem_rho = CHEM_RHO
        for k_, v in kw.items():
            assert hasattr(oi, k_), k_
            setattr(oi, k_, v)
        set_mode(oi, mode)
        self.oi, self.f, self.mode = oi, np.dtype(real_t).type, mode
        shp = tuple(n for n in (nx, nz) if n > 0) or (1,)
        rng = np.random.default_rng(5)
        self.rhod = (1.1 - 0.01 * rng.random(shp)).astype(real_t)
        self.th = (289. + 0.2 * rng.random(shp)).astype(real_t)
        self.rv = np.array([rv_at(1.004 + 0.003 * rng.random(), t, r) for t, r in zip(self.th.ravel(), self.rhod.ravel())]).reshape(shp).astype(real_t)
        self.gas = [(g * (1 + 0.05 * rng.random(shp))).astype(real_t) for g in gases]
        self.C = {}
        if nx and nz:
            self.C = dict(Cx=np.zeros((nx + 1, nz), dtype=real_t), Cz=np.zeros((nx, nz + 1), dtype=real_t))
            if courant:
                self.C = {k_: v.astype(real_t) for k_, v in h.box_fields(oi)[3].items()}
        self.p = h.hip_particles(oi, real_t)
        self.p.init(self.th, self.rv, self.rhod, ambient_chem=self.amb(), **self.C)
        if empty_cell is not None:
            s = self.state()
            keep = s["ijk"] != empty_cell
            xs = self.p.state_real("x")[keep]
            zs = self.p.state_real("z")[keep]
            self.p.set_particles(s["n"][keep], s["rd3"][keep], s["rw2"][keep], self.p.state_real("kappa")[keep], self.p.state_real("vt")[keep], x=xs, z=zs)
        o = self.opts()
        o.cond = True
        for _ in range(cond_steps):
            self.step(o)

    def amb(self):
        return {SP(g): self.gas[g] for g in GASES}

    def opts(self, **kw):
        o = lgrngn.opts_t()
        o.adve = o.sedi = o.cond = o.coal = False
        for k_, v in kw.items():
            assert hasattr(o, k_), k_
            setattr(o, k_, v)
        return o

    def step(self, o, rhod=True, async_=True):
        self.p.step_sync(o, self.th, self.rv, self.rhod if rhod else None, ambient_chem=self.amb(), **self.C)
        if async_:
            self.p.step_async(o)

    def state(self):
        p = self.p
        return dict(n=p.state_u64("n").astype(np.float64), ijk=p.state_u64("ijk").astype(np.int64), rw2=p.state_real("rw2"), rd3=p.state_real("rd3"),
                    m=[p.state_real("chem_" + nm) for nm in NAMES], T=p.state_real("T"), rhod=p.state_real("rhod"), dv=p.state_real("dv"),
                    amb=[p.state_real("ambient_" + NAMES[g]) for g in GASES])


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.abs(b)
    d = np.abs(a - b)
    return float(np.max(np.where(den > 0, d / np.where(den > 0, den, 1), np.where(d > 0, np.inf, 0)), initial=0.))


def bar_for(real_t, r32, r64):
    """rtol 1e-12 for a double object; for a float one four times the largest relative difference of the restatement in the two precisions"""
    if np.dtype(real_t) == np.float64:
        return 1e-12
    return 4 * max(rel(a, b) for a, b in zip(r32, r64))


def sum_bar(real_t, n_terms, n_ops):
    """the bar of a per-cell sum: 1e-12 for a double object; for a float one the forward error bound of a sum of n_terms terms in any
    order followed or preceded by n_ops further roundings, (n_terms - 1 + n_ops) u with u = eps / 2, relative to the sum of the absolute
    terms -- taken twice, (n_terms + n_ops) eps, for the second-order terms and the rounding of the inputs read back in float"""
    if np.dtype(real_t) == np.float64:
        return 1e-12
    return (n_terms + n_ops) * float(np.finfo(np.float32).eps)


def both_classes(flag):
    frac = float(np.mean(flag))
    print("dilute fraction", frac)
    assert 0.1 <= frac <= 0.9, frac


BOXES = [((0, 0), 130, None), ((3, 4), 24, 5)]
REALS = [np.float64, np.float32]


def flat(seq):
    return [np.asarray(x, dtype=np.float64).ravel() for x in seq]


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("real_t", REALS)
def test_init_masses_and_diag_chem(real_t):
    """case 1: NH3, S_VI and H as NH4HSO4 of density chem_rho from rd3, the rest 0; diag_chem = sum n m / dv / rhod over the selection"""
    b = Box((3, 4), 24, real_t, cond_steps=0)
    s = b.state()
    f64, f32 = np.float64, np.float32

    def init(f):
        r = s["rd3"].astype(f)
        return [f(4. / 3) * f(np.pi) * f(CHEM_RHO) * r * (f(M[k_]) / (f(M["NH4"]) + f(M["HSO4"]))) for k_ in ("NH3_H2O", "H2SO4", "H")]
    bar = bar_for(real_t, init(f32), init(f64))
    for got, want in zip((s["m"][NH3], s["m"][S_VI], s["m"][H]), init(f64)):
        assert rel(got, want) <= bar, (rel(got, want), bar)
    for sp in (HNO3, CO2, SO2, H2O2, O3):
        assert not s["m"][sp].any()
    for sp in (NH3, S_VI, H):
        b.p.diag_all()
        b.p.diag_chem(SP(sp))
        got = b.p.outbuf_array().astype(np.float64)
        terms = s["n"] * s["m"][sp]
        want = np.bincount(s["ijk"], weights=terms, minlength=12) / s["dv"] / s["rhod"]
        tol = sum_bar(real_t, int(np.bincount(s["ijk"]).max()), 4)       # (n to real, n m, the sum, two divisions)
        assert np.all(np.abs(got - want) <= tol * np.abs(want)), (got, want)
    pud = b.p.diag_puddle()
    assert all(pud[k_] == 0 for k_ in list(pud)[:8])


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("dims,sd_conc,empty", BOXES)
def test_dissolution_alone(dims, sd_conc, empty, real_t):
    """case 2: chem_dsl -- the masses of the dilute droplets, the new ambient value per cell (an empty cell untouched), the caller's arrays,
    and the moles of gas plus dissolved form"""
    b = Box(dims, sd_conc, real_t, empty_cell=empty)
    s = b.state()
    info = {}
    m64, _, a64, V64, flag = substep(s, 1., True, False, False, np.float64, info=info)
    m32, _, a32, V32, flag32 = substep(s, 1., True, False, False, np.float32)
    both_classes(flag)
    before = [g.copy() for g in b.gas]
    b.step(b.opts(chem_dsl=True), async_=False)
    t = b.state()
    same = flag == flag32
    bar = bar_for(real_t, [x[same] for x in m32[:6]], [x[same] for x in m64[:6]])
    print("bar", bar)
    # (a float object: the droplets whose flag the restatement gives differently in the two precisions are left out, here and below)
    sel = same if real_t is np.float32 else slice(None)
    assert np.array_equal((b.p.state_real("chem_flag") != 0)[sel], flag[sel])
    vbar = bar_for(real_t, [V32], [V64])
    print("volume", rel(b.p.state_real("chem_V"), V64), vbar)
    assert rel(b.p.state_real("chem_V"), V64) <= vbar
    cnt_max = int(np.bincount(s["ijk"]).max())
    for g in GASES:
        r = rel(t["m"][g][sel], m64[g][sel])
        print(NAMES[g], "mass", r)
        assert r <= bar, (NAMES[g], r, bar)
        assert np.array_equal(t["m"][g][~flag & same], s["m"][g][~flag & same])          # the concentrated droplets keep theirs
        scale = np.abs(s["amb"][g]) + info["abs_terms"][g]
        err = np.abs(t["amb"][g] - a64[g]) / scale
        abar = 1e-12 if real_t is np.float64 else max(bar, 4 * float(np.max(np.abs(a32[g].astype(np.float64) - a64[g]) / scale)))
        print(NAMES[g], "ambient", float(err.max()), abar)
        assert err.max() <= abar
        assert np.array_equal(b.gas[g].ravel().astype(np.float64), t["amb"][g])             # the caller's array was written
        if empty is not None:
            assert t["amb"][g][empty] == before[g].ravel()[empty]
        # moles: gas (mixing ratio x rhod x dv / M_gas) + dissolved (sum n m / M_aq), per cell
        def moles(st):
            return st["amb"][g] * st["rhod"] * st["dv"] / M_GAS[g] + np.bincount(st["ijk"], weights=st["n"] * st["m"][g], minlength=st["T"].size) / M_AQ[g]
        s_amb = dict(s, amb=[x.ravel().astype(np.float64) for x in before])
        r = rel(moles(t), moles(s_amb))
        print(NAMES[g], "moles", r)
        # (float: n (m_new - m_old) two roundings, the sum, four factors and the subtraction from c -- all below the moles of the cell)
        assert r <= sum_bar(real_t, cnt_max, 7)
    for sp in (S_VI, H):
        assert np.array_equal(t["m"][sp], s["m"][sp])
    assert np.array_equal(t["rd3"], s["rd3"]) and np.array_equal(t["rw2"], s["rw2"])


@pytest.mark.parametrize("real_t", REALS)
def test_dissociation_alone(real_t):
    """case 3: chem_dsc after a few steps of dissolution -- H+ of the dilute droplets is the root of the electroneutrality function, the other
    seven masses and the ambient fields are untouched"""
    b = Box((0, 0), 130, real_t)
    for _ in range(3):
        b.step(b.opts(chem_dsl=True))
    s = b.state()
    m64, _, _, _, flag = substep(s, 1., False, True, False, np.float64)
    both_classes(flag)
    b.step(b.opts(chem_dsc=True), async_=False)
    t = b.state()
    r = rel(t["m"][H][flag], m64[H][flag])
    print("H+ root", r)
    assert r <= TOL_ROOT, r
    assert np.any(t["m"][H][flag] != s["m"][H][flag])
    assert np.array_equal(t["m"][H][~flag], s["m"][H][~flag])
    for sp in range(7):
        assert np.array_equal(t["m"][sp], s["m"][sp])
    for g in GASES:
        assert np.array_equal(t["amb"][g], s["amb"][g])


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("stress", [False, True])
def test_reaction_alone(stress, real_t):
    """case 4: chem_rct after a few steps of dissolution and dissociation -- RK4 of the oxidation, the dry radius, and per droplet
    d S_IV = - d S_VI = d (O3 + H2O2) in moles.  stress: a long step with hardly any O3, where the rate limiters engage"""
    gases = list(ICICLE_GAS)
    if stress:
        gases[O3] = 1e-13
    b = Box((3, 4), 24, real_t, gases=gases, variable_dt_switch=True)
    for _ in range(3):
        b.step(b.opts(chem_dsl=True, chem_dsc=True))
    dt = 64. if stress else 1.
    s = b.state()
    info = {}
    m64, rd64, _, _, flag = substep(s, dt, False, False, True, np.float64, info=info)
    m32, rd32, _, _, flag32 = substep(s, dt, False, False, True, np.float32)
    both_classes(flag)
    print("limited droplets", int(info["limited"].sum()))
    if stress:
        assert info["limited"].sum() >= 0.1 * flag.sum()
    b.step(b.opts(chem_rct=True, dt=dt), async_=False)
    t = b.state()
    same = (flag == flag32) if real_t is np.float32 else np.ones(flag.shape, dtype=bool)
    bar = bar_for(real_t, [x[same] for x in m32] + [rd32[same]], [x[same] for x in m64] + [rd64[same]])
    print("bar", bar)
    for sp in (SO2, H2O2, O3, S_VI):
        r = rel(t["m"][sp][same], m64[sp][same])
        print(NAMES[sp], r)
        assert r <= bar, (NAMES[sp], r, bar)
    r = rel(t["rd3"][same], rd64[same])
    print("rd3", r)
    assert r <= bar
    assert np.any(t["rd3"][flag] != s["rd3"][flag]) and np.array_equal(t["rd3"][~flag & same], s["rd3"][~flag & same])
    for sp in (HNO3, NH3, CO2, H):
        assert np.array_equal(t["m"][sp], s["m"][sp])
    # moles per droplet: what S_IV loses, S_VI gains and O3 + H2O2 lose
    d = {sp: (t["m"][sp] - s["m"][sp]) for sp in (SO2, S_VI, O3, H2O2)}
    dS4, dS6, dOx = d[SO2] / M["SO2_H2O"], d[S_VI] / M["H2SO4"], d[O3] / M["O3"] + d[H2O2] / M["H2O2"]
    scale = np.abs(s["m"][SO2] / M["SO2_H2O"]) + np.abs(dS6) + 1e-300
    # (float: a new mass is four stage terms of three roundings each and four additions, 16 roundings of u = eps / 2, each below the scale
    # of its species: 8 eps per species, taken twice for the products with the molar masses on both sides)
    eps = 1e-12 if real_t is np.float64 else 16 * float(np.finfo(np.float32).eps)
    scale6 = (np.abs(s["m"][S_VI]) + np.abs(s["m"][SO2])) / M["H2SO4"]
    assert np.all(np.abs(dS4 + dS6) <= eps * (scale + scale6)), float(np.max(np.abs(dS4 + dS6) / (scale + scale6)))
    scale_ox = np.abs(s["m"][O3] / M["O3"]) + np.abs(s["m"][H2O2] / M["H2O2"]) + scale
    assert np.all(np.abs(dS4 - dOx) <= eps * scale_ox), float(np.max(np.abs(dS4 - dOx) / scale_ox))


@pytest.mark.parametrize("real_t", REALS)
def test_clamp_at_zero_and_rate_limiters_together(real_t):
    """the box with O3 near zero, one long step of dissolution and oxidation: the droplets would take up more of the soluble gases than a
    cell holds, so the new ambient value is clamped at 0 (exactly 0 in the library's field and in the caller's array), and the rate
    limiters engage on what little O3 there is; the masses still follow the restatement"""
    gases = list(ICICLE_GAS)
    gases[O3] = 1e-13
    b = Box((3, 4), 24, real_t, gases=gases, variable_dt_switch=True, empty_cell=5)
    for _ in range(3):
        b.step(b.opts(chem_dsl=True, chem_dsc=True))
    dt = 1024.                                              # (long enough for the droplets to ask for all of a cell's HNO3)
    s = b.state()
    info, info32 = {}, {}
    m64, rd64, a64, _, flag = substep(s, dt, True, False, True, np.float64, info=info)
    m32, rd32, a32, _, flag32 = substep(s, dt, True, False, True, np.float32, info=info32)
    both_classes(flag)
    clamped = np.array(info["clamped"])
    if real_t is np.float32:                                # (a cell at the very edge may clamp in one precision only: left out)
        edge = clamped != np.array(info32["clamped"])
        clamped &= ~edge
    else:
        edge = np.zeros(clamped.shape, dtype=bool)
    print("clamped cells per gas", clamped.sum(axis=1), "limited droplets", int(info["limited"].sum()), "of", int(flag.sum()))
    assert clamped.any()
    assert info["limited"].sum() >= 0.1 * flag.sum()
    b.step(b.opts(chem_dsl=True, chem_rct=True, dt=dt), async_=False)
    t = b.state()
    for g in GASES:
        assert np.all(t["amb"][g][clamped[g]] == 0), (NAMES[g], t["amb"][g][clamped[g]])
        assert np.all(b.gas[g].ravel()[clamped[g]] == 0)
        assert np.array_equal(b.gas[g].ravel().astype(np.float64), t["amb"][g])
        assert t["amb"][g][5] == s["amb"][g][5]            # (the emptied cell keeps its value)
        free = ~clamped[g] & ~edge[g]
        scale = np.abs(s["amb"][g]) + info["abs_terms"][g]
        err = float(np.max((np.abs(t["amb"][g] - a64[g]) / scale)[free], initial=0.))
        abar = 1e-12 if real_t is np.float64 else 4 * float(np.max(np.abs(a32[g].astype(np.float64) - a64[g]) / scale))
        print(NAMES[g], "ambient", err, abar)
        assert err <= abar
    same = (flag == flag32) if real_t is np.float32 else np.ones(flag.shape, dtype=bool)
    for sp in range(7):                                     # (a bar per species: in float the O3 terms of the oxidation underflow)
        bar = bar_for(real_t, [m32[sp][same]], [m64[sp][same]])
        r = rel(t["m"][sp][same], m64[sp][same])
        print(NAMES[sp], r, bar)
        assert r <= bar, (NAMES[sp], r, bar)
    assert rel(t["rd3"][same], rd64[same]) <= bar_for(real_t, [rd32[same]], [rd64[same]])
    assert np.array_equal(t["m"][H], s["m"][H])


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("with_rhod", [True, False])
def test_substeps_of_the_ambient_fields(with_rhod, real_t):
    """case 5: sstp_chem = 3 with the ambient values changed between the steps -- each substep sees old + (k + 1) / 3 of the change; without
    rhod in sync_in only the first five gases are substepped (the reference's sstp_chem.ipp:69), the sixth jumps at once"""
    b = Box((3, 4), 24, real_t, sstp_chem=3, empty_cell=5)
    o = b.opts(chem_dsl=True)
    b.step(o, rhod=with_rhod)
    s = b.state()                                         # (ambient: what the previous step left, = sstp_tmp_chem after step_async)
    for g in GASES:
        b.gas[g] *= np.dtype(real_t).type(1.25 + 0.05 * g)
    new = [x.ravel().copy() for x in b.gas]

    def run(f):
        st = dict(s, m=[x.copy() for x in s["m"]])
        n_sub = 6 if with_rhod else 5
        old = [a.astype(f) for a in s["amb"]]
        tmp = [new[g].astype(f) - old[g] for g in GASES]
        amb = [(new[g].astype(f) - (f(3) - 1) * tmp[g] / f(3)) if g < n_sub else new[g].astype(f) for g in GASES]
        abs_terms = [np.zeros(s["T"].size) for _ in GASES]
        for step in range(3):
            if step > 0:
                amb = [(amb[g] + tmp[g] / f(3)) if g < n_sub else amb[g] for g in GASES]
            info = {}
            m, _, amb, _, _ = substep(st, 1. / 3 if f is np.float64 else np.float32(1.) / np.float32(3), True, False, False, f, amb=amb, info=info)
            st = dict(st, m=[x.astype(np.float64) for x in m])
            abs_terms = [a + b_ for a, b_ in zip(abs_terms, info["abs_terms"])]
        return st["m"], amb, abs_terms
    m64, a64, abs_terms = run(np.float64)
    b.step(o, rhod=with_rhod, async_=False)
    t = b.state()
    if real_t is np.float64:
        for g in GASES:
            r = rel(t["m"][g], m64[g])
            scale = np.abs(new[g]) + abs_terms[g]
            e = float(np.max(np.abs(t["amb"][g] - a64[g]) / scale))
            print(NAMES[g], r, e)
            assert r <= 1e-12 and e <= 1e-12, (NAMES[g], r, e)
    else:
        m32, a32, _ = run(np.float32)
        # (three substeps in float: the flag of a droplet at the threshold may differ between the precisions; such droplets are left out)
        ok = np.ones(s["rw2"].shape, dtype=bool)
        for g in GASES:
            ok &= np.abs(np.asarray(m32[g], dtype=np.float64) - m64[g]) <= 1e-3 * np.abs(m64[g])
        bar = 4 * max(rel(np.asarray(m32[g])[ok], m64[g][ok]) for g in GASES)
        for g in GASES:
            r = rel(t["m"][g][ok], m64[g][ok])
            print(NAMES[g], r, bar)
            assert r <= bar
            assert rel(t["amb"][g], a64[g]) <= max(bar, 4 * rel(a32[g], a64[g]))


def sulfur_moles(b):
    s = b.state()
    return (np.sum(s["amb"][SO2] * s["rhod"] * s["dv"]) / M["SO2"] + np.sum(s["n"] * s["m"][SO2]) / M["SO2_H2O"] + np.sum(s["n"] * s["m"][S_VI]) / M["H2SO4"])


def run_all_processes(steps=50):
    b = Box((0, 0), 130)
    o = b.opts(cond=True, chem_dsl=True, chem_dsc=True, chem_rct=True)
    s0 = sulfur_moles(b)
    for _ in range(steps):
        b.step(o)
    return b, s0


def sulfate(b):
    s = b.state()
    return float(np.sum(s["n"] * s["m"][S_VI]))


def test_sulfur_is_conserved_and_the_run_is_reproducible():
    """cases 6 and 12: all three processes with condensation, 50 steps in 0-D -- total sulfur (gas, S_IV, S_VI) in moles conserved to the
    reference's own bar of chem_coal.py, 1e-10; a second run gives the same bits"""
    b, s0 = run_all_processes()
    assert sulfate(b) > 1.0001 * sulfate(Box((0, 0), 130))      # (the oxidation did produce sulfate)
    s1 = sulfur_moles(b)
    print("sulfur", s0, s1, abs(s1 - s0) / s0)
    assert abs(s1 - s0) <= 1e-10 * s0
    st = b.state()
    b2, _ = run_all_processes()
    st2 = b2.state()
    for k_ in ("n", "rw2", "rd3", "T"):
        assert np.array_equal(st[k_], st2[k_]), k_
    for x, y in zip(st["m"] + st["amb"], st2["m"] + st2["amb"]):
        assert np.array_equal(x, y)
    assert np.array_equal(b.th, b2.th) and np.array_equal(b.rv, b2.rv)


def test_coalescence_conserves_the_masses():
    """case 7: the set-up of the reference's chem_coal.py -- 64 super-droplets, dt = 2^15, geometric kernel, 300 steps of coalescence alone:
    NH3, H and S_VI from diag_chem conserved to 1e-10"""
    oi = lgrngn.opts_init_t()
    oi.dt = 2. ** 15
    oi.sstp_coal = 1

    def expvolumelnr(lnr):
        r_zero, n_zero = 30.531e-6, 2. ** 8
        r = np.exp(lnr)
        return n_zero * 3. * np.power(r, 3) / np.power(r_zero, 3) * np.exp(-np.power((r / r_zero), 3))
    oi.dry_distros = {(.1, 0.): expvolumelnr}
    oi.sd_conc = oi.n_sd_max = 64
    oi.chem_switch = True
    oi.sedi_switch = False
    oi.chem_rho = 1.8e-3
    oi.kernel = lgrngn.kernel_t.geometric
    oi.terminal_velocity = lgrngn.vt_t.beard77fast
    th, rv, rhod = 300. * np.ones((1,)), 0.01 * np.ones((1,)), 1. * np.ones((1,))
    amb = {SP(g): np.ones((1,)) for g in GASES}
    p = h.hip_particles(oi)
    p.init(th, rv, rhod, ambient_chem=amb)
    o = lgrngn.opts_t()
    o.adve = o.sedi = o.cond = False
    o.coal = True

    def totals():
        out = []
        for sp in (NH3, H, S_VI):
            p.diag_all()
            p.diag_chem(SP(sp))
            out.append(float(p.outbuf_array()[0]))
        return out
    t0, n0 = totals(), p.n_part
    for _ in range(300):
        p.step_sync(o, th, rv, rhod, ambient_chem=amb)
        p.step_async(o)
    t1 = totals()
    print(t0, t1, n0, p.n_part)
    assert p.n_part < n0                                  # (droplets did coalesce)
    for a, c in zip(t0, t1):
        assert a > 0 and abs(c - a) <= 1e-10 * a


def tagged_masses(reorder_every, rcyc):
    """four steps of all of the chemistry without motion, then six of sedimentation with dissociation and oxidation alone: in the second
    phase, where big drops of the lowest cells fall out and the storage is compacted and re-ordered, nothing depends on the order of a
    per-cell sum, so that the bits can be compared.  (No condensation once the big drops are in: mm-sized drops with aerosol
    multiplicities are not a state to condense on.)"""
    b = Box((3, 4), 24, sedi_switch=True, dbg_flags=int(lgrngn.dbg.TAG), reorder_every=reorder_every, cond_steps=4)
    s = b.state()
    x, z = b.p.state_real("x"), b.p.state_real("z")
    # (the storage order so far depends on reorder_every: the droplets are handed back in an order of their own, by position, so that
    # both runs tag the same droplet with the same number)
    perm = np.lexsort((z, x))
    x, z = x[perm], z[perm]
    low = (z < 40.) & (np.arange(z.size) % 2 == 0)
    rw2 = np.where(low, (2e-3) ** 2, s["rw2"][perm])
    b.p.set_particles(s["n"][perm], s["rd3"][perm], rw2, b.p.state_real("kappa")[perm], b.p.state_real("vt")[perm], x=x, z=np.where(low, 1. + 0 * z, z))
    o = b.opts(chem_dsl=True, chem_dsc=True, chem_rct=True)
    for _ in range(4):
        b.step(o)
    o = b.opts(sedi=True, chem_dsc=True, chem_rct=True, rcyc=rcyc)
    for _ in range(6):
        b.step(o)
    tag = b.p.state_real("tag").astype(np.int64)
    order = np.argsort(tag, kind="stable")
    return tag[order], [b.p.state_real("chem_" + nm)[order] for nm in NAMES], int(low.sum())


def test_masses_travel_with_their_droplet():
    """case 8: the masses followed by tag are the same bits with the storage re-ordered in every step as with the storage never re-ordered;
    with recycling, a recycled super-droplet carries its donor's masses (rcyc copies them with the other attributes)"""
    t0, m0, n_big = tagged_masses(-1, False)
    t1, m1, _ = tagged_masses(1, False)
    assert n_big >= 3 and len(t0) <= 24 * 12 - n_big                # (the big drops left)
    assert np.array_equal(t0, t1)
    for a, c in zip(m0, m1):
        assert np.array_equal(a, c)
    assert np.any(m0[SO2] > 0) and np.any(m0[S_VI] > 0)
    t2, m2, _ = tagged_masses(-1, True)
    tags, cnt = np.unique(t2, return_counts=True)
    assert np.any(cnt > 1)                                          # (slots were recycled: the copy carries its donor's tag)
    for tg in tags[cnt > 1]:
        for x in m2:
            assert len(set(x[t2 == tg])) == 1


def test_puddle_takes_the_masses_of_what_falls_out():
    """case 9: puddle slots 0 ... 7 = sum n m of the super-droplets that left through the bottom"""
    b = Box((3, 4), 24, sedi_switch=True, dbg_flags=int(lgrngn.dbg.TAG), cond_steps=3)
    # big drops in the lowest cells so that they fall out within a step
    s = b.state()
    z = b.p.state_real("z")
    rw2 = s["rw2"].copy()
    low = z < 40.
    rw2[low] = (2e-3) ** 2
    z2 = np.where(low, 1., z)
    b.p.set_particles(s["n"], s["rd3"], rw2, b.p.state_real("kappa"), b.p.state_real("vt"), x=b.p.state_real("x"), z=z2)
    s = b.state()
    tag0 = b.p.state_real("tag").astype(np.int64)
    o = b.opts(sedi=True)
    b.step(o)
    left = ~np.isin(tag0, b.p.state_real("tag").astype(np.int64))
    assert left.sum() >= 3
    pud = b.p.diag_puddle()
    keys = list(pud)
    for sp in range(8):
        want = float(np.sum(s["n"][left] * s["m"][sp][left]))
        got = pud[keys[sp]]
        assert abs(got - want) <= 1e-12 * abs(want), (NAMES[sp], got, want)
    assert pud[keys[S_VI]] > 0


def test_switch_on_with_all_processes_off_changes_nothing():
    """case 10: chem_switch on and the three opts.chem_* off gives the same bits in n, rw2, rd3, th and rv as the switch off"""
    res = []
    for chem in (True, False):
        oi = h.box_opts(3, 0, 4, 24, sedi_switch=True, coal_switch=True)
        oi.chem_switch, oi.chem_rho = chem, CHEM_RHO
        th, rv, rhod, C = h.box_fields(oi, seed=3)
        rv = rv * 0.66
        p = h.hip_particles(oi)
        amb = {SP(g): np.full(th.shape, ICICLE_GAS[g]) for g in GASES} if chem else None
        p.init(th, rv, rhod, ambient_chem=amb, **C)
        o = lgrngn.opts_t()
        for _ in range(5):
            p.step_sync(o, th, rv, rhod, ambient_chem=amb, **C)
            p.step_async(o)
        res.append((p.state_u64("n"), p.state_real("rw2"), p.state_real("rd3"), th.copy(), rv.copy()))
    for a, c in zip(*res):
        assert np.array_equal(a, c)


def _raises(text, fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    assert text in str(e.value), str(e.value)


def test_error_texts():
    """case 11: the reference's texts"""
    def make(**kw):
        oi = h.box_opts(2, 0, 2, 8, coal_switch=False, sedi_switch=False)
        oi.chem_switch, oi.chem_rho = True, CHEM_RHO
        for k_, v in kw.items():
            assert hasattr(oi, k_), k_
            setattr(oi, k_, v)
        return h.hip_particles(oi)
    _raises("chemistry and aerosol source are not compatible", lambda: make(src_type=lgrngn.src_t.simple))
    _raises("CCN relaxation does not work with chemistry", lambda: make(rlx_switch=True))
    _raises("chemistry and multiple kappa distributions are not compatible",
            lambda: make(dry_distros={(.61, 0.): h.lgrngn_bimodal(), (.8, 0.): h.lgrngn_bimodal()}))
    _raises("chem_rho", lambda: make(chem_rho=0.))
    _raises("multi_CUDA is not yet compatible with chemistry", lambda: lgrngn.factory(lgrngn.backend_t.multi_HIP, _chem_oi()))
    th, rv, rhod = np.full((2, 2), 289.), np.full((2, 2), 0.006), np.full((2, 2), 1.1)
    amb = {SP(g): np.full((2, 2), ICICLE_GAS[g]) for g in GASES}
    C = dict(Cx=np.zeros((3, 2)), Cz=np.zeros((2, 3)))
    p = make()
    _raises("chemistry was not switched off and ambient_chem is empty", lambda: p.init(th, rv, rhod, **C))
    _raises("chemistry was not switched off and ambient_chem is empty", lambda: p.init(th, rv, rhod, ambient_chem={SP.SO2: amb[SP.SO2]}, **C))
    p.init(th, rv, rhod, ambient_chem=amb, **C)
    o = lgrngn.opts_t()
    o.chem_dsl = True
    _raises("chemistry was not switched off and ambient_chem is empty", lambda: p.step_sync(o, th, rv, rhod, **C))
    _raises("chemistry was not switched off and ambient_chem is empty", lambda: p.sync_in(th, rv, rhod, **C))
    p.sync_in(th, rv, rhod, ambient_chem=amb, **C)
    _raises("chemistry was not switched off and ambient_chem is empty", lambda: p.step_cond(o, th, rv))
    # an object without chemistry
    oi = h.box_opts(2, 0, 2, 8, coal_switch=False, sedi_switch=False)
    q = h.hip_particles(oi)
    _raises("chemistry was switched off and ambient_chem is not empty", lambda: q.init(th, rv, rhod, ambient_chem=amb, **C))
    q.init(th, rv, rhod, **C)
    _raises("chemistry was switched off and ambient_chem is not empty", lambda: q.step_sync(lgrngn.opts_t(), th, rv, rhod, ambient_chem=amb, **C))
    _raises("chemistry is switched off in opts_init, but diag_chem was called", lambda: q.diag_chem(SP.SO2))
    q.sync_in(th, rv, rhod, **C)
    _raises("all chemistry was switched off", lambda: q.step_cond(o, th, rv))
    # ice, and relaxation together with a source, keep their text
    _raises("option outside the accelerated hot path", lambda: make(chem_switch=False, ice_switch=True))


def _chem_oi():
    oi = h.box_opts(4, 0, 2, 8, coal_switch=False, sedi_switch=False)
    oi.chem_switch, oi.chem_rho = True, CHEM_RHO
    return oi
