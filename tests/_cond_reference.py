"""Condensation (step_cond with per-cell substepping) droplet by droplet in numpy long double (64-bit mantissa on x86-64), written from
the reference's sources.  It imports nothing of the project and shares no line with lcx_kernels.hpp, lcx_math.hpp or the oracle, so a
misreading that those share does not pass here.

  src/particles_step.ipp:188-267                       the order: hskpng_mfp ONCE ahead of the substeps (on the T and p the object held
                                                       before this step_sync), then per substep sstp_percell_step, hskpng_Tpr,
                                                       save_liq_ice_content_before_change, cond, update_th_rv
  src/impl/condensation/percell/sstp_percell_step.ipp  the fields' increments
  src/impl/condensation/common/particles_impl_cond_common.ipp:79-174  advance_rw2_minfun: F(x) = x0 + dt drw2_dt(x) - x
  ...cond_common.ipp:176-338                           advance_rw2: the early outs, the bracket, explicit Euler, the clamp
  src/impl/condensation/percell/particles_impl_cond.ipp:84,100  dt / sstp_cond, RH_max, config.cond_mlt
  src/impl/common/particles_impl_update_th_rv.ipp:93-168        rv -= 4/3 pi rho_w dM3;  th -= drv d_th_d_rv(T, th)
  src/detail/config.hpp:15,26,39, common/detail/toms748.hpp:262-286  n_iter, cond_mlt = 2, eps_tolerance(sizeof(real_t) * 8 / 4)
  include/libcloudph++/common/: maxwell-mason.hpp:15-47 (rdrdt), kappa_koehler.hpp:46-54 (a_w), kelvin_term.hpp:25-50,
      transition_regime.hpp:15-20 (beta), ventil.hpp:16-80 (Re, Nu, Sh, Sc, Pr), mean_free_path.hpp:16-51, theta_dry.hpp:24-65
      (T, p, d_th_d_rv), const_cp.hpp:22-43,82-86 (p_vs, l_v), moist_air.hpp:26-52,83-112, vterm.hpp:22-31 (visc)

Inputs are the values as the object's real type holds them (th, rv, rhod per cell; rw2, rd3, kappa, vt per droplet), converted exactly;
everything from there on is long double.  Out of scope: exact_sstp_cond, turb_cond, const_p, the non-default RH_formulas.
"""
import numpy as np

LD = np.longdouble

c_pd, c_pv, c_pw = LD(1005), LD(1850), LD(4218)                       # moist_air.hpp:26-28
M_d, M_v = LD("0.02897"), LD("0.018")                                 # moist_air.hpp:32-33 (M_H + M_OH)
kaBoNA = LD("8.3144621")                                              # moist_air.hpp:40
R_d, R_v = kaBoNA / M_d, kaBoNA / M_v                                 # moist_air.hpp:43-44
eps_v = M_v / M_d                                                     # moist_air.hpp:34
rho_w = LD(1000)                                                      # moist_air.hpp:50
D_0, K_0 = LD("2.26e-5"), LD("2.4e-2")                                # moist_air.hpp:91,112
p_1000 = LD(100000)                                                   # theta_std.hpp
p_tri, T_tri, l_tri = LD("611.73"), LD("273.16"), LD(2500000)         # const_cp.hpp:22-24
PI = LD("3.14159265358979323846264338327950288")
COND_MLT = LD(2)                                                      # config.hpp:26

SKIP, ZERO, AEQB, EULER, IMPLICIT = range(5)
KIND_NAMES = ("skip", "zero", "a_eq_b", "euler", "implicit")


def eps_tol(real_t):
    """toms748.hpp:272 with bits = sizeof(real_t) * 8 / 4 (config.hpp:39): 2^-15 for double, 2^-7 for float"""
    bits = np.dtype(real_t).itemsize * 2
    return max(LD(2) ** (1 - bits), 4 * LD(np.finfo(real_t).eps))


def T_of(th, rhod):                                   # theta_dry.hpp:31-35
    return (th * (rhod * R_d / p_1000) ** (R_d / c_pd)) ** (c_pd / (c_pd - R_d))


def p_of(rhod, rv, T):                                # theta_dry.hpp:52
    return rhod * (R_d + rv * R_v) * T


def p_vs(T):                                          # const_cp.hpp:39-42
    return p_tri * np.exp((l_tri + (c_pw - c_pv) * T_tri) / R_v * (1 / T_tri - 1 / T) - (c_pw - c_pv) / R_v * np.log(T / T_tri))


def RH_of(p, rv, T):                                  # RH_formula_t::pv_cc (hskpng_Tpr.ipp): moist_air::p_v (moist_air.hpp:87) / p_vs
    return p * rv / (rv + eps_v) / p_vs(T)


def visc(T):                                          # vterm.hpp:27-30
    r = T / T_tri
    return LD("1.72e-5") * (393 / (T + 120)) * (r * np.sqrt(r))


def l_v(T):                                           # const_cp.hpp:85
    return l_tri + (c_pv - c_pw) * (T - T_tri)


def lambda_D_of(T):                                   # mean_free_path.hpp:25-29
    return 2 * D_0 / np.sqrt(2 * R_v * T)


def lambda_K_of(T, p):                                # mean_free_path.hpp:46-50
    return LD("0.8") * (K_0 * T / p) / np.sqrt(2 * R_d * T)


def d_th_d_rv(T, th):                                 # theta_dry.hpp:64
    return -th / T * l_v(T) / c_pd


def kelvin_A(T):                                      # kelvin_term.hpp:28,38
    return 2 * (LD("0.07275") * (1 - LD("0.002") * (T - 291))) / R_v / T / rho_w


def rv_of_RH(RH, T, rhod):
    """the vapour mixing ratio that gives RH: p rv / (rv + eps) = rhod R_v T rv, since R_d = eps R_v"""
    return RH * p_vs(T) / (rhod * R_v * T)


def cell_fields(th, rv, rhod):
    """hskpng_Tpr with th_dry, variable pressure, pv_cc: dict of T, p, RH, eta per cell"""
    th, rv, rhod = (np.asarray(a).astype(LD).ravel() for a in (th, rv, rhod))
    T = T_of(th, rhod)
    p = p_of(rhod, rv, T)
    return {"th": th, "rv": rv, "rhod": rhod, "T": T, "p": p, "RH": RH_of(p, rv, T), "eta": visc(T)}


def mean_free_paths(held):
    """hskpng_mfp (particles_step.ipp:196) runs ahead of the first hskpng_Tpr of the step: T and p are those of the fields the object
    HELD, i.e. what the last hskpng_Tpr saw (init's fields, or the last step's after its condensation)"""
    return lambda_D_of(held["T"]), lambda_K_of(held["T"], held["p"])


class Droplets:
    """one substep's view of the droplets: per-droplet inputs of advance_rw2_minfun (cell values gathered through ijk)"""

    def __init__(self, cells, ijk, rd3, kpa, vt, lam_D, lam_K, dt, RH_max):
        g = lambda a: np.asarray(a).astype(LD)[ijk]
        self.rhod, self.rv, self.T, self.p, self.eta = (g(cells[k]) for k in ("rhod", "rv", "T", "p", "eta"))
        RH = g(cells["RH"])
        self.RH = np.where(RH > RH_max, LD(RH_max), RH)                 # cond_common.ipp:159
        self.lam_D, self.lam_K = g(lam_D), g(lam_K)
        self.rd3, self.kpa, self.vt = (np.asarray(a).astype(LD) for a in (rd3, kpa, vt))
        self.dt = LD(dt)
        rd = np.cbrt(self.rd3)
        self.rd2 = rd * rd                                              # cond_common.ipp:250-251
        lv = l_v(self.T)
        self.Sc = self.eta / self.rhod / D_0                            # ventil.hpp:67
        self.Pr = c_pd * self.eta / K_0                                 # ventil.hpp:79
        self.heat = lv / self.RH / self.T * (lv / R_v / self.T - 1)     # maxwell-mason.hpp:40-44, without the 1 / K
        self.kA = kelvin_A(self.T)

    def parts(self, x, sel=None):
        """(drw2_dt(x), the rounding scale of dt * drw2_dt(x) in units of the real type's eps, without x0 + x)"""
        s = (lambda a: a) if sel is None else (lambda a: a[sel])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            rw = np.sqrt(x)                                             # cond_common.ipp:137-138
            rw3 = rw * rw * rw
            Re = s(self.vt) * (2 * rw) * s(self.rhod) / s(self.eta)     # ventil.hpp:23
            pw = np.power(Re, LD("0.077"))                              # NaN for a negative Reynolds number (vt = -1) ...
            vent = np.where(pw > 1, pw, LD(1))                          # ... and std::max(real_t(1), NaN) is 1 (ventil.hpp:41)
            Sh = 1 + np.cbrt(1 + Re * s(self.Sc)) * vent                # ventil.hpp:41,55
            Nu = 1 + np.cbrt(1 + Re * s(self.Pr)) * vent
            beta = lambda Kn: (1 + Kn) / (1 + LD("1.71") * Kn + LD("1.33") * Kn * Kn)    # transition_regime.hpp:19
            D = D_0 * beta(s(self.lam_D) / rw) * (Sh / 2)               # cond_common.ipp:148
            K = K_0 * beta(s(self.lam_K) / rw) * (Nu / 2)               # cond_common.ipp:151
            den = 1 / D / (s(self.rhod) * s(self.rv)) + s(self.heat) / K            # maxwell-mason.hpp:35-45
            rd3 = s(self.rd3)
            A = rw3 - rd3
            B = rw3 - rd3 * (1 - s(self.kpa))
            a_w = A / B                                                 # kappa_koehler.hpp:53
            klv = np.exp(s(self.kA) / rw)                               # kelvin_term.hpp:49
            RH = s(self.RH)
            rate = 2 * ((1 - a_w * klv / RH) / rho_w / den)             # cond_common.ipp:153, maxwell-mason.hpp:33-34
            P = np.abs(2 / (rho_w * den))
            mag = self.dt * P * ((1 + np.abs(a_w * klv / RH)) + klv / RH * (rw3 + rd3) * (1 / np.abs(B) + np.abs(A) / (B * B)))
        return rate, mag

    def F(self, x0, x, sel=None):
        """advance_rw2_minfun::operator() (cond_common.ipp:169-173) and Mag(x)"""
        rate, mag = self.parts(x, sel)
        return x0 + self.dt * rate - x, x0 + x + mag


class Classes:
    pass


def classify(d, x0):
    """every droplet as advance_rw2 (cond_common.ipp:187-337) treats it: kind, drw2, the bracket [a, b], F at the bracket's far end,
    Mag at x0 and there"""
    c = Classes()
    x0 = np.asarray(x0).astype(LD)
    live = x0 > 0                                                       # cond_common.ipp:200
    xs = np.where(live, x0, LD(1))
    rate, mag0 = d.parts(xs)
    c.drw2 = d.dt * rate                                                # cond_common.ipp:204
    c.mag0 = 2 * xs + mag0
    lo2 = xs + np.minimum(LD(0), COND_MLT * c.drw2)
    c.a = np.maximum(d.rd2, lo2)                                        # cond_common.ipp:254-255
    c.b = xs + np.maximum(LD(0), COND_MLT * c.drw2)
    c.up = c.drw2 > 0
    c.far = np.where(c.up, c.b, c.a)
    c.f_far, c.mag_far = d.F(xs, c.far)                                 # cond_common.ipp:294-303: the near end's value is drw2 itself
    kind = np.full(x0.shape, IMPLICIT)
    kind[c.drw2 * c.f_far > 0] = EULER                                  # cond_common.ipp:309
    kind[c.a == c.b] = AEQB                                             # cond_common.ipp:258
    kind[c.drw2 == 0] = ZERO                                            # cond_common.ipp:242
    kind[~live] = SKIP
    c.kind = kind
    c.euler = np.maximum(xs + c.drw2, d.rd2)                            # cond_common.ipp:309,318
    c.x0 = x0
    return c


def bisect_roots(d, c):
    """a root of F in [a, b] for the implicit droplets, bisected to 2^-36 of the bracket, far inside any tolerance asked here (the others: 0)"""
    sel = np.nonzero(c.kind == IMPLICIT)[0]
    root = np.zeros(c.x0.shape, dtype=LD)
    if sel.size == 0:
        return root
    x0, lo, hi = c.x0[sel], c.a[sel].copy(), c.b[sel].copy()
    f_lo = np.where(c.up[sel], c.drw2[sel], c.f_far[sel])
    for _ in range(36):
        mid = (lo + hi) / 2
        f_mid = d.F(x0, mid, sel)[0]
        same = (f_mid > 0) == (f_lo > 0)
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    root[sel] = (lo + hi) / 2
    return root


def advance(d, x0, shift=LD(0)):
    """advance_rw2 with exact roots: the new rw2 of every droplet.  shift: the implicit droplets' roots moved by that relative amount
    inside their brackets -- any point within the root finder's tolerance of a root is an answer the reference's algorithm admits"""
    c = classify(d, x0)
    new = np.where(c.kind == EULER, c.euler, c.x0)
    root = np.minimum(np.maximum(bisect_roots(d, c) * (1 + shift), c.a), c.b)
    new = np.where(c.kind == IMPLICIT, np.maximum(root, d.rd2), new)
    return new


def cube(rw2):
    x = np.asarray(rw2).astype(LD)
    return x * np.sqrt(x)


def cell_sums(n, ijk, rw2_0, rw2_1, n_cell):
    """per cell: sum n (rw3_1 - rw3_0), S = sum n (rw3_1 + rw3_0), max |n (rw3_1 - rw3_0)|, droplets with n > 0"""
    nn = np.asarray(n).astype(LD)
    c0, c1 = cube(rw2_0), cube(rw2_1)
    term = nn * (c1 - c0)
    dM3, S, tmax = np.zeros(n_cell, dtype=LD), np.zeros(n_cell, dtype=LD), np.zeros(n_cell, dtype=LD)
    np.add.at(dM3, ijk, term)
    np.add.at(S, ijk, nn * (c1 + c0))
    np.maximum.at(tmax, ijk, np.abs(term))
    N_c = np.bincount(ijk[np.asarray(n) > 0], minlength=n_cell)
    return dM3, S, tmax, N_c


def to_drv(x, rhod, dv):
    """a cell's sum of n rw^3 as a change of rv: specific (moms_calc: / dv / rhod), times 4/3 pi rho_w (update_th_rv.ipp:93-101)"""
    return x / dv / rhod * (rho_w * (LD(4) / 3) * PI)


def substep_fields(new, old, sstp, step, cur):
    """sstp_percell_step.ipp: at substep 0 the field goes back to old + (new - old) / sstp, later substeps add (new - old) / sstp"""
    if sstp == 1:
        return cur
    inc = (new - old) / sstp
    return new - (sstp - 1) * (new - old) / sstp if step == 0 else cur + inc


def propagate(th_new, rv_new, rhod, held, n, ijk, rw2, rd3, kpa, vt, dv, dt, sstp, RH_max, shift=LD(0)):
    """the whole step_cond with exact roots: (rw2, th, rv) after sstp substeps.  held: cell_fields() of what the object held before;
    shift: see advance()"""
    n_cell = held["T"].size
    lam_D, lam_K = mean_free_paths(held)
    th_new, rv_new, rhod, dv = (np.asarray(a).astype(LD).ravel() for a in (th_new, rv_new, rhod, dv))
    th, rv = th_new, rv_new
    x = np.asarray(rw2).astype(LD)
    for step in range(sstp):
        th = substep_fields(th_new, held["th"], sstp, step, th)
        rv = substep_fields(rv_new, held["rv"], sstp, step, rv)
        cells = cell_fields(th, rv, rhod)
        d = Droplets(cells, ijk, rd3, kpa, vt, lam_D, lam_K, LD(dt) / sstp, RH_max)
        x1 = advance(d, x, shift)
        drv = to_drv(cell_sums(n, ijk, x, x1, n_cell)[0], rhod, dv)
        rv = rv - drv
        th = th - drv * d_th_d_rv(cells["T"], th)
        x = x1
    return x, th, rv
