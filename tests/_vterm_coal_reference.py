"""Terminal velocities, collision kernels, the pair probability and collide() in numpy long double (64-bit mantissa on x86-64),
written from the reference's sources (cited by file and line below; paths relative to the reference's root).  Like
tests/_diag_reference.py it imports nothing of the project and shares no line with lcx_kernels.hpp or the oracle.

What defines the operation is rounded to the object's real type T as the reference does it: the regime thresholds real_t(9.5e-6),
real_t(5.035e-4), real_t(20e-6) and Wang's knots R0[], rat[] (compared with r = the T-rounded sqrt(rw2), so that a radius "at" a threshold
is at it in every arithmetic), the table range real_t(log(5e-7)), real_t(log(3e-3)), the multiplicity real_t(n).  Where the reference
compares a real_t with a bare literal -- Long's `r_L < 50.e-6`, `r_s <= 3e-6`, Wang's `R > 100e-6`, `eps <= 2.5e-2`, Onishi's
`eps < 1e-10` -- C++ compares in DOUBLE, and so does this module: a float radius of float(50e-6) IS below 50e-6.
Everything else -- the square roots, logarithms, polynomials, products -- is long double.

Every index into a table or an array goes through _at(), which asserts that it is in range: nothing here reads past an array, and
no negative index wraps around.
"""
import numpy as np

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")


def _at(arr, idx, what):
    idx = np.asarray(idx)
    assert idx.dtype.kind in "iu", what
    assert ((idx >= 0) & (idx < len(arr))).all(), ("index out of range", what, int(idx.min()), int(idx.max()), len(arr))
    return np.asarray(arr)[idx]


def _ld(x):
    return np.asarray(x).astype(LD)


# ---- constants: include/libcloudph++/common/moist_air.hpp:26-112, const_cp.hpp:22-26, earth.hpp:16-22
c_pd = LD(1005)
M_d, M_v = LD("0.02897"), LD("0.018")
kaBoNA = LD("8.3144621")
R_d, R_v = kaBoNA / M_d, kaBoNA / M_v
p_1000 = LD(100000)
rho_w = LD(1000)
T_tri = LD("273.16")
g = LD("9.81")                                        # earth.hpp:18
p_stp = LD(101325)                                    # earth.hpp:19
T_stp = LD("273.15") + 15                             # earth.hpp:20
# earth.hpp:22: derived, p_stp / T_stp / R_d = 1.225 kg/m3, not the 1.204 of Beard (1977) (vterm.hpp:150 says so): kept, it is what the
# reference computes with
rho_stp = p_stp / T_stp / R_d
assert abs(rho_stp - LD("1.225")) < LD("5e-4")


# ---- the cell's state: include/libcloudph++/common/theta_dry.hpp:24-55, vterm.hpp:22-31 (hskpng_Tpr.ipp fills T, p, eta with these)
def T_of(th, rhod):
    return (th * (rhod * R_d / p_1000) ** (R_d / c_pd)) ** (c_pd / (c_pd - R_d))


def p_of(rhod, rv, T):
    return rhod * (R_d + rv * R_v) * T


def visc(T):
    tt = T / T_tri
    return LD("1.72e-5") * (393 / (T + 120)) * (tt * np.sqrt(tt))


def sg_surf(T):                                       # kelvin_term.hpp:25-33
    return LD("0.07275") * (1 - LD("0.002") * (T - 291))


def r_of(rw2, real_t):
    """(long-double radius, the radius as the real type holds it: what the reference's thresholds are compared with)"""
    rw2 = np.asarray(rw2, dtype=real_t)
    return np.sqrt(rw2.astype(LD)), np.sqrt(rw2).astype(real_t)


def _poly(coef, x):
    y = np.zeros_like(x)
    for i, c in enumerate(coef):
        y = y + LD(c) * x ** i
    return y


# ---- vterm.hpp:112-135
M_S = ("0.105035e2", "0.108750e1", "-0.133245", "-0.659969e-2")
M_L = ("0.65639e1", "-0.10391e1", "-0.14001e1", "-0.82736e0", "-0.34277e0", "-0.83072e-1", "-0.10583e-1", "-0.54208e-3")


def vt_beard77_v0(r, r_T):
    x = np.log(200 * r)
    small = r_T.astype(np.float64) <= 20e-6            # (vterm.hpp:127: compared in double)
    return np.where(small, np.exp(_poly(M_S, x)), np.exp(_poly(M_L, x))) / 100


# ---- vterm.hpp:140-166
def vt_beard77_fact(r, r_T, p, rhoa, eta):
    eta_0, l_0 = LD("1.818e-5"), LD("6.62e-8")
    small = r_T <= r_T.dtype.type(20e-6)
    l = l_0 * (eta / eta_0) * np.sqrt(p_stp / p * rho_stp / rhoa)
    f_s = (eta_0 / eta) * (1 + LD("1.255") * (l / r)) / (1 + LD("1.255") * (l_0 / r))
    eps_s = eta_0 / eta - 1
    eps_c = np.sqrt(rho_stp / rhoa) - 1
    f_l = LD("1.104") * eps_s + ((LD("1.058") * eps_c - LD("1.104") * eps_s) * (LD("5.52") + np.log(200 * r)) / LD("5.01")) + 1
    return np.where(small, f_s, f_l)


# ---- vterm.hpp:172-220
B_MID = ("-0.318657e1", "0.992696", "-0.153193e-2", "-0.987059e-3", "-0.578878e-3", "0.855176e-4", "-0.327815e-5")
B_BIG = ("-0.500015e1", "0.523778e1", "-0.204914e1", "0.475294", "-0.542819e-1", "0.238449e-2")


def vt_beard76(r, r_T, T, p, rhoa, eta):
    t = r_T.dtype.type
    l = LD("6.62e-8") * (eta / LD("1.818e-5")) * (p_stp / p) * np.sqrt(T / LD("293.15"))
    C_ac = 1 + LD("1.255") * l / r
    v_small = (rho_w - rhoa) * g / (LD("4.5") * eta) * C_ac * r * r
    log_N_Da = np.log(LD(32) / 3 * r * r * r * rhoa * (rho_w - rhoa) * g / eta / eta)
    v_mid = eta * (C_ac * np.exp(_poly(B_MID, log_N_Da))) / rhoa / 2 / r
    sg = sg_surf(T)
    Bo = LD(16) / 3 * r * r * (rho_w - rhoa) * g / sg
    N_p = sg * sg * sg * rhoa * rhoa / eta / eta / eta / eta / g / (rho_w - rhoa)
    N_p6 = N_p ** (LD(1) / 6)
    v_big = eta * (N_p6 * np.exp(_poly(B_BIG, np.log(Bo * N_p6)))) / rhoa / 2 / r
    return np.where(r_T <= t(9.5e-6), v_small, np.where(r_T <= t(5.035e-4), v_mid, v_big))


# ---- vterm.hpp:38-106
def vt_khvorostyanov(r, rhoa, eta, spherical):
    X = LD(32) / 3 * (rho_w - rhoa) / rhoa * g * r * r * r / eta / eta * rhoa * rhoa
    h = np.sqrt(1 + LD("0.0902") * np.sqrt(X))
    b = LD("0.0902") / 2 * np.sqrt(X) / ((h - 1) * h)
    a = LD("9.06") * LD("9.06") / 4 * (h - 1) * (h - 1) / X ** b
    if spherical:
        Av = a * (eta / rhoa * LD(1e4)) ** (1 - 2 * b) * (LD(4) / 3 * rho_w / rhoa * g * 100) ** b
    else:
        lam = LD("2.35e-3")
        ksi = np.exp(-r / lam) + (1 - np.exp(-r / lam)) / (1 + r / lam)
        alfa = PI / 6 * rho_w * ksi
        Av = a * (eta / rhoa * LD(1e4)) ** (1 - 2 * b) * (LD("2.546479") * alfa / rhoa * g * 100) ** b
    return Av * (200 * r) ** (3 * b - 1) / 100


# ---- the vt_0 table: src/detail/config.hpp:27-38, particles_impl_init_vterm.ipp:9-59, particles_impl_hskpng_vterm.ipp:16-36
VT0_N_BIN = 10000


def vt0_range(real_t):
    """ln_r_min, ln_r_max, dlnr as config_t<real_t> holds them"""
    lo, hi = real_t(np.log(np.float64(5e-7))), real_t(np.log(np.float64(3e-3)))
    return LD(lo), LD(hi), (LD(hi) - LD(lo)) / VT0_N_BIN


def vt0_bin_mids(real_t):
    lo, _, dlnr = vt0_range(real_t)
    return np.exp(lo + (np.arange(VT0_N_BIN).astype(LD) + LD("0.5")) * dlnr)


def vt0_table(real_t):
    mids = vt0_bin_mids(real_t)
    return vt_beard77_v0(mids, mids.astype(np.float64))


def vt0_bin(rw2, real_t):
    """(bin, distance to the nearer bin edge in bin widths; inf where the radius lies outside the table's range)"""
    lo, hi, dlnr = vt0_range(real_t)
    lnr = np.log(np.asarray(rw2, dtype=real_t).astype(LD)) / 2
    pos = (lnr - lo) / dlnr
    b = np.where(lnr <= lo, 0, np.where(lnr >= hi, VT0_N_BIN - 1, np.floor(np.clip(pos, 0, VT0_N_BIN))))
    frac = pos - np.floor(pos)
    margin = np.where((lnr <= lo) | (lnr >= hi), np.minimum(np.abs(lnr - lo), np.abs(lnr - hi)) / dlnr, np.minimum(frac, 1 - frac))
    b = b.astype(np.int64)
    assert ((b >= 0) & (b < VT0_N_BIN)).all()
    return b, margin


def vterm(formula, rw2, th, rv, rhod, real_t):
    """hskpng_vterm.ipp:38-129 for the super-droplets' own cells: formula = the name of the vt_t value; th, rv, rhod per droplet"""
    r, r_T = r_of(rw2, real_t)
    th, rv, rhod = _ld(th), _ld(rv), _ld(rhod)
    T = T_of(th, rhod)
    p = p_of(rhod, rv, T)
    eta = visc(T)
    if formula == "beard76":
        return vt_beard76(r, r_T, T, p, rhod, eta)
    if formula == "beard77":
        return vt_beard77_fact(r, r_T, p, rhod, eta) * vt_beard77_v0(r, r_T)
    if formula == "beard77fast":
        return vt_beard77_fact(r, r_T, p, rhod, eta) * _at(vt0_table(real_t), vt0_bin(rw2, real_t)[0], "vt_0")
    assert formula in ("khvorostyanov_spherical", "khvorostyanov_nonspherical"), formula
    return vt_khvorostyanov(r, rhod, eta, formula == "khvorostyanov_spherical")


# ---- efficiencies: src/detail/kernel_utils.hpp:10-29, kernel_interpolation.hpp:9-65
def kernel_index(R):
    R = np.asarray(R, dtype=np.int64)
    return np.where(R <= 100, R, 100 + (R - 100) // 10)


def kernel_vector_index(i, j):
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    return hi * (hi + 1) // 2 + lo


def interpolated_efficiency(table, r_max, r1, r2):
    """table: the efficiencies alone (without user parameters in front); r_max in micrometres; radii in metres"""
    r1, r2 = r1 * LD(1e6), r2 * LD(1e6)
    r_max = LD(r_max)
    r1 = np.where(r1 >= r_max, r_max - LD(1e-6), r1)
    r2 = np.where(r2 >= r_max, r_max - LD(1e-6), r2)

    def knots(r):
        coarse = r >= 100
        x0 = np.where(coarse, np.floor(r / 10) * 10, np.floor(r)).astype(np.int64)
        d = np.where(coarse, 10, 1)
        return x0, x0 + d, d
    x0, x1, dx = knots(r1)
    y0, y1, dy = knots(r2)
    e = lambda x, y: _ld(_at(table, kernel_vector_index(kernel_index(x), kernel_index(y)), "efficiency table"))
    w0, w1, w2, w3 = r1 - x0, x1 - r1, r2 - y0, y1 - r2
    return (e(x0, y0) * w1 * w3 + e(x1, y0) * w0 * w3 + e(x0, y1) * w1 * w2 + e(x1, y1) * w0 * w2) / dx / dy


# ---- src/detail/kernels.hpp:82-124
def k_geometric(nmax, rw2a, rw2b, vta, vtb):
    return PI * nmax * np.abs(vta - vtb) * (rw2a + rw2b + 2 * np.sqrt(rw2a * rw2b))


# ---- src/detail/kernel_onishi_nograv.hpp:29-153
def kernel_onishi_nograv(r1, r2, Re_l, eps, dnu, ratio_den):
    zero = np.asarray(eps, dtype=np.float64) < 1e-10             # (eps arrives as the real type holds it; compared in double, line 32)
    eps = np.where(zero, LD(1), eps)
    urms = np.sqrt(Re_l / np.sqrt(15 / dnu / eps))
    CR = r1 + r2
    taup1, taup2 = ratio_den * 4 * r1 * r1 / 18 / dnu, ratio_den * 4 * r2 * r2 / 18 / dnu
    # kernel_onishi_nograv.hpp:66: pow(dnu^3 / eps, real_t(1/4)) with an INTEGER 1/4 == 0: the Kolmogorov length is 1.  Kept, the
    # product computes what the reference computes.
    leta = LD(1)
    tauk = leta * leta / dnu
    Te = Re_l * tauk / np.sqrt(LD(15))
    theta1, theta2 = LD("2.5") * taup1 / Te, LD("2.5") * taup2 / Te
    phi = np.maximum(theta2 / theta1, theta1 / theta2)
    cw = 1 + LD("0.6") * np.exp(-(phi - 1) ** LD("1.5"))
    gamma = phi * (LD("0.183") * urms * urms / (dnu * dnu / leta / leta))
    WrS2 = (dnu * dnu * CR * CR) / leta ** 4 / 15
    WrA2 = (urms * urms * gamma / (gamma - 1)
            * ((theta1 + theta2) - 4 * theta1 * theta2 / (theta1 + theta2) * np.sqrt((1 + theta1 + theta2) / (1 + theta1) / (1 + theta2)))
            * (1 / (1 + theta1) / (1 + theta2) - 1 / (1 + gamma * theta1) / (1 + gamma * theta2)))
    WrA2 = cw * WrA2 / 3
    Wr = np.sqrt(2 / PI * (WrA2 + WrS2))
    A1, A2, A3 = LD(110), LD("0.38"), LD("0.16")
    alpha = np.maximum(np.log10(LD("0.26") * np.sqrt(Re_l)) / np.log10(LD(2)), LD("1e-20"))
    CA, CB = LD("0.06") * Re_l ** LD("0.30"), LD("0.4")
    StA = (A2 / A1 * Re_l) ** LD("0.25")
    StB = np.cbrt(A2 / A3) ** 2 * np.cbrt(Re_l)
    St1, St2 = taup1 / tauk, taup2 / tauk
    y11 = np.where(St2 <= StA, A1 * St1 * St1, 0)
    y21 = np.where(St2 <= StA, 0, A2 * Re_l / (St1 * St1))
    y31 = A3 * np.sqrt(Re_l / St1)
    y12 = np.where(St1 <= StA, A1 * St2 * St2, 0)
    y22 = np.where(St1 <= StA, 0, A2 * Re_l / (St2 * St2))
    y32 = A3 * np.sqrt(Re_l / St2)
    za1 = (1 - np.tanh((np.log10(St1) - np.log10(StA)) / CA)) / 2
    zb1 = (1 + np.tanh((np.log10(St1) - np.log10(StB)) / CB)) / 2
    za2 = (1 - np.tanh((np.log10(St2) - np.log10(StA)) / CA)) / 2
    zb2 = (1 + np.tanh((np.log10(St2) - np.log10(StB)) / CB)) / 2
    gR1 = y11 * za1 ** alpha + y21 * (1 - za1) ** alpha + y31 * zb1 + 1
    gR2 = y12 * za2 ** alpha + y22 * (1 - za2) ** alpha + y32 * zb2 + 1
    xai = np.maximum(taup2 / taup1, taup1 / taup2)
    RG12 = LD("2.6") * np.exp(-xai) + LD("0.205") * np.exp(-LD("0.0206") * xai) * (1 + np.tanh(xai - 3)) / 2
    gR = 1 + RG12 * np.sqrt(gR1 - 1) * np.sqrt(gR2 - 1)
    return np.where(zero, LD(0), 2 * PI * CR * CR * Wr * gR)


# ---- src/detail/wang_collision_enhancement.hpp:13-85
WANG_R0 = ("10e-6", "20e-6", "30e-6", "40e-6", "50e-6", "60e-6", "100e-6")
WANG_RAT = ("0", ".1", ".2", ".3", ".4", ".5", ".6", ".7", ".8", ".9", "1")
WANG_ETA = np.array([                                   # [ratio][eps class][collector radius]
    [[1.74, 1.74, 1.773, 1.49, 1.207, 1.207, 1.0], [4.976, 4.976, 3.593, 2.519, 1.445, 1.445, 1.0]],
    [[1.46, 1.46, 1.421, 1.245, 1.069, 1.069, 1.0], [2.984, 2.984, 2.181, 1.691, 1.201, 1.201, 1.0]],
    [[1.32, 1.32, 1.245, 1.123, 1.000, 1.000, 1.0], [1.988, 1.988, 1.475, 1.313, 1.150, 1.150, 1.0]],
    [[1.250, 1.250, 1.148, 1.087, 1.025, 1.025, 1.0], [1.490, 1.490, 1.187, 1.156, 1.126, 1.126, 1.0]],
    [[1.186, 1.186, 1.066, 1.060, 1.056, 1.056, 1.0], [1.249, 1.249, 1.088, 1.090, 1.092, 1.092, 1.0]],
    [[1.045, 1.045, 1.000, 1.014, 1.028, 1.028, 1.0], [1.139, 1.139, 1.130, 1.091, 1.051, 1.051, 1.0]],
    [[1.070, 1.070, 1.030, 1.038, 1.046, 1.046, 1.0], [1.220, 1.220, 1.190, 1.138, 1.086, 1.086, 1.0]],
    [[1.000, 1.000, 1.054, 1.042, 1.029, 1.029, 1.0], [1.325, 1.325, 1.267, 1.165, 1.063, 1.063, 1.0]],
    [[1.223, 1.223, 1.117, 1.069, 1.021, 1.021, 1.0], [1.716, 1.716, 1.345, 1.223, 1.100, 1.100, 1.0]],
    [[1.570, 1.570, 1.244, 1.166, 1.088, 1.088, 1.0], [3.788, 3.788, 1.501, 1.311, 1.120, 1.120, 1.0]],
    [[20.3, 20.3, 14.6, 8.61, 2.60, 2.60, 1.0], [36.52, 36.52, 19.16, 22.80, 26.0, 26.0, 1.0]]])


def wang_collision_enhancement(r1_T, r2_T, eps, real_t):
    """r1_T, r2_T: the radii as the real type holds them (the knots R0[], rat[] are real_t, and so is ratio = r / R: which knot a
    radius or a ratio is "at" is decided in the real type; the weights are long double).
    Where the reference's loops run off their arrays -- ratio == 1 leaves n_rat == 11, R == 100e-6 leaves n_R0 == 7 (lines 54-59) --
    it reads past eta_e, rat and R0: undefined behaviour.  This module, the product and the oracle clamp n_rat to 10 and n_R0 to 6,
    which is the continuous limit of what the reference computes just beside: w3 == 0 gives row 10, w1 == 0 gives column 6 (1.0)."""
    r1_T, r2_T = np.asarray(r1_T, dtype=real_t), np.asarray(r2_T, dtype=real_t)
    R_T, r_T = np.maximum(r1_T, r2_T), np.minimum(r1_T, r2_T)
    R0_T = np.array([real_t(float(x)) for x in WANG_R0])
    rat_T = np.array([real_t(float(x)) for x in WANG_RAT])
    ratio_T = (r_T / R_T).astype(real_t)
    n_eps = np.where(np.asarray(eps, dtype=real_t).astype(np.float64) <= 2.5e-2, 0, 1)           # (line 52: against a double literal)
    n_R0 = np.minimum((R0_T[None, :] <= R_T[:, None]).sum(axis=1), 6)          # first knot greater than R, clamped
    n_rat = np.minimum(1 + (rat_T[None, 1:] <= ratio_T[:, None]).sum(axis=1), 10)
    R, ratio = R_T.astype(LD), r_T.astype(LD) / R_T.astype(LD)
    R0, rat = R0_T.astype(LD), rat_T.astype(LD)
    flat = WANG_ETA.reshape(-1)

    def e(i, j):
        assert ((i >= 0) & (i < 11)).all() and ((j >= 0) & (j < 7)).all(), ("eta_e index out of range", i, j)
        return _ld(_at(flat, (i * 2 + n_eps) * 7 + j, "eta_e"))
    lo = np.maximum(n_R0 - 1, 0)                         # (not used where n_R0 == 0: the reference returns before it, line 61)
    w0, w1 = R - _at(R0, lo, "R0"), _at(R0, n_R0, "R0") - R
    w2, w3 = ratio - _at(rat, n_rat - 1, "rat"), _at(rat, n_rat, "rat") - ratio
    res = ((e(n_rat - 1, lo) * w1 * w3 + e(n_rat - 1, n_R0) * w0 * w3 + e(n_rat, lo) * w1 * w2 + e(n_rat, n_R0) * w0 * w2)
           / np.where(n_R0 == 0, LD(1), _at(R0, n_R0, "R0") - _at(R0, lo, "R0")) / (_at(rat, n_rat, "rat") - _at(rat, n_rat - 1, "rat")))
    res = np.where(n_R0 == 0, e(n_rat, n_R0), res)
    return np.where(R_T.astype(np.float64) > 100e-6, LD(1), res)                                 # (line 48: against a double literal)


# ---- every kernel: src/detail/kernels.hpp:38-250
TABULATED = ("hall", "hall_davis_no_waals", "hall_pinsky_1000mb_grav", "hall_pinsky_cumulonimbus", "hall_pinsky_stratocumulus",
             "vohl_davis_no_waals")


def kernel(name, real_t, na, nb, rw2a, rw2b, vta, vtb, params=(), table=None, r_max=None, rhod=None, eta=None, diss=None):
    """K of a pair (it carries max(na, nb), as real_t).  name: the kernel_t value's name; params: the user's kernel parameters;
    table, r_max: the efficiencies of a tabulated or Onishi kernel; rhod, eta, diss: the pair's cell (Onishi)"""
    nmax = np.maximum(np.asarray(na, dtype=np.uint64), np.asarray(nb, dtype=np.uint64)).astype(real_t).astype(LD)
    ra, ra_T = r_of(rw2a, real_t)
    rb, rb_T = r_of(rw2b, real_t)
    rw2a, rw2b, vta, vtb = (_ld(np.asarray(x, dtype=real_t)) for x in (rw2a, rw2b, vta, vtb))
    geo = k_geometric(nmax, rw2a, rw2b, vta, vtb)
    if name == "golovin":                               # kernels.hpp:50-78
        return PI * 4 / 3 * LD(real_t(params[0])) * nmax * (rw2a * ra + rw2b * rb)
    if name == "geometric":                             # kernels.hpp:96-142
        return geo * LD(real_t(params[0])) if len(params) else geo
    if name == "long":                                  # kernels.hpp:154-175
        rL, rs = np.maximum(ra, rb), np.minimum(ra, rb)
        rL_T, rs_T = np.maximum(ra_T, rb_T), np.minimum(ra_T, rb_T)
        small = geo * (LD("4.5e8") * rL * rL * (1 - LD("3e-6") / rs))
        # kernels.hpp:165,168: real_t against double literals, i.e. compared in double
        return np.where(rL_T.astype(np.float64) < 50e-6, np.where(rs_T.astype(np.float64) <= 3e-6, LD(0), small), geo)
    eff = interpolated_efficiency(table, r_max, ra, rb)
    if name in TABULATED:                               # kernels.hpp:189-201
        return eff * geo
    assert name in ("onishi_hall", "onishi_hall_davis_no_waals"), name          # kernels.hpp:222-249
    Re_l = LD(real_t(params[0]))
    rhod, eta = _ld(rhod), _ld(eta)
    nograv = kernel_onishi_nograv(ra, rb, Re_l, _ld(diss), eta / rhod, rho_w / rhod)
    # kernels.hpp:242: k_params[0], the Taylor-microscale Reynolds number, is handed to the enhancement's dissipation-rate argument
    # (the comment there calls it epsilon): kept, the product computes what the reference computes
    wang = wang_collision_enhancement(ra_T, rb_T, np.full(ra.shape, real_t(params[0])), real_t)
    return eff * wang * np.sqrt(geo * geo + nograv * nograv)


# ---- src/impl/coalescence/particles_impl_coal.ipp:99-107, 218-220
def scale_factor(N):
    N = np.asarray(N, dtype=np.int64)
    return np.where(N > 1, _ld(N * (N - 1)) / 2 / np.maximum(N // 2, 1), LD(0))


def prob(dt, dv, N_cell, K):
    return LD(dt) / _ld(dv) * scale_factor(N_cell) * K


# ---- particles_impl_coal.ipp:118-143, 243-267
def collide(na, nb, rw2a, rw2b, rd3a, rd3b, col_no):
    """col_no: the collisions drawn for the pair (before the cap).  Returns a dict: the count after the quotient cap
    min(col_no, n_big / n_small), "a_is_big" (na >= nb: the tie goes to a), the new n, rw2, rd3 of both, and "used_up" (the bigger
    one's multiplicity has become 0)."""
    na, nb, col_no = int(na), int(nb), int(col_no)
    a_big = na >= nb
    nB, nS = (na, nb) if a_big else (nb, na)
    rw2B, rw2S = (LD(rw2a), LD(rw2b)) if a_big else (LD(rw2b), LD(rw2a))
    rd3B, rd3S = (LD(rd3a), LD(rd3b)) if a_big else (LD(rd3b), LD(rd3a))
    cnt = min(col_no, nB // nS) if nS > 0 else col_no
    out = {"count": cnt, "a_is_big": a_big}
    nB_new = nB - cnt * nS
    rwS = np.cbrt(cnt * rw2B * np.sqrt(rw2B) + rw2S * np.sqrt(rw2S))
    big = (nB_new, rw2B, rd3B)
    small = (nS, rwS * rwS, cnt * rd3B + rd3S)
    (out["na"], out["rw2a"], out["rd3a"]), (out["nb"], out["rw2b"], out["rd3b"]) = (big, small) if a_big else (small, big)
    out["used_up"] = nB_new == 0
    return out
