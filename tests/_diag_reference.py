"""A plain statement of every diagnostic in numpy long double (64-bit mantissa on x86-64), written from the reference's
particles_diag.ipp, particles_impl_moms.ipp, particles_impl_mass_dens.ipp, particles_impl_hskpng_Tpr.ipp and its `common`
headers.  It imports nothing of the project and shares no line with lcx_kernels.hpp or the oracle, so a misreading that those two
share does not pass here.

Input: the state as read back from the object under test (a dict of arrays, see DiagRef), in whatever order the object stores it.
What defines the operation is rounded to the object's real type T exactly as the reference does it: the multiplicity T(n), the power
T(k / 3.), T(k / 2.), the thresholds T(pow(r, 3)), T(pow(r, 2)), the kernel's radius and width.  Everything else -- the pow, the
products, the sum of a cell (terms sorted by magnitude), the divisions -- is long double.

Every counting call returns, per cell, (value, sum of |term| scaled like the value, number of super-droplets of the cell in the
order): the last two are what the derived error bounds of tests/test_oracle_diagnostics.py need.
"""
import numpy as np

LD = np.longdouble

# libcloudph++/common/moist_air.hpp, const_cp.hpp, kelvin_term.hpp, theta_dry.hpp
c_pd, c_pv, c_pw = LD(1005), LD(1850), LD(4218)
M_d, M_v = LD("0.02897"), LD("0.018")
kaBoNA = LD("8.3144621")
R_d, R_v = kaBoNA / M_d, kaBoNA / M_v
eps_v = M_v / M_d
p_1000 = LD(100000)
rho_w = LD(1000)
p_tri, T_tri, l_tri = LD("611.73"), LD("273.16"), LD(2500000)


def T_of(th, rhod):                                   # theta_dry::T
    return (th * (rhod * R_d / p_1000) ** (R_d / c_pd)) ** (c_pd / (c_pd - R_d))


def p_of(rhod, rv, T):                                # theta_dry::p
    return rhod * (R_d + rv * R_v) * T


def p_vs(T):                                          # const_cp::p_vs
    return p_tri * np.exp((l_tri + (c_pw - c_pv) * T_tri) / R_v * (1 / T_tri - 1 / T) - (c_pw - c_pv) / R_v * np.log(T / T_tri))


def RH_of(p, rv, T):                                  # RH_formula_t::pv_cc: moist_air::p_v / const_cp::p_vs
    return p * rv / (rv + eps_v) / p_vs(T)


def kelvin_A(T):                                      # kelvin::A with kelvin::sg_surf
    return 2 * (LD("0.07275") * (1 - LD("0.002") * (T - 291))) / R_v / T / rho_w


def rw3_cr(rd3, kappa, T):
    """kappa_koehler::rw3_cr: the root in [rd3, 1e8 rd3] of A (rd3 - w)((kappa - 1) rd3 + w) + 3 kappa rd3 w^(4/3), here as a
    polynomial in u = w^(1/3), bisected until the bracket is one long-double ulp wide"""
    A = kelvin_A(T)

    def f(u):
        w = u * u * u
        return A * (rd3 - w) * ((kappa - 1) * rd3 + w) + 3 * kappa * rd3 * w * u
    lo = np.cbrt(rd3)
    hi = lo * np.cbrt(LD(1e8))
    assert (f(lo) > 0).all() and (f(hi) < 0).all()
    for _ in range(96):
        mid = (lo + hi) / 2
        up = f(mid) > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    u = (lo + hi) / 2
    return u * u * u


def S_cr(rd3, kappa, T):                              # kappa_koehler::S_cr = a_w(rw3_cr) * klvntrm(cbrt(rw3_cr))
    w = rw3_cr(rd3, kappa, T)
    return (w - rd3) / (w - rd3 * (1 - kappa)) * np.exp(kelvin_A(T) / np.cbrt(w))


class DiagRef:
    """st: dict with per-super-droplet arrays "n", "ijk", "rw2", "rd3", "kappa", "vt" (and "up", "vp", "wp", "incloud_time" where
    the set-up carries them), per-cell arrays "th", "rv", "rhod", "dv", and "courant_x" / "_y" / "_z" as the object stores them.
    shape: (nx, ny, nz) of opts_init (0 for a dimension that is not there); dt: opts_init.dt; real_t: the object's real type."""

    def __init__(self, st, shape, dt, real_t):
        self.T_ = real_t
        self.shape = tuple(int(s) for s in shape)
        self.n_dims = sum(1 for s in self.shape if s > 0)
        self.n_cell = int(np.prod([max(s, 1) for s in self.shape]))
        self.dt = LD(real_t(dt))
        self.n = np.asarray(st["n"], dtype=np.uint64)
        self.ijk = np.asarray(st["ijk"]).astype(np.int64)
        assert self.ijk.size == self.n.size and (self.ijk.size == 0 or self.ijk.max() < self.n_cell)
        for k, v in st.items():
            if k in ("rw2", "rd3", "kappa", "vt", "up", "vp", "wp", "incloud_time", "th", "rv", "rhod", "dv", "courant_x", "courant_y", "courant_z"):
                a = np.asarray(v)
                assert np.array_equal(a.astype(real_t).astype(np.float64), a), k     # (stored values of the real type, read back exactly)
                setattr(self, k, a.astype(LD))
        self.count = np.bincount(self.ijk, minlength=self.n_cell)              # super-droplets of a cell, n == 0 included
        self.order = np.argsort(self.ijk, kind="stable")
        self.start = np.concatenate([[0], np.cumsum(self.count)])
        self.nf = None

    # ---- cell fields (hskpng_Tpr with th_dry, !const_p, pv_cc)
    def temperature(self):
        return T_of(self.th, self.rhod)

    def pressure(self):
        return p_of(self.rhod, self.rv, self.temperature())

    def RH(self):
        return RH_of(self.pressure(), self.rv, self.temperature())

    def vel_div(self):
        """(value, sum of |term|): y, then z, then x differences of the Courant numbers of a cell's faces, each / dt"""
        nx, ny, nz = (max(s, 1) for s in self.shape)
        val = np.zeros((nx, ny, nz), dtype=LD)
        mag = np.zeros((nx, ny, nz), dtype=LD)
        if self.n_dims == 0:
            return val.ravel(), mag.ravel()

        def faces(name, ext):                          # the object keeps `halo` extra planes in x on either side: drop them
            a = getattr(self, name)
            shp = [nx, ny, nz]
            shp[ext] += 1
            per_x = shp[1] * shp[2]
            halo = (a.size // per_x - shp[0]) // 2
            assert a.size == (shp[0] + 2 * halo) * per_x
            a = a.reshape(shp[0] + 2 * halo, shp[1], shp[2])[halo:halo + shp[0]]
            sl_l, sl_r = [slice(None)] * 3, [slice(None)] * 3
            sl_l[ext], sl_r[ext] = slice(0, -1), slice(1, None)
            return a[tuple(sl_l)], a[tuple(sl_r)]
        for cond, name, ext in ((self.n_dims == 3, "courant_y", 1), (self.n_dims >= 2, "courant_z", 2), (True, "courant_x", 0)):
            if cond:
                l, r = faces(name, ext)
                val = val + (r - l) / self.dt
                mag = mag + (np.abs(r) + np.abs(l)) / self.dt
        return val.ravel(), mag.ravel()

    # ---- selections (particles_impl_moms.ipp:50-234, particles_diag.ipp:222-407): n_filtered = n or 0, in the real type
    def _thr(self, r, p):
        return LD(self.T_(LD(self.T_(r)) ** p))

    def _n(self):
        return self.n.astype(self.T_).astype(LD)

    def _sel(self, keep, cons):
        if cons:
            assert self.nf is not None
        y = self.nf if cons else self._n()
        self.nf = np.where(keep, y, LD(0))

    def all(self):
        self.nf = self._n()

    def rng(self, attr, lo, hi, cons=False):
        vec, p = {"dry": (self.rd3, 3), "wet": (self.rw2, 2), "kappa": (self.kappa, 1)}[attr]
        lo, hi = self._thr(lo, p), self._thr(hi, p)
        self._sel((vec >= lo) & (vec < hi), cons)

    def water(self, cons=False):
        self._sel(self.rw2 > 0, cons)

    def RH_minus_Sc(self):
        T = self.temperature()[self.ijk]
        return self.RH()[self.ijk] - S_cr(self.rd3, self.kappa, T), T

    def RH_ge_Sc(self):
        """returns the smallest |RH - S_cr| / S_cr of the state, for the caller's margin check"""
        d, T = self.RH_minus_Sc()
        self._sel(d >= 0, False)
        return np.min(np.abs(d) / S_cr(self.rd3, self.kappa, T)) if d.size else LD(1)

    def rc2(self):
        return rw3_cr(self.rd3, self.kappa, self.temperature()[self.ijk]) ** (LD(2) / 3)

    def rw_ge_rc(self):
        """returns the smallest |rw2 - rc2| / rc2 of the state"""
        rc2 = self.rc2()
        self._sel(self.rw2 >= rc2, False)
        return np.min(np.abs(self.rw2 - rc2) / rc2) if rc2.size else LD(1)

    # ---- counting
    def _cells(self, terms):
        val = np.zeros(self.n_cell, dtype=LD)
        mag = np.zeros(self.n_cell, dtype=LD)
        t = terms[self.order]
        for c in np.nonzero(self.count)[0]:
            seg = t[self.start[c]:self.start[c + 1]]
            seg = seg[np.argsort(np.abs(seg), kind="stable")]
            acc = LD(0)
            for v in seg:
                acc = acc + v
            val[c], mag[c] = acc, np.sum(np.abs(seg))
        return val, mag

    def _specific(self, val, mag, specific):
        if specific and self.n_dims > 0:               # (a parcel implicitly holds 1 kg of dry air)
            return val / self.dv / self.rhod, mag / self.dv / self.rhod, self.count
        return val, mag, self.count

    def sd_conc(self):
        assert self.nf is not None
        v = np.bincount(self.ijk, weights=(self.nf > 0).astype(np.float64), minlength=self.n_cell).astype(LD)
        return v, v.copy(), self.count

    def mom(self, attr, k):
        assert self.nf is not None
        vec, power = {"dry": (self.rd3, self.T_(k / 3.)), "wet": (self.rw2, self.T_(k / 2.)), "kappa": (self.kappa, self.T_(k)),
                      "incloud_time": (getattr(self, "incloud_time", None), self.T_(k)), "up": (getattr(self, "up", None), self.T_(k)),
                      "vp": (getattr(self, "vp", None), self.T_(k)), "wp": (getattr(self, "wp", None), self.T_(k))}[attr]
        assert vec is not None, attr
        return self._specific(*self._cells(self._moment_terms(vec, power)), True)

    def _moment_terms(self, x, power):                 # moment_counter: x >= 0 ? n * pow(x, xp) : n * pow(x, int(xp))
        neg = x < 0
        with np.errstate(all="ignore"):
            pos_t = np.power(np.where(neg, LD(1), x), LD(power))
        neg_t = np.where(neg, x, LD(1)) ** int(power)
        return self.nf * np.where(neg, neg_t, pos_t)

    def precip_rate(self):
        """1st non-specific moment of rw2^(3/2) * vt with the terminal velocities as the call left them"""
        assert self.nf is not None
        x = np.power(self.rw2, LD(self.T_(3. / 2))) * self.vt
        return self._specific(*self._cells(self._moment_terms(x, self.T_(1))), False)

    def wet_mass_dens(self, rad, sig0):
        """mass_dens_estimator with xp = 1/2; the kernel's width from the super-droplet count of the cell; prefactor / dv"""
        assert self.nf is not None
        rad, sig0, xp = LD(self.T_(rad)), LD(self.T_(sig0)), LD(self.T_(.5))
        sig = sig0 / np.power(self.count.astype(LD), LD(self.T_(.2)))[self.ijk]
        x = self.rw2
        with np.errstate(all="ignore"):
            t = self.nf / sig * np.power(x, 3 * xp) * np.exp(-((np.log(np.power(x, xp)) - np.log(rad)) / sig) ** 2 / 2)
        val, mag = self._cells(t)
        pref = LD(4) / 3 * rho_w * np.sqrt(2 * np.arctan(LD(1)))
        return pref * val / self.dv, pref * mag / self.dv, self.count

    def max_rw(self):
        """per cell the largest sqrt(rw2) of ALL its super-droplets, whatever is selected"""
        v = np.zeros(self.n_cell, dtype=LD)
        np.maximum.at(v, self.ijk, np.sqrt(self.rw2))
        return v
