"""The move of the super-droplets -- advection (Euler, implicit, predictor-corrector), SGS velocities, sedimentation, subsidence, the
boundary conditions with the puddle, the new cell index -- in numpy long double, written from the reference's sources
(ref: src/impl/advection/particles_impl_adve.ipp, _turb_adve.ipp, sedimentation/_sedi.ipp, subsidence/_subs.ipp,
boundary_conditions/_bcnd.ipp, housekeeping/_hskpng_ijk.ipp, initialization/_init_grid.ipp for the face maps, particles_step.ipp:127-145
for the first-order fallback).  No project code.  tests/test_oracle_move.py and tests/test_hip_move.py hold both oracle flavours and the
HIP object to it.

Every input is what the object STORES, in its real type, converted exactly; every operation here is then done once in long double, so
the result is the reference's arithmetic without its roundings.  Beside the new position the module returns, per droplet,
  mag      per coordinate, the sum of the absolute values of the terms that were added on the way (what one rounding error scales with);
           the implicit scheme's carries its conditioning 1 / |1 - (C_r - C_l)|
  wrapmag  per coordinate, |a| + |x - a| + 10 (b - a) where `periodic` was applied, else 0: (x - a) + 10 (b - a) is rounded at the ulp of
           eleven domain lengths, four bits coarser than the position
  margin   the smallest distance of a compared quantity from its threshold -- position against wall, position against cell face, the
           predicted position against a face or the clamp -- in units of eps (K_s mag + K_w wrapmag), the bar a position is held to: a droplet
           with margin <= 1 is near a decision, and move(nudge = +1 / -1) decides every comparison as if the quantity were that bar larger /
           smaller, which is the neighbouring outcome; nudge = (sx, sy, sz) does so coordinate by coordinate
  fate     stay, moved, side, top, bottom, left, right; cell (-1 where the droplet has none); n after; the four puddle terms.
"""
import numpy as np

LD = np.longdouble
FATES = ("stay", "moved", "side", "top", "bottom", "left", "right")
STAY, MOVED, SIDE, TOP, BOTTOM, LEFT, RIGHT = range(7)
EULER, IMPLICIT, PRED_CORR = "euler", "implicit", "pred_corr"
PI = LD(4) * np.arctan(LD(1))
PUDDLE = ("liq_vol", "dry_vol", "liq_num", "prtcl_num")


def effective_scheme(scheme, Cx):
    """particles_step.ipp:130-144: pred_corr falls back to first order for the step when a Courant number of the x array, halo included,
    lies beyond -2 or 2.  Returns (the scheme of the step, the distance of the nearest value from +-2)."""
    if scheme != PRED_CORR or Cx is None:
        return scheme, np.inf
    c = np.asarray(Cx).astype(LD)
    margin = float(np.min(np.abs(np.abs(c) - 2)))
    return (EULER if (c.min() < -2 or c.max() > 2) else PRED_CORR), margin


class Setup:
    """what the move reads beside the droplets.  Reals are rounded to real_t first (the object holds them so) and are long doubles from
    there.  scheme: the scheme of THIS step (effective_scheme); halo: the x planes on each side of the Courant arrays (2 where
    opts_init.adve_scheme is pred_corr, whatever this step runs); Cx, Cy, Cz: the stored arrays, flat, halo included"""

    def __init__(self, real_t, nx, ny, nz, dx, dy, dz, x0, y0, z0, x1, y1, z1, dt, scheme=EULER, halo=0, Cx=None, Cy=None, Cz=None,
                 w_LS=None, adve=True, turb=False, sedi=True, subs=False, bcnd=True, open_side_walls=False, periodic_topbot=False,
                 distmem=False, open_lft=False, open_rgt=False):
        r = lambda v: LD(real_t(v))
        self.real_t, self.eps = real_t, LD(np.finfo(real_t).eps)
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.ndims = sum(1 for n in (nx, ny, nz) if n > 0)
        self.dx, self.dy, self.dz = r(dx), r(dy), r(dz)
        self.x0, self.y0, self.z0, self.x1, self.y1, self.z1 = r(x0), r(y0), r(z0), r(x1), r(y1), r(z1)
        self.dt = r(dt)
        self.scheme, self.halo = scheme, int(halo)
        f = lambda a: None if a is None else np.asarray(a, dtype=real_t).astype(LD).ravel()
        self.Cx, self.Cy, self.Cz, self.w_LS = f(Cx), f(Cy), f(Cz), f(w_LS)
        self.adve, self.turb, self.sedi, self.subs, self.bcnd = adve, turb, sedi, subs, bcnd
        self.open_side_walls, self.periodic_topbot = bool(open_side_walls), bool(periodic_topbot)
        self.distmem, self.open_lft, self.open_rgt = bool(distmem), bool(open_lft), bool(open_rgt)

    def but(self, **kw):
        import copy
        s = copy.copy(self)
        for k, v in kw.items():
            assert hasattr(s, k), k
            setattr(s, k, v)
        return s

    def wrapped(self):
        """per coordinate: does bcnd put the position through `periodic`"""
        side = self.bcnd and not self.open_side_walls
        return (side and not self.distmem and self.nx > 0, side and self.ndims == 3, self.bcnd and self.periodic_topbot and self.ndims > 1)

    def lengths(self):
        return (self.x1 - self.x0, self.y1 - self.y0, self.z1 - self.z0)


class _Decisions:
    def __init__(self, N, nudge, K_s, K_w, eps):
        self.margin = np.full(N, np.inf)
        self.s = [LD(v) for v in (nudge if np.ndim(nudge) else (nudge,) * 3)]      # per coordinate
        self.K_s, self.K_w, self.eps = LD(K_s), LD(K_w), eps

    def bar(self, mag, wmag):
        return self.eps * (self.K_s * mag + self.K_w * wmag)

    def note(self, dist, bar, where=None):
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.minimum(np.where(bar > 0, dist / np.where(bar > 0, bar, 1), np.inf), LD(1e300)).astype(np.float64)    # (bar 0: nothing was added, nothing rounded)
        if where is not None:
            m = np.where(where, m, np.inf)
        self.margin = np.minimum(self.margin, m)

    def ge(self, ax, q, thr, mag, wmag=0, where=None):
        b = self.bar(mag, wmag)
        self.note(np.abs(q - thr), b, where)
        return q + self.s[ax] * b >= thr

    def le(self, ax, q, thr, mag, wmag=0, where=None):
        b = self.bar(mag, wmag)
        self.note(np.abs(q - thr), b, where)
        return q + self.s[ax] * b <= thr

    def cell(self, ax, x, d, mag, wmag=0):
        """hskpng_ijk.ipp:16-28: the position over the cell length, truncated"""
        b = self.bar(mag, wmag)
        i0 = np.floor(x / d)
        self.note(np.minimum(x - i0 * d, (i0 + 1) * d - x), b)
        return np.floor((x + self.s[ax] * b) / d).astype(np.int64)


def _expl(x, fl, Cl, Cr, d, apply_):
    """adve_helper_expl: (new position or increment, the magnitude of what was added to x)"""
    new = apply_ * x + (Cr - Cl) * (x - d * fl) + d * Cl
    return new, (np.abs(Cr) + np.abs(Cl)) * (np.abs(x) + d * fl) + d * np.abs(Cl)


def _impl(x, mag, fl, Cl, Cr, d):
    """adve_helper_impl: (new position, its magnitude: the numerator's terms over |D|, and the quotient's sensitivity to D = 1 - (C_r -
    C_l), whose own terms are 1, C_r and C_l)"""
    D = 1 - (Cr - Cl)
    new = (x + d * (Cl - fl * (Cr - Cl))) / D
    num = mag + d * (np.abs(Cl) + fl * (np.abs(Cr) + np.abs(Cl)))
    return new, num / np.abs(D) + np.abs(new) * (1 + np.abs(Cr) + np.abs(Cl)) / np.abs(D)


def _periodic(x, a, b):
    """bcnd.ipp:98-110; fmod keeps the sign of its first argument, so a droplet more than ten lengths to the left stays outside"""
    return a + np.fmod((x - a) + 10 * (b - a), b - a)


class Result:
    pass


def move(S, d, nudge=0, K_s=16., K_w=16.):
    """d: per storage slot n, ijk (as stored), x / y / z (those the set-up has), vt, rw2, rd3 and, with S.turb, up / vp / wp"""
    N = d["n"].size
    nx, ny, nz, nd = S.nx, S.ny, S.nz, S.ndims
    ny1, nz1 = max(ny, 1), max(nz, 1)
    g = lambda k, on: d[k].astype(LD) if on else np.zeros(N, dtype=LD)
    x, y, z = g("x", nx > 0), g("y", ny > 0), g("z", nz > 0)
    mag = [np.abs(x), np.abs(y), np.abs(z)]
    wmag = [np.zeros(N, dtype=LD) for _ in range(3)]
    dec = _Decisions(N, nudge, K_s, K_w, S.eps)
    ijk = d["ijk"].astype(np.int64)
    n0 = d["n"].astype(np.uint64)
    # unravel_ijk, hskpng_ijk.ipp:86-156
    i, j, k = (ijk // nz1) // ny1, (ijk // nz1) % ny1, ijk % nz1
    k_subs = k
    plane = 1 if nd == 1 else nz if nd == 2 else nz * ny
    rgt_off = nz * ny if nd == 3 else nz                            # init_grid.ipp:109-131 (one dimension: nz = 0, the right face IS the left one)

    def faces(c):
        """the six Courant numbers of cell c of the extended grid (init_grid.ipp:94-154)"""
        out = [S.Cx[c], S.Cx[c + rgt_off], None, None, None, None]
        if nd == 3:
            fre = c + (c // (nz * ny)) * nz
            out[2], out[3] = S.Cy[fre], S.Cy[fre + nz]
        if nd > 1:
            blw = c + c // nz if nd == 2 else c + ny * (c // (nz * ny)) + (c - (c // (nz * ny)) * (nz * ny)) // nz
            out[4], out[5] = S.Cz[blw], S.Cz[blw + 1]
        return out

    if S.adve and nd > 0 and S.scheme in (EULER, IMPLICIT):
        Cxl, Cxr, Cyl, Cyr, Czl, Czr = faces(ijk + S.halo * plane)       # adve_calc(true, halo_x)
        todo = [(0, i, Cxl, Cxr, S.dx)] + ([(1, j, Cyl, Cyr, S.dy)] if nd == 3 else []) + ([(2, k, Czl, Czr, S.dz)] if nd > 1 else [])
        pos = [x, y, z]
        for a, fl, Cl, Cr, dd in todo:
            if S.scheme == EULER:
                pos[a], add = _expl(pos[a], fl.astype(LD), Cl, Cr, dd, 1)
                mag[a] = mag[a] + add
            else:
                pos[a], mag[a] = _impl(pos[a], mag[a], fl.astype(LD), Cl, Cr, dd)
        x, y, z = pos
    elif S.adve and nd > 0:
        shift = LD(S.halo) * S.dx
        x = x + shift
        mag[0] = mag[0] + shift
        ravel = lambda a, b, c: a if nd == 1 else a * nz + c if nd == 2 else a * (nz * ny) + b * nz + c
        cells = lambda: (dec.cell(0, x, S.dx, mag[0], wmag[0]), dec.cell(1, y, S.dy, mag[1], wmag[1]) if ny else 0 * i, dec.cell(2, z, S.dz, mag[2], wmag[2]) if nz else 0 * i)
        i1, j1, k1 = cells()
        old, mag_old = [x, y, z], [m.copy() for m in mag]
        Cs = faces(ravel(i1, j1, k1))
        todo = [(0, i1, S.dx)] + ([(1, j1, S.dy)] if nd == 3 else []) + ([(2, k1, S.dz)] if nd > 1 else [])
        pos = [x, y, z]
        for a, fl, dd in todo:
            pos[a], add = _expl(pos[a], fl.astype(LD), Cs[2 * a], Cs[2 * a + 1], dd, 1)
            mag[a] = mag[a] + add
        x, y, z = pos
        if nd > 1:
            up = dec.ge(2, z, S.z1, mag[2])
            z = np.where(up, S.z1 - LD(1e-8) * S.dz, z)
            mag[2] = np.where(up, np.abs(S.z1) + LD(1e-8) * S.dz, mag[2])
            dn = dec.le(2, z, S.z0, mag[2])
            z = np.where(dn, S.z0 + LD(1e-8) * S.dz, z)
            mag[2] = np.where(dn, np.abs(S.z0) + LD(1e-8) * S.dz, mag[2])
        if nd == 3:
            L = S.y1 - S.y0
            hi = dec.ge(1, y, S.y1, mag[1])
            lo = ~dec.ge(1, y, S.y0, mag[1])
            old[1] = old[1] + np.where(hi, L, 0) - np.where(lo, L, 0)
            mag_old[1] = mag_old[1] + np.where(hi | lo, L, 0)
            wmag[1] = np.abs(S.y0) + np.abs(y - S.y0) + 10 * L
            y = _periodic(y, S.y0, S.y1)
        i2, j2, k2 = cells()
        if nd == 3:
            j2 = j2 % ny                                            # (a nudged y may sit a hair beyond a wall that `periodic` has just applied)
        k2 = np.clip(k2, 0, nz1 - 1)
        k_subs = k2
        Cs = faces(ravel(i2, j2, k2))
        half, mag_half = [x, y, z], mag
        todo = [(0, i2, S.dx)] + ([(1, j2, S.dy)] if nd == 3 else []) + ([(2, k2, S.dz)] if nd > 1 else [])
        pos, mag = [x, y, z], [m.copy() for m in mag]
        for a, fl, dd in todo:
            rhs, add = _expl(half[a], fl.astype(LD), Cs[2 * a], Cs[2 * a + 1], dd, 0)
            pos[a] = (rhs + (half[a] + old[a])) / 2
            mag[a] = (add + mag_half[a] + mag_old[a]) / 2
        x, y, z = pos
        x = x - shift
        mag[0] = mag[0] + shift
        # the wrap inside the predictor is part of y's path: its coarse rounding goes through the corrector halved
        wmag[1] = wmag[1] / 2
    if S.turb:                                                       # turb_adve.ipp:13-33
        for a, nm, on in ((0, "up", nx > 0), (1, "vp", ny > 0), (2, "wp", nz > 0)):
            if on:
                v = d[nm].astype(LD) * S.dt
                if a == 0: x = x + v
                elif a == 1: y = y + v
                else: z = z + v
                mag[a] = mag[a] + np.abs(v)
    if S.sedi and nz:
        v = S.dt * d["vt"].astype(LD)
        z = z - v
        mag[2] = mag[2] + np.abs(v)
    if S.subs and nz:
        v = S.dt * S.w_LS[k_subs]
        z = z - v
        mag[2] = mag[2] + np.abs(v)
    R = Result()
    kill_side, top, below = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    left, right = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    n_puddle = np.zeros(N, dtype=np.uint64)
    if S.bcnd and nd > 0:
        def side(ax, q, a, b, m, w):
            return dec.ge(ax, q, b, m, w) | ~dec.ge(ax, q, a, m, w)

        def wrap(q, a, b, m, w):
            arg = (q - a) + 10 * (b - a)
            ww = w + np.abs(a) + np.abs(q - a) + 10 * (b - a)
            L = b - a
            dec.note(np.abs(arg - np.round(arg / L) * L), dec.bar(m, ww))
            return _periodic(q, a, b), ww
        if not S.distmem:
            if not S.open_side_walls:
                x, wmag[0] = wrap(x, S.x0, S.x1, mag[0], wmag[0])
            else:
                kill_side |= side(0, x, S.x0, S.x1, mag[0], wmag[0])
        else:
            left = ~dec.ge(0, x, S.x0, mag[0], wmag[0])
            right = dec.ge(0, x, S.x1, mag[0], wmag[0])
            if S.open_lft: kill_side |= left
            if S.open_rgt: kill_side |= right
        if nd == 3:
            if not S.open_side_walls:
                y, wmag[1] = wrap(y, S.y0, S.y1, mag[1], wmag[1])
            else:
                kill_side |= side(1, y, S.y0, S.y1, mag[1], wmag[1])
        if nd > 1:
            if not S.periodic_topbot:
                top = dec.ge(2, z, S.z1, mag[2], wmag[2])
                below = ~dec.ge(2, z, S.z0, mag[2], wmag[2])
                n_puddle = np.where(below & ~(kill_side | top), n0, 0).astype(np.uint64)      # n as the side and top flags have left it
            else:
                z, wmag[2] = wrap(z, S.z0, S.z1, mag[2], wmag[2])
    killed = kill_side | top | below
    emig = (left | right) & ~killed
    R.x, R.y, R.z, R.mag, R.wmag = x, y, z, mag, wmag
    R.n = np.where(killed, 0, n0).astype(np.uint64)
    # the new cell, hskpng_ijk.ipp:158-200: of the droplets that keep one
    ci = dec.cell(0, x, S.dx, mag[0], wmag[0]) if nx else np.zeros(N, dtype=np.int64)
    cj = dec.cell(1, y, S.dy, mag[1], wmag[1]) if ny else np.zeros(N, dtype=np.int64)
    ck = dec.cell(2, z, S.dz, mag[2], wmag[2]) if nz else np.zeros(N, dtype=np.int64)
    wx, wy, wz = S.wrapped()
    if np.any(nudge):
        ci, cj, ck = (ci % nx if wx else ci), (cj % ny1 if wy else cj), (ck % nz1 if wz else ck)
    cell = ci if nd == 1 else ci * nz + ck if nd == 2 else ci * (nz * ny) + cj * nz + ck
    has_cell = ~killed & ~emig
    R.cell = np.where(has_cell, cell, -1)
    R.fate = np.where(kill_side, SIDE, np.where(top, TOP, np.where(below, BOTTOM, np.where(emig & left, LEFT, np.where(emig, RIGHT,
                      np.where(cell == ijk, STAY, MOVED))))))
    dec.margin = np.where(has_cell | (dec.margin < np.inf), dec.margin, np.inf)
    R.margin, R.below, R.k_subs = dec.margin, below, k_subs
    R.left, R.right = left, right                                    # bcnd.ipp:160-172 lists them whatever else happens to them
    nf = n_puddle.astype(LD)
    rw2, rd3 = d["rw2"].astype(LD), d["rd3"].astype(LD)
    R.terms = {"liq_vol": LD(4) / 3 * PI * nf * rw2 * np.sqrt(rw2), "dry_vol": LD(4) / 3 * PI * nf * rd3,
               "liq_num": np.where(rw2 == 0, 0, nf), "prtcl_num": nf}
    return R


def puddle(R, pick=None):
    """the four sums over the droplets below the floor, with the number of terms"""
    m = R.below if pick is None else R.below & pick
    return {k: (v[m].sum(dtype=LD) if m.any() else LD(0), int(m.sum())) for k, v in R.terms.items()}
