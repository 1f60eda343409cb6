"""The move -- advection, SGS velocities, sedimentation, subsidence, boundary conditions, puddle, new cell index -- of the CPU oracle
(double and float) droplet by droplet against tests/_move_reference.py, a plain long-double statement written from the reference's
sources.  tests/test_hip_move.py runs the same cases (CASES, run_case) through the HIP object; here they prove the reference module and
the crafted inputs without a GPU and give the oracle's move a check that is not its own authors' reading.

Every case runs twice: by single stages (adve, sedi, bcnd, hskpng_ijk), each held to the reference started from what the stage before
STORED, and as one step_async with cond = coal = False.  Droplets come from set_particles and carry a unique rd3 = (id + 1) 2^-70 (exact
in float), by which they are found again whatever the storage has become.  At most 2000 droplets, never a multiple of 64, at least five
workgroups of 256.
  A   exact box, dx = dy = dz = 32, 5 x 3 x 4 / 5 x 4 / 7 cells, Courant numbers multiples of 1/4 (1/2 under the implicit scheme),
      positions multiples of 1/4: every operation is exact in float, and wherever the reference's result is a number of the real type
      the object's must be THAT number.  Droplets start on the lower walls and on interior faces, arrive exactly on every wall and face,
      stand still in a column without wind one ulp either side of the faces and walls that no `periodic` rounds (z; x and y with open
      side walls), cross exactly one and ten domain lengths to the left and one, ten and 10.9 to the right, carry n = 0, carry rw2 = 0
      through the floor, and (open side walls) leave through a side and the floor at once.  No decision escape.
  B   rounding box, dx = 37.3, dy = 41.9, dz = 23.7 (walls 2^-20 inside the last faces, see Case): Courant numbers uniform in +-0.9 with
      a few faces at +-1.9; uniform droplets and, per coordinate, a third within 1e-3 m of a face; euler, pred_corr, and implicit with
      |C| <= 0.45 but for two cells with C_r - C_l = 0.9 and -0.9 (a denominator near zero throws a droplet out of every array)
  C   pred_corr specials: a step whose Cx lies beyond 2 (first order with the halo's offset) followed by a predictor-corrector step;
      predicted z beyond top and bottom, predicted y beyond both walls; subsidence read at the predictor's level
  D   switches: open_side_walls, periodic_topbot_walls, subs, sedi off (3-D and 2-D: whole steps that carry rw2 = 0 through the floor),
      adve off, turb_adve (euler and pred_corr)
  E   a slab with two neighbours (euler, implicit) and one whose right side is open
  A*_beyond  (by stages only, no hskpng_ijk) A with every other level of the first column sent 10.9 lengths to the LEFT: the argument of
      `periodic` is negative, fmod_nonneg falls through to fmod, which keeps the sign, and the droplet is left at x < x0, alive: bit for bit.
      A whole step must not meet it: nobody defines the cell of such a droplet, and a re-indexing would count it into one.
Not covered: fmod_nonneg's upper fall-through (a million domain lengths), the invalid marker's vt and rw2 = 0 in a whole step that
sediments (the step recomputes vt, and beard76 of rw2 = 0 is 0 x infinity).  Tolerances: check_move().
"""
import itertools

import numpy as np
import pytest

import _harness as h
import _move_reference as R
from libcloudphxx_amd import lgrngn, multi

LD = np.longdouble
ORACLES = {np.float64: h.oracle_particles, np.float32: h.oracle_f32_particles}
SCHEMES = {R.EULER: lgrngn.as_t.euler, R.IMPLICIT: lgrngn.as_t.implicit, R.PRED_CORR: lgrngn.as_t.pred_corr}

# measured worsts of the CPU oracle of the same real type over all cases below, in eps mag (K_wrap: eps wrapmag), and the bar given to
# every object: 8 x that, never below 16.  K_sedi: one stage of z - dt v.  "whole": |error| of a whole step over
# its bar K_scheme eps mag + K_wrap eps wrapmag, for the record (held to 1 by construction).
MEASURED = {np.float64: {"K_euler": .936, "K_implicit": .595, "K_pred_corr": 1.063, "K_wrap": 1.822, "K_sedi": .5},
            np.float32: {"K_euler": .895, "K_implicit": .606, "K_pred_corr": 1.136, "K_wrap": 1.735, "K_sedi": .5}}
BARS = {t: {k: max(16., 8. * v) for k, v in m.items()} for t, m in MEASURED.items()}
MAX_ESCAPED = 0.01                   # share of a case's living droplets that may pass as the neighbouring outcome of a decision
K_POW = 4                            # eps of the real type per puddle term: pow(rw2, 3/2) (2), T(n), pi, the product's last rounding
DX_A, DX_B = (32., 32., 32.), (37.3, 41.9, 23.7)
CELLS = {3: (5, 3, 4), 2: (5, 0, 4), 1: (7, 0, 0)}


# ---------------------------------------------------------------------------------------------------- crafted inputs
class Case:
    """oi, the Courant numbers of every step (a list of dicts), set_particles' arguments, the opts of the step"""

    def __init__(self, real_t, dims, dxyz, scheme=R.EULER, exact=False, opts=None, staged=True, turb=False, **kw):
        nx, ny, nz = CELLS[dims]
        self.real_t, self.dims, self.exact, self.staged, self.turb = real_t, dims, exact, staged, turb
        kw.setdefault("n_sd_max", 2100)
        if turb:
            kw.update(turb_adve_switch=True, SGS_mix_len=np.linspace(20., 40., max(nz, 1)))
        oi = h.box_opts(nx, ny, nz, 2, dx=dxyz[0], dt=1., coal_switch=False, reorder_every=-1, adve_scheme=SCHEMES[scheme],
                        terminal_velocity=lgrngn.vt_t.beard76, **kw)
        if dims == 1:
            oi.sedi_switch = False                               # (init refuses sedimentation without a z)
        if ny: oi.dy, oi.y1 = dxyz[1], ny * dxyz[1]
        if nz: oi.dz, oi.z1 = dxyz[2], nz * dxyz[2]
        if not exact:
            # 5 x 37.3 is 186.5 in double and the number below it has the cell index 5 -- the hazard that hskpng_ijk.ipp:171 names.  The
            # walls of the rounding box stand 2^-20 of the domain inside the last faces (dv_eval, init_grid.ipp:46-50, admits that)
            oi.x1, oi.y1, oi.z1 = (v * (1 - 2. ** -20) if n else v for n, v in ((nx, oi.x1), (ny, oi.y1), (nz, oi.z1)))
        self.oi, self.scheme = oi, scheme
        self.shape = tuple(n for n in (nx, ny, nz) if n)
        self.opts = dict(adve=True, sedi=dims > 1, subs=False, turb_adve=turb)
        self.opts.update(opts or {})
        self.C, self.args, self.outside = [], None, False
        # no number of the real type below x1 may have the cell index nx
        for n, d, x1 in ((nx, oi.dx, oi.x1), (ny, oi.dy, oi.y1), (nz, oi.dz, oi.z1)):
            if n:
                assert int(np.float64(np.nextafter(real_t(x1), real_t(0))) / np.float64(real_t(d))) == n - 1, (n, d, x1)

    def zeros(self):
        nx, ny, nz = CELLS[self.dims]
        if self.dims == 3: return dict(Cx=np.zeros((nx + 1, ny, nz)), Cy=np.zeros((nx, ny + 1, nz)), Cz=np.zeros((nx, ny, nz + 1)))
        if self.dims == 2: return dict(Cx=np.zeros((nx + 1, nz)), Cz=np.zeros((nx, nz + 1)))
        return dict(Cx=np.zeros(nx + 1))

    def fields(self, step):
        f = lambda a: np.ascontiguousarray(a, dtype=self.real_t)
        return f(np.full(self.shape, 289.)), f(np.full(self.shape, 6.0e-3)), f(np.full(self.shape, 1.1)), {k: f(v) for k, v in self.C[step].items()}

    def finish(self, pos, n, rw2, vt):
        """set_particles' arguments from positions (N, 3) in the real type; asserts what keeps a kernel inside its arrays"""
        oi, t = self.oi, self.real_t
        N = pos.shape[0]
        assert N % 64 != 0 and 5 * 256 < N + 255 and N <= 2000, N
        for C in self.C:
            # nobody goes more than ten domain lengths to the left (`periodic` would leave the droplet outside the domain, where a cell
            # index is anybody's guess), and the implicit scheme's denominator stays away from zero
            for a, nm in enumerate(("Cx", "Cy", "Cz")):
                if nm in C:
                    assert C[nm].min() >= (-11 if self.outside and a == 0 else -10) * CELLS[self.dims][a] and np.isfinite(C[nm]).all(), nm
                    if self.scheme == R.IMPLICIT and self.dims > 1:
                        d = np.diff(C[nm], axis={"Cx": 0, "Cy": 1, "Cz": self.dims - 1}[nm])
                        assert np.abs(1 - d).min() >= .09, (nm, float(np.abs(1 - d).min()))
        args = dict(n=np.asarray(n, dtype=np.uint64), rd3=(np.arange(N) + 1.) * 2. ** -70, rw2=np.asarray(rw2, dtype=t).astype(np.float64),
                    kpa=np.full(N, .5), vt=np.asarray(vt, dtype=t).astype(np.float64))
        for a, (nm, nn, d, x1) in enumerate((("x", oi.nx, oi.dx, oi.x1), ("y", oi.ny, oi.dy, oi.y1), ("z", oi.nz, oi.dz, oi.z1))):
            if nn:
                p = pos[:, a].astype(t)
                assert (p >= 0).all() and (p < t(x1)).all() and ((p.astype(np.float64) / np.float64(t(d))).astype(np.int64) < nn).all(), nm
                args[nm] = p.astype(np.float64)
        self.args, self.N = args, N
        return self


def _radii(rng, N):
    """1 um .. 2 mm: beard76 gives 1e-4 .. 9 m/s; the staged runs take vt as given: 1e-6 .. 9 m/s, every 11th the invalid marker's -1"""
    r = np.exp(rng.uniform(np.log(1e-6), np.log(2e-3), N))
    vt = 10 ** rng.uniform(-6, np.log10(9.), N)
    vt[::11] = -1.
    return r * r, vt


def case_A(real_t, dims, scheme=R.EULER, open_walls=False, beyond=False):
    """the exact box (module docstring).  beyond: every other level of the first column goes 10.9 domain lengths to the LEFT, where the
    argument of `periodic` is negative, fmod keeps its sign and the droplet is left outside the domain, alive and without a cell: by
    stages only, and without the hskpng_ijk stage"""
    c = Case(real_t, dims, DX_A, scheme, exact=True, open_side_walls=open_walls)
    c.outside = beyond
    nx, ny, nz = CELLS[dims]
    ny1, nz1 = max(ny, 1), max(nz, 1)
    rng = np.random.default_rng(11 + dims)
    C = c.zeros()
    col = 2                                                  # the column without wind: every face of the cells i == col
    far = scheme == R.EULER and not open_walls
    if scheme == R.IMPLICIT:
        # 1 - (C_r - C_l) must divide exactly: differences of 0, 1/2 and -1 only
        ext = lambda v, a: np.asarray(v).reshape([-1 if b == a else 1 for b in range(dims)])
        C["Cx"][...] = ext([.5, 1., 0., 0., .5, .5], 0)
        C["Cy"][...] = ext([0., .5, .5, 1.], 1)
        C["Cz"][...] = ext([0., .5, .5, 1., 0.], 2)
    else:
        for nm, arr in C.items():
            arr[...] = .25 * rng.integers(-1, 2, arr.shape)
    if dims > 1:
        C["Cz"][..., 0] = 0                                    # (no flow through floor and lid)
        C["Cz"][..., nz] = 0
        C["Cz"][col] = 0
    if dims == 3:
        C["Cy"][col] = 0
    C["Cx"][col] = 0
    C["Cx"][col + 1] = 0
    if open_walls:
        C["Cx"][nx - 1] = C["Cx"][nx] = .25                    # (the last column drifts out through the right wall)
    if far:
        # whole domain lengths: the first column goes one and ten to the left, the last one, ten and 10.9 to the right, level by level
        if dims == 1:
            C["Cx"][0] = C["Cx"][1] = -76.25 if beyond else -7.
            C["Cx"][nx - 1] = C["Cx"][nx] = 70.
        else:
            for k in range(nz):
                C["Cx"][0, ..., k] = C["Cx"][1, ..., k] = (-5., -54.5 if beyond else -50.)[k % 2]
                C["Cx"][nx - 1, ..., k] = C["Cx"][nx, ..., k] = (5., 50., 54.5, 5.)[k]
    c.C = [C]
    n_cell = nx * ny1 * nz1
    per = 1216 // n_cell
    cells = np.repeat(np.arange(n_cell), per)
    N0 = cells.size
    i, j, k = (cells // nz1) // ny1, (cells // nz1) % ny1, cells % nz1
    frac = lambda: rng.integers(0, 128, N0) / 128.            # multiples of 1/4 m; 0: on the face / the lower wall
    pos = np.stack([(i + frac()) * 32., (j + frac()) * 32., (k + frac()) * 32.], axis=1)
    n = rng.integers(1, 1000, N0)
    n[::97] = 0                                               # n == 0 and not marked dead
    rw2, vt = _radii(rng, N0)
    vt = np.round(vt * 4) / 4.                                # staged runs: exact; 0 .. 9 m/s
    vt[::3] = 0.
    rw2[5::41] = 0.                                            # (liq_num leaves them out, prtcl_num does not)
    P = []                                                     # planted: (x, y, z, n, rw2, vt)

    def plant(x, y, z, vt_=0., n_=7, rw2_=1e-10):
        P.append((x, y, z, n_, rw2_, vt_))
    xc, yc = 32. * col + 16., 16.                              # inside the column without wind
    ulp = lambda v, up: float(np.nextafter(real_t(v), real_t(np.inf if up else -np.inf)))
    if dims > 1:
        for f in range(1, nz):                                 # one ulp either side of the interior z faces, and on them
            plant(xc, yc, ulp(32. * f, True)); plant(xc, yc, ulp(32. * f, False)); plant(xc, yc, 32. * f)
        plant(xc, yc, ulp(32. * nz, False))                    # one ulp below the lid
        plant(xc, yc, 0.); plant(xc, yc, float(np.finfo(real_t).tiny))
        plant(xc, yc, 8., vt_=8.)                              # arrives exactly on the floor: stays
        plant(xc, yc, 8., vt_=8.25)                            # ... a quarter below: the puddle
        plant(xc, yc, 8., vt_=8.25, rw2_=0.)                   # ... with rw2 = 0
        plant(xc, yc, 8., vt_=8.25, n_=0)                      # ... with n = 0
        plant(xc, yc, .25, vt_=8.25, rw2_=4e-6)                # a 2 mm drop just above the floor: falls through in a whole step too
        plant(xc, yc, 32. * nz - 8., vt_=-8.)                  # arrives exactly on the lid: removed
        plant(xc, yc, 32. * nz - 8., vt_=-7.75)                # ... a quarter below it: stays
    if far:                                                    # from the wall / onto a face across whole domain lengths
        for k in range(max(nz, 1)):
            plant(0., yc, 16. + 32. * k); plant(32. * (nx - 1) + 16., yc, 16. + 32. * k)
    if open_walls:
        plant(32. * nx - 4., yc, .25, vt_=8.25, rw2_=4e-6)     # through the right wall and the floor in one pass: nothing for the puddle
        plant(ulp(32. * col, True), yc, 16.); plant(ulp(32. * (col + 1), False), yc, 16.)
        if dims == 3:
            for f in range(1, ny):
                plant(xc, ulp(32. * f, True), 16.); plant(xc, ulp(32. * f, False), 16.)
            plant(xc, ulp(32. * ny, False), 16.); plant(xc, 0., 16.)
    pos = np.concatenate([pos, np.array([p[:3] for p in P]).reshape(-1, 3)])
    n = np.concatenate([n, [p[3] for p in P]])
    rw2 = np.concatenate([rw2, [p[4] for p in P]])
    vt = np.concatenate([vt, [p[5] for p in P]])
    while pos.shape[0] % 64 == 0 or pos.shape[0] % 2 == 0:   # (an odd count, no multiple of 64)
        pos, n, rw2, vt = np.vstack([pos, [xc, yc, 16.]]), np.append(n, 3), np.append(rw2, 1e-10), np.append(vt, 0.)
    return c.finish(pos, n, rw2, vt)


def _rounding_box(c, rng, N, near_share=1 / 3.):
    nx, ny, nz = CELLS[c.dims]
    oi = c.oi
    L = np.array([oi.x1, oi.y1 if ny else 1., oi.z1 if nz else 1.])
    d = np.array([oi.dx, oi.dy, oi.dz])
    pos = rng.uniform(.002, .998, (N, 3)) * L
    for a, nn in enumerate((nx, ny, nz)):
        if nn:
            near = rng.random(N) < near_share                    # 1e-5 .. 1e-3 m from a face or wall, either side; never outside the walls
            f = rng.integers(0, nn + 1, N)
            face = np.where(f == nn, L[a], f * d[a])
            off = 10 ** rng.uniform(np.where(f == nn, -4, -5), -3, N) * np.where(f == 0, 1, np.where(f == nn, -1, rng.choice([-1, 1], N)))
            pos[:, a] = np.where(near, face + off, pos[:, a])
    n = rng.integers(1, 1000, N)
    n[::97] = 0
    rw2, vt = _radii(rng, N)
    rw2[5::41] = 0.
    return pos, n, rw2, vt


def _random_courant(c, rng, amp=.9, strong=1.9):
    C = c.zeros()
    for nm, arr in C.items():
        arr[...] = rng.uniform(-amp, amp, arr.shape)
        flat = arr.reshape(-1)
        idx = rng.choice(flat.size, 4, replace=False)
        flat[idx] = strong * rng.choice([-1, 1], 4) * (1 - rng.uniform(0, .01, 4))
    C["Cx"][CELLS[c.dims][0]] = C["Cx"][0]
    return C


def case_B(real_t, dims, scheme):
    c = Case(real_t, dims, DX_B, scheme)
    rng = np.random.default_rng({R.EULER: 21, R.IMPLICIT: 22, R.PRED_CORR: 23}[scheme] + 10 * dims)
    # (implicit: |C| <= 0.45 keeps 1 - (C_r - C_l) above 0.1 everywhere but in the two cells made for it)
    C = _random_courant(c, rng, amp=.45, strong=.45) if scheme == R.IMPLICIT else _random_courant(c, rng)
    if scheme == R.IMPLICIT:                                   # two cells with C_r - C_l = 0.9 and -0.9 (1 / (1 - 0.9): the conditioning)
        sl = (slice(None),) * (dims - 1)
        C["Cx"][2][sl], C["Cx"][3][sl], C["Cx"][4][sl] = -.2, .7, -.2
    c.C = [C]
    return c.finish(*_rounding_box(c, rng, 1531))


def case_C(real_t, dims, which):
    """fallback: step 0 has Cx = 2.5 on the wall's pair of faces (so in the halo too): first order with the halo's offset; step 1 is a
    predictor-corrector step again.  clamps: strong Cz towards lid and floor, strong Cy towards both walls, subsidence on"""
    kw = dict(subs_switch=True, w_LS=np.linspace(-.5, 1.5, CELLS[dims][2])) if which == "clamps" else {}
    c = Case(real_t, dims, DX_B, R.PRED_CORR, opts=dict(subs=which == "clamps"), staged=which != "clamps", **kw)
    nx, ny, nz = CELLS[dims]
    rng = np.random.default_rng(31 + dims + (7 if which == "clamps" else 0))
    C = _random_courant(c, rng, amp=.6, strong=1.2)
    if which == "fallback":
        C0 = {k: v.copy() for k, v in C.items()}
        C0["Cx"][0] = C0["Cx"][nx] = 2.5
        c.C = [C0, C]
    else:
        C["Cz"][..., nz] = rng.uniform(1.2, 1.6, C["Cz"][..., nz].shape)
        C["Cz"][..., nz - 1] = rng.uniform(.8, 1.2, C["Cz"][..., nz].shape)
        C["Cz"][..., 0] = rng.uniform(-1.6, -1.2, C["Cz"][..., 0].shape)
        C["Cz"][..., 1] = rng.uniform(-1.2, -.8, C["Cz"][..., 0].shape)
        if dims == 3:
            C["Cy"][:, ny] = C["Cy"][:, 0] = rng.uniform(1.2, 1.6, C["Cy"][:, 0].shape) * np.where(np.arange(nz) % 2, 1, -1)
        c.C = [C]
    return c.finish(*_rounding_box(c, rng, 1339, near_share=.1))


def case_D(real_t, which):
    dims = 2 if which.endswith("_2d") else 3
    key = which[:-3] if which.endswith("_2d") else which
    kw, opts, scheme, staged, turb = {}, {}, R.EULER, True, False
    if key == "open_side_walls": kw = dict(open_side_walls=True)
    elif key == "periodic_topbot": kw = dict(periodic_topbot_walls=True)
    elif key == "subs": kw, opts, staged = dict(subs_switch=True, w_LS=np.linspace(-.5, 1.5, 4)), dict(subs=True), False
    elif key == "no_sedi": opts, staged = dict(sedi=False), False
    elif key == "no_adve": opts, staged = dict(adve=False), False
    elif key in ("turb", "turb_pred_corr"):
        kw, staged, turb = dict(periodic_topbot_walls=True), False, True
        scheme = R.PRED_CORR if key == "turb_pred_corr" else R.EULER
    else:
        raise KeyError(which)
    c = Case(real_t, dims, DX_B, scheme, opts=opts, staged=staged, turb=turb, **kw)
    rng = np.random.default_rng(41 + sum(map(ord, which)))
    c.C = [_random_courant(c, rng, amp=.6, strong=1.2)]
    # (no_adve: nothing carries a droplet away from the face it starts next to, and the wrap's rounding, 6e-5 m in float, would decide
    # more than MAX_ESCAPED of the fates: uniform droplets only)
    pos, n, rw2, vt = _rounding_box(c, rng, 1403, near_share=0. if key == "no_adve" else .1)
    if turb:
        n[n == 0] = 5                                          # (nobody is removed: up, vp, wp are read behind the step)
    if key == "no_sedi":                                       # the wind alone takes droplets with rw2 = 0 through the floor: they start just above it
        c.C[0]["Cz"][..., 0] = -np.abs(c.C[0]["Cz"][..., 0]) - .1
        pos[rw2 == 0, 2] = rng.uniform(.01, .05, int((rw2 == 0).sum())) * c.oi.dz
    return c.finish(pos, n, rw2, vt)


def case_E(real_t, which):
    """one slab of a decomposed domain on its own: neighbours on both sides (euler, implicit), or a neighbour on the left and the open
    wall on the right (opts_init.open_side_walls, as libcloudphxx_amd.multi.distmem_opts sets the last slab up)"""
    scheme = R.IMPLICIT if which == "implicit" else R.EULER
    c = Case(real_t, 3, DX_B, scheme, open_side_walls=which == "open_rgt")
    c.oi.n_x_tot, c.oi.n_x_bfr = c.oi.nx, 0                  # (as tests/_harness.py LocalRing hands a slab its own part of every array)
    c.oi.bcond_lft = multi.BCOND_DISTMEM
    c.oi.bcond_rgt = multi.BCOND_OPEN if which == "open_rgt" else multi.BCOND_DISTMEM
    rng = np.random.default_rng(51 + len(which))
    C = _random_courant(c, rng, amp=.45, strong=.45) if scheme == R.IMPLICIT else _random_courant(c, rng, amp=.6, strong=1.2)
    c.C = [C]
    return c.finish(*_rounding_box(c, rng, 1467, near_share=.1))


CASES = {"A3": lambda t: case_A(t, 3), "A3_implicit": lambda t: case_A(t, 3, R.IMPLICIT), "A3_open": lambda t: case_A(t, 3, open_walls=True),
         "A2": lambda t: case_A(t, 2), "A1": lambda t: case_A(t, 1),
         "B3_euler": lambda t: case_B(t, 3, R.EULER), "B3_implicit": lambda t: case_B(t, 3, R.IMPLICIT), "B3_pred_corr": lambda t: case_B(t, 3, R.PRED_CORR),
         "B2_euler": lambda t: case_B(t, 2, R.EULER), "B2_implicit": lambda t: case_B(t, 2, R.IMPLICIT), "B2_pred_corr": lambda t: case_B(t, 2, R.PRED_CORR),
         "B1_euler": lambda t: case_B(t, 1, R.EULER),
         "C3_fallback": lambda t: case_C(t, 3, "fallback"), "C2_fallback": lambda t: case_C(t, 2, "fallback"),
         "C3_clamps": lambda t: case_C(t, 3, "clamps"), "C2_clamps": lambda t: case_C(t, 2, "clamps"),
         "D_open_side_walls": lambda t: case_D(t, "open_side_walls"), "D_open_side_walls_2d": lambda t: case_D(t, "open_side_walls_2d"),
         "D_periodic_topbot": lambda t: case_D(t, "periodic_topbot"), "D_subs": lambda t: case_D(t, "subs"),
         "D_no_sedi": lambda t: case_D(t, "no_sedi"), "D_no_sedi_2d": lambda t: case_D(t, "no_sedi_2d"), "D_no_adve": lambda t: case_D(t, "no_adve"),
         "D_turb": lambda t: case_D(t, "turb"), "D_turb_pred_corr": lambda t: case_D(t, "turb_pred_corr"),
         "E_euler": lambda t: case_E(t, "euler"), "E_implicit": lambda t: case_E(t, "implicit"), "E_open_rgt": lambda t: case_E(t, "open_rgt")}


# ---------------------------------------------------------------------------------------------------- the checks
def _worst(worst, key, val):
    if worst is not None and np.size(val):
        worst[key] = max(worst.get(key, 0.), float(np.max(val)))


def cell_of_stored(S, st):
    """hskpng_ijk.ipp:16-28, 33-82 in integers: size_t(double(x) / double(dx)) of the STORED position, z fastest"""
    c = lambda nm, d: (st[nm].astype(np.float64) / np.float64(d)).astype(np.int64) if nm in st else 0
    i, j, k = c("x", S.dx), c("y", S.dy), c("z", S.dz)
    return i if S.ndims == 1 else i * S.nz + k if S.ndims == 2 else i * (S.nz * S.ny) + j * S.nz + k


def align(b, a):
    """for every slot of the state before, the slot of the state after that holds the same droplet (-1: it is gone)"""
    where = {v: s for s, v in enumerate(a["rd3"])}
    assert len(where) == a["rd3"].size
    return np.array([where.get(v, -1) for v in b["rd3"]], dtype=np.int64)


def check_move(real_t, S, b, a, bars, worst, tag, K_name, exact=False, reindexed=False, whole=False):
    """one stage or one whole step: b the droplets before (storage order), a after.
      cell     (reindexed) the stored ijk of every living droplet that keeps a cell equals cell_of_stored() of ITS stored position, in
               integers: no rounding, no escape
      position |x - x_ref| -- modulo the domain length where bcnd wrapped the coordinate -- <= eps (K_scheme mag + K_wrap wrapmag);
               exact cases: wherever x_ref is a number of the real type, x is that number
      fate, n  n after is the reference's (0 for side, top, bottom), the stored cell is the reference's; a removed droplet may be gone
               from the storage, a living one may not
      escape   a droplet that fails and whose margin is inside the bar passes if it meets all of the above for the reference with the
               comparisons of a coordinate decided as if its quantities were one bar larger or smaller (R.move nudge, every combination
               over the coordinates); never in an exact case; at most MAX_ESCAPED of the living
    whole: droplets that start with n == 0 are not looked at (the step drops them without moving them).
    Returns (the reference's results by droplet as accepted, statistics)."""
    Ks, Kw, eps = bars[K_name], bars["K_wrap"], S.eps
    N = b["n"].size
    where = align(b, a)
    present = where >= 0
    w = np.where(present, where, 0)
    looked = (b["n"] != 0) if whole else np.ones(N, dtype=bool)
    n_dev = np.where(present, a["n"][w], 0).astype(np.uint64)
    ijk_dev = a["ijk"][w]
    if reindexed:
        keeps = present & (n_dev != 0) & looked & (ijk_dev != 0xFFFFFFFF)
        own = cell_of_stored(S, {k: v[w] for k, v in a.items() if k in "xyz"})
        assert np.array_equal(ijk_dev[keeps], own[keeps]), (tag, "ijk is not the cell of the stored position", np.nonzero(keeps & (ijk_dev != own))[0][:8])
    wrapped, L = S.wrapped(), S.lengths()

    def judge(Rv, record=False):
        ok = n_dev == Rv.n
        for ax, nm in enumerate("xyz"):
            if nm not in b:
                continue
            dev, ref = a[nm][w].astype(LD), (Rv.x, Rv.y, Rv.z)[ax]
            err = np.abs(dev - ref)
            if wrapped[ax]:
                err = np.minimum(err, np.abs(err - L[ax]))
            bar = eps * (Ks * Rv.mag[ax] + Kw * Rv.wmag[ax])
            okp = err <= bar
            if exact:
                repres = ref.astype(real_t).astype(LD) == ref
                okp = np.where(repres, dev == ref, okp)
            ok &= ~present | okp
            if record:
                sel = present & looked & (n_dev == Rv.n) & (Rv.margin > 1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    if whole:
                        _worst(worst, "whole", np.where(bar > 0, err / bar, 0)[sel])
                    else:
                        pure, wr = sel & (Rv.wmag[ax] == 0) & (Rv.mag[ax] > 0), sel & (Rv.wmag[ax] > 0)
                        _worst(worst, K_name, (err / (eps * np.where(pure, Rv.mag[ax], 1)))[pure])
                        _worst(worst, "K_wrap", (err / (eps * np.where(wr, Rv.wmag[ax], 1)))[wr])
        if reindexed:
            has = present & (n_dev != 0) & (Rv.cell >= 0)
            ok &= ~has | (ijk_dev == Rv.cell)
        return ok | ~looked

    R0 = R.move(S, b, 0, Ks, Kw)
    primary = judge(R0, record=True)
    near = R0.margin <= 1
    accepted = np.zeros(N, dtype=np.int64)
    variants = [R0]
    if not primary.all():
        assert not exact, (tag, "an exact case: %d droplets differ" % (~primary).sum(), _rows(b, a, w, R0, np.nonzero(~primary)[0][:6]))
        for s in itertools.product((0, 1, -1), repeat=3):       # coordinate by coordinate: a droplet may sit near a face in each
            if any(s) and (~primary & near & (accepted == 0)).any():
                Rv = R.move(S, b, s, Ks, Kw)
                variants.append(Rv)
                alt = judge(Rv) & ~primary & near & (accepted == 0)
                accepted[alt] = len(variants) - 1
        bad = ~primary & (accepted == 0)
        if bad.any():
            raise AssertionError((tag, "%d droplets fail" % bad.sum(), _rows(b, a, w, R0, np.nonzero(bad)[0][:6])))
    live = looked & (b["n"] != 0)
    escaped = int((accepted != 0).sum())
    assert escaped <= MAX_ESCAPED * max(1, int(live.sum())), (tag, "droplets that pass as the neighbouring outcome", escaped, int(live.sum()))
    pick = lambda f: np.choose(accepted, [f(v) for v in variants])
    acc = R.Result()
    acc.n, acc.cell, acc.fate, acc.below = pick(lambda v: v.n), pick(lambda v: v.cell), pick(lambda v: v.fate), pick(lambda v: v.below)
    acc.left, acc.right = pick(lambda v: v.left), pick(lambda v: v.right)
    acc.terms = {k: pick(lambda v, k=k: v.terms[k]) for k in R.PUDDLE}
    acc.looked = looked
    stats = {nm: int(((R0.fate == f) & looked).sum()) for f, nm in enumerate(R.FATES)}
    stats.update(near=int((near & live).sum()), escaped=escaped, live=int(live.sum()))
    return acc, stats


def _rows(b, a, w, R0, idx):
    out = []
    for i in idx:
        row = dict(slot=int(i), n0=int(b["n"][i]), n1=int(a["n"][w[i]]), n_ref=int(R0.n[i]), ijk0=int(b["ijk"][i]), ijk1=int(a["ijk"][w[i]]), cell_ref=int(R0.cell[i]),
                   fate=R.FATES[R0.fate[i]], margin=float(R0.margin[i]), vt=float(b["vt"][i]))
        for ax, nm in enumerate("xyz"):
            if nm in b:
                ref = (R0.x, R0.y, R0.z)[ax][i]
                row[nm] = (float(b[nm][i]), float(a[nm][w[i]]), float(ref), "err/eps/mag %.2f" % float(abs(LD(a[nm][w[i]]) - ref) / (R0.mag[ax][i] + R0.wmag[ax][i] + LD(1e-300)) / LD(np.finfo(a[nm].dtype).eps)))
        out.append(row)
    return out


PUDDLE_KEYS = {"liq_vol": "liquid_volume", "dry_vol": "dry_volume", "liq_num": "liquid_number", "prtcl_num": "particle_number"}


def check_puddle(real_t, acc, before, after, eps_acc, worst, tag):
    """what diag_puddle gained against the accepted droplets below the floor: the two counts exact; the two volumes within (N + 8)
    eps_acc sum|term| -- eps_acc the type the object accumulates in: double on the device, the real type in the oracle as in the
    reference -- plus K_POW eps sum|term| for the terms' own roundings in the real type"""
    eps = LD(np.finfo(real_t).eps)
    got = {k: LD(after[v]) - LD(before[v]) for k, v in PUDDLE_KEYS.items()}
    want = R.puddle(acc, acc.looked)
    for k in ("liq_num", "prtcl_num"):
        assert got[k] == want[k][0], (tag, k, float(got[k]), float(want[k][0]))
    for k in ("liq_vol", "dry_vol"):
        S_, cnt = want[k]
        # the running total is rounded too: one eps_acc of its value per addition
        bar = (cnt + 8) * LD(eps_acc) * S_ + K_POW * eps * S_ + 2 * LD(eps_acc) * abs(LD(after[PUDDLE_KEYS[k]]))
        err = abs(got[k] - S_)
        if bar > 0:
            _worst(worst, "puddle / bar", float(err / bar))
        assert err <= bar, (tag, k, float(got[k]), float(S_), "bar", float(bar))
    return want["prtcl_num"][1]


# ---------------------------------------------------------------------------------------------------- running a case
def read_state(prt, real_t, p):
    """p: "" or "raw_" (the storage as it is, dead slots included: the HIP object's names that disturb nothing)"""
    oi = prt.opts_init
    st = {"n": prt.state_u64(p + "n"), "ijk": prt.state_u64(p + "ijk").astype(np.int64), "rd3": prt.state_real(p + "rd3")}
    for k in ("rw2", "vt"):
        st[k] = prt.state_real(p + k).astype(real_t)
    for nm in "xyz":
        if getattr(oi, "n" + nm):
            st[nm] = prt.state_real(p + nm).astype(real_t)
    return st


def setup_of(prt, case, **kw):
    """the reference's set-up from what the OBJECT holds: its Courant arrays, halo included, and through them the step's scheme"""
    oi, t = case.oi, case.real_t
    C = {k: prt.state_real("courant_" + k[1]) for k in ("Cx", "Cy", "Cz")[:1] + (("Cy",) if oi.ny else ()) + (("Cz",) if oi.nz else ())}
    halo = 2 if case.scheme == R.PRED_CORR else 0
    nxh = oi.nx + 2 * halo
    assert C["Cx"].size == (nxh + 1) * max(oi.ny, 1) * max(oi.nz, 1), "the x array with its halo"
    scheme, margin = R.effective_scheme(case.scheme, C["Cx"])
    assert margin > 1e-3, "no Courant number within rounding of +-2"
    dist = int(oi.bcond_lft) == multi.BCOND_DISTMEM or int(oi.bcond_rgt) == multi.BCOND_DISTMEM
    S = R.Setup(t, oi.nx, oi.ny, oi.nz, oi.dx, oi.dy, oi.dz, oi.x0, oi.y0, oi.z0, oi.x1, oi.y1, oi.z1, oi.dt, scheme, halo, C["Cx"], C.get("Cy"), C.get("Cz"),
                w_LS=oi.w_LS if np.size(oi.w_LS) else None, open_side_walls=oi.open_side_walls, periodic_topbot=oi.periodic_topbot_walls,
                distmem=dist, open_lft=int(oi.bcond_lft) == multi.BCOND_OPEN, open_rgt=int(oi.bcond_rgt) == multi.BCOND_OPEN)
    return S.but(**kw)


def make_opts(case):
    opts = lgrngn.opts_t()
    opts.cond = opts.coal = False
    for k, v in case.opts.items():
        setattr(opts, k, v)
    return opts


def _add(tot, st):
    for k, v in st.items():
        tot[k] = tot.get(k, 0) + v


def run_case(name, make, real_t, staged, prefix="", worst=None, eps_acc=None, saw_kernel=None, counts_dead_migrants=True):
    """make(oi, real_t) -> the object.  saw_kernel(prt, case, step, stage or None): called behind every launch of the move.
    counts_dead_migrants: migrate_counts lists a droplet beyond a slab face whatever else happened to it (bcnd.ipp:160-172; the HIP
    object does not ship what it has removed)"""
    case = ALL_CASES[name](real_t)
    bars = BARS[real_t]
    assert staged or not case.outside, "a droplet outside the domain must not meet a re-indexing"
    eps_acc = np.finfo(real_t).eps if eps_acc is None else eps_acc
    assert case.staged or not staged, "this case has no staged form (subsidence and the SGS velocities have no stage)"
    oi, opts = case.oi, make_opts(case)
    prt = make(oi, real_t)
    th, rv, rhod, C = case.fields(0)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C.items()})
    args = dict(case.args)
    if not staged and opts.sedi:
        # a whole step that sediments computes vt itself, and beard76 of rw2 = 0 is 0 x infinity: there rw2 = 0 becomes 1e-12.  The staged
        # runs and the whole steps without sedimentation keep it and carry it through the floor
        args["rw2"] = np.where(args["rw2"] == 0, 1e-12, args["rw2"])
    prt.set_particles(**args)
    K_of = lambda S: "K_" + S.scheme
    total = {}
    for step in range(1 if staged else len(case.C)):
        tag = "%s %s %s step %d" % (name, real_t.__name__, "staged" if staged else "whole", step)
        th, rv, rhod, C = case.fields(step)
        kw = dict(diss_rate=np.full(case.shape, 1e-3, dtype=real_t)) if case.turb else {}
        prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C.items()}, **kw)
        pud0 = prt.diag_puddle()
        # (read here, where nothing is dead or on its way to a neighbour: the getter of a Courant array may put the storage in order first)
        S0 = setup_of(prt, case)
        if staged:
            # every stage first, reading nothing but the storage as it is; the checks afterwards
            st = [read_state(prt, real_t, prefix)]
            assert np.array_equal(st[0]["rd3"], args["rd3"]), "set_particles keeps the order"
            for stage in ("adve", "sedi", "bcnd"):
                if stage == "sedi" and not oi.nz:                # (no z: the stage has nothing to move, and the state before stands for the state after)
                    st.append(st[-1])
                    continue
                prt.stage(stage, opts)
                if saw_kernel: saw_kernel(prt, case, step, stage)
                st.append(read_state(prt, real_t, prefix))
            pud1, mig = prt.diag_puddle(), prt.migrate_counts()
            S = S0.but(turb=False, subs=False)
            if not S.distmem and not case.outside:               # (a slab's emigrants lie outside it: "cell indices are anyway undefined", bcnd.ipp:149)
                prt.stage("hskpng_ijk")
            st.append(read_state(prt, real_t, prefix))
            _, s1 = check_move(real_t, S.but(sedi=False, bcnd=False), st[0], st[1], bars, worst, tag + " adve", K_of(S), case.exact)
            check_move(real_t, S.but(adve=False, bcnd=False), st[1], st[2], bars, worst, tag + " sedi", "K_sedi", case.exact)
            acc, s3 = check_move(real_t, S.but(adve=False, sedi=False), st[2], st[3], bars, worst, tag + " bcnd", "K_sedi", case.exact)
            n_precip = check_puddle(real_t, acc, pud0, pud1, eps_acc, worst, tag)
            check_migrants(mig, S, acc, counts_dead_migrants, tag)
            for k in ("n", "x", "y", "z"):
                assert k not in st[3] or np.array_equal(st[3][k], st[4][k]), (tag, "hskpng_ijk moves nothing", k)
            keeps = (st[4]["n"] != 0) & (acc.cell >= 0)
            assert S.distmem or case.outside or np.array_equal(st[4]["ijk"][keeps], cell_of_stored(S, st[4])[keeps]), (tag, "hskpng_ijk: not the cell of the stored position")
            s3.update(stay=int(((st[0]["ijk"] == st[4]["ijk"]) & keeps).sum()), moved=int(((st[0]["ijk"] != st[4]["ijk"]) & keeps).sum()), near=s1["near"] + s3["near"],
                      escaped=s1["escaped"] + s3["escaped"], precipitated=n_precip)
            if case.outside:
                assert ((st[3]["x"] < real_t(oi.x0)) & (st[3]["n"] != 0)).sum() >= 4, (tag, "droplets that `periodic` leaves outside the domain")
                s3["outside"] = int(((st[3]["x"] < real_t(oi.x0)) & (st[3]["n"] != 0)).sum())
            _add(total, s3)
        else:
            if opts.sedi:
                prt.stage("hskpng_vterm_all")                    # vt as the step is about to compute it: the removed droplets' cannot be read behind it
            st0 = read_state(prt, real_t, prefix)
            prt.step_async(opts)
            st1 = read_state(prt, real_t, prefix)
            S = S0.but(turb=case.turb, adve=bool(opts.adve), sedi=bool(opts.sedi), subs=bool(opts.subs))
            if saw_kernel: saw_kernel(prt, case, step, None)
            where = align(st0, st1)
            kept = where >= 0
            if opts.sedi:
                assert np.array_equal(st1["vt"][where[kept]], st0["vt"][kept]), (tag, "the step's vt is the stage's")
            if case.turb:
                assert kept.all(), "nobody is removed in the turbulent cases"
                late = {k: prt.state_real(k) for k in ("rd3", "up", "vp", "wp")}
                at = align(st0, late)
                for k in ("up", "vp", "wp"):
                    if late[k].size:
                        st0[k] = late[k][at].astype(real_t)
            acc, s = check_move(real_t, S, st0, st1, bars, worst, tag, K_of(S), case.exact, reindexed=not S.distmem, whole=True)
            s["precipitated"] = check_puddle(real_t, acc, pud0, prt.diag_puddle(), eps_acc, worst, tag)
            check_migrants(prt.migrate_counts(), S, acc, counts_dead_migrants, tag)
            s["precipitated_rw2_0"] = int((acc.below & (st0["rw2"] == 0) & (acc.terms["prtcl_num"] > 0)).sum())
            assert opts.sedi or not oi.nz or oi.periodic_topbot_walls or s["precipitated_rw2_0"] >= 1, (tag, "rw2 = 0 through the floor of a whole step")
            _add(total, s)
            if S.distmem:
                break                                            # (a slab on its own: the exchange that would finish the step has nobody to talk to)
            # census: the object's counts against the accepted fates
            alive = acc.looked & (acc.n != 0)
            cnt = np.bincount(acc.cell[alive], minlength=prt.n_cell)
            got = np.zeros(prt.n_cell, dtype=np.int64)
            got[prt.state_u64("count_ijk").astype(np.int64)] = prt.state_u64("count_num").astype(np.int64)
            assert np.array_equal(got, cnt), (tag, "per-cell counts")
            assert prt.n_part == int(alive.sum()), (tag, "n_part", prt.n_part, int(alive.sum()))
            if prefix:
                raw_n = prt.state_u64(prefix + "n")
                assert int((raw_n != 0).sum()) == int(alive.sum()), (tag, "dead slots")
    return total


def check_migrants(got, S, acc, counts_dead, tag):
    if not S.distmem:
        return
    # (acc.looked: a whole step of the HIP object drops a droplet that came with n == 0 where it stands)
    lft = int((acc.left if counts_dead else (acc.fate == R.LEFT) & acc.looked).sum())
    rgt = int((acc.right if counts_dead else (acc.fate == R.RIGHT) & acc.looked).sum())
    assert tuple(got) == (lft, rgt), (tag, "migrate_counts", got, (lft, rgt))


# by stages only: what leaves a droplet outside the domain (module docstring, A)
STAGED_ONLY = {"A3_beyond": lambda t: case_A(t, 3, beyond=True), "A2_beyond": lambda t: case_A(t, 2, beyond=True), "A1_beyond": lambda t: case_A(t, 1, beyond=True)}
ALL_CASES = dict(CASES, **STAGED_ONLY)
STAGED = [k for k in CASES if not k.startswith(("C3_clamps", "C2_clamps", "D_subs", "D_no_", "D_turb"))] + list(STAGED_ONLY)

# ---------------------------------------------------------------------------------------------------- which k_move a run launches
M3D, FULL, DISTMEM, IMPLICIT = 1, 2, 4, 8
NINE = {(False, False, 0), (False, False, M3D), (False, False, M3D | FULL), (False, False, M3D | FULL | DISTMEM), (False, False, M3D | FULL | IMPLICIT),
        (False, False, M3D | FULL | DISTMEM | IMPLICIT), (True, False, 0), (False, True, 0), (True, True, 0)}


def expected_kernel(case, step, stage):
    """(PC, TURB, SPEC) as move() chooses them (lcx_core.hip): the predictor-corrector unless this step's Cx made it fall back; the SGS
    velocities in a whole step only; SPEC for the rest: three dimensions, and the full step's pass where nothing but advection (euler or
    implicit, no halo), sedimentation and the default walls is asked for.  stage: "adve" / "sedi" / "bcnd", or None for a whole step"""
    oi = case.oi
    scheme = R.effective_scheme(case.scheme, case.C[step]["Cx"])[0]
    pc, tb = scheme == R.PRED_CORR, case.turb and stage is None
    if pc or tb or case.dims < 3:
        return pc, tb, 0
    full = (stage is None and case.opts["adve"] and case.opts["sedi"] and not case.opts["subs"] and case.scheme != R.PRED_CORR
            and not oi.open_side_walls and not oi.periodic_topbot_walls)
    if not full:
        return pc, tb, M3D
    dist = multi.BCOND_DISTMEM in (int(oi.bcond_lft), int(oi.bcond_rgt))
    return pc, tb, M3D | FULL | (DISTMEM if dist else 0) | (IMPLICIT if scheme == R.IMPLICIT else 0)


def planned_kernels():
    """{(PC, TURB, SPEC): (case, staged)}: one run that reaches each k_move the cases are laid out for"""
    plan = {}
    for name, make in ALL_CASES.items():
        case = make(np.float64)
        if name in CASES:
            for step in range(len(case.C)):
                plan.setdefault(expected_kernel(case, step, None), (name, False))
        if name in STAGED:
            for s in ("adve", "sedi", "bcnd"):
                plan.setdefault(expected_kernel(case, 0, s), (name, True))
    return plan


def test_the_cases_are_laid_out_for_all_nine_instantiations():
    assert set(planned_kernels()) == NINE, sorted(set(planned_kernels()) ^ NINE)


def held_to_the_record(worst, real_t):
    """the oracle stays at or below the worsts that the bars were derived from (MEASURED holds three decimals)"""
    for k, v in MEASURED[real_t].items():
        assert worst.get(k, 0.) <= v + 1e-3, (k, worst[k], v)



@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", STAGED)
def test_oracle_stages_match_the_plain_reference(name, real_t):
    worst = {}
    seen = run_case(name, lambda oi, t: ORACLES[t](oi), real_t, True, worst=worst)
    held_to_the_record(worst, real_t)
    print("\nmove %s staged %s: worst %s bars %s fates %s" % (name, real_t.__name__, {k: round(v, 3) for k, v in worst.items()}, BARS[real_t], seen))


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_whole_step_matches_the_plain_reference(name, real_t):
    worst = {}
    seen = run_case(name, lambda oi, t: ORACLES[t](oi), real_t, False, worst=worst)
    held_to_the_record(worst, real_t)
    print("\nmove %s whole %s: worst %s bars %s fates %s" % (name, real_t.__name__, {k: round(v, 3) for k, v in worst.items()}, BARS[real_t], seen))
