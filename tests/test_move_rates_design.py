"""The boxes that tests/test_hip_move_rates.py tallies, run on the strict CPU oracle (no GPU): one step_async of advection and sedimentation
must make every row of include/lcx_move_rates.h's table occur at every threshold, or the device test would pass on an empty case.  Judged
through the long-double reference (tests/_move_rates_reference.py) alone.

The 2-D box: 4 x 4 cells of 1 m, dt = 1 s, occupancies OCC (527 droplets, not a multiple of 64: cell runs end inside a wave, span waves and
span a workgroup; cell 0 is empty).  Courant numbers: column 0 rises (Cz = 0.6) and drifts right, or left through the periodic wall on
level 2; column 1 rises slowly and converges on its right face; column 2 stands still between two faces of Cx = 0, so only sedimentation
moves its droplets and cell 10 (two haze droplets, haze above it) sees no traffic at all; column 3 sinks (Cz = -0.2) and drifts through the
periodic wall into column 0 -- on level 0 into the empty cell.  Radii are log-uniform in 1 ... 80 um, a handful of drizzle drops of
150 ... 200 um are placed by hand: one falls two levels, one reaches the ground from level 1.  Thresholds 0, 25 um and 60 um.  n in
1 ... 2000, rd3 = (1e-8 (1 + id / 7))^3: unique per droplet and unchanged by the move, so it identifies a droplet across the step.
Nobody moves by two cell lengths or more, so a removed droplet left through the bottom if it started in the lower half and through the top
otherwise; and few enough are removed (less than 1 in 32) that the device leaves every slot where it is.

The 3-D box: 3 x 3 x 4 cells with the same kind of occupancies and smooth Courant numbers in all three directions."""
import numpy as np
import pytest

import _harness as h
import _move_rates_reference as MV
from libcloudphxx_amd import lgrngn

LD = np.longdouble
OCC = [0, 1, 2, 3, 5, 63, 64, 65, 300, 2, 2, 2, 3, 5, 8, 2]
OCC3 = [0, 1, 63, 64, 65, 300] + [2, 3, 5, 8, 2, 1] * 5
THR = [0., 25e-6, 60e-6]
MARGIN = 1e-6                        # of dx: how far every new position stays from every cell face and wall


def courant_2d():
    Cx, Cz = np.zeros((5, 4)), np.zeros((4, 5))
    Cx[0] = Cx[4] = [.3, .3, -.3, .3]
    Cx[1] = [.2, .2, -.2, .2]
    Cz[0], Cz[1], Cz[3] = .6, .1, -.2
    return dict(Cx=Cx, Cz=Cz)


def courant_3d():
    i, j = np.indices((3, 3))
    Cz = np.repeat((.3 * ((i + j) % 3 - 1) + .2)[:, :, None], 5, axis=2)
    return dict(Cx=np.full((4, 3, 4), .25), Cy=np.full((3, 4, 4), -.2), Cz=Cz)


def design(real_t, dims=2, seed=5, **kw):
    kw.setdefault("coal_switch", False)
    kw.setdefault("reorder_every", -1)
    occ = OCC if dims == 2 else OCC3
    nx, ny, nz = (4, 0, 4) if dims == 2 else (3, 3, 4)
    kw.setdefault("n_sd_max", sum(occ) + 64)
    oi = h.box_opts(nx, ny, nz, 2, dx=1., dt=1., kernel=lgrngn.kernel_t.geometric, terminal_velocity=lgrngn.vt_t.beard76, **kw)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    shp = (nx, nz) if dims == 2 else (nx, ny, nz)
    th, rv, rhod = np.full(shp, 289.), np.full(shp, 6.0e-3), np.full(shp, 1.1)
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.arange(len(occ)), occ)
    N = cells.size
    r = np.exp(rng.uniform(np.log(1e-6), np.log(80e-6), N))
    n = rng.integers(1, 2000, N).astype(np.uint64)
    rd3 = (1e-8 * (1 + np.arange(N) / 7.)) ** 3
    k = cells % nz
    i = cells // nz if dims == 2 else cells // (nz * ny)
    j = (cells // nz) % ny if dims == 3 else np.zeros(N, dtype=np.int64)
    fx, fy, fz = rng.uniform(.05, .95, N), rng.uniform(.05, .95, N), rng.uniform(.05, .95, N)
    if dims == 2:
        haze = (cells == 10) | (cells == 11)                           # the still cell and the one above it
        r[haze], fz[haze] = 1e-6 * (1 + np.arange(haze.sum())), .5
        first = lambda c: int(np.flatnonzero(cells == c)[0])
        fz[cells == 8] = rng.uniform(.5, .95, OCC[8])                  # (the 300 droplets of level 0: only the drizzle placed below reaches the ground)
        for c, rr, zz in ((9, 200e-6, .2), (15, 180e-6, .1), (7, 190e-6, .15), (8, 170e-6, .5), (8, 150e-6, .05), (5, 160e-6, .1), (2, 65e-6, .95), (3, 70e-6, .9)):
            s = first(c) + (1 if (c, zz) == (8, .05) else 0)
            r[s], fz[s] = rr, zz                                       # drizzle: to the ground from level 1 (cell 9), two levels down (15, 7), ...;
                                                                       # and two drops of 65 and 70 um that the updraught of column 0 still lifts
    else:
        for s, (rr, zz) in zip(np.flatnonzero(k == 1)[:3], ((200e-6, .2), (180e-6, .3), (70e-6, .02))):
            r[s], fz[s] = rr, zz
        for s in np.flatnonzero(k == 3)[:2]:
            r[s], fz[s] = 190e-6, .1
        for c in (10, 11):                                             # (the column of Cz = 0.5 lifts a drop of 65 um a level up, and out of the top)
            s = int(np.flatnonzero(cells == c)[0])
            r[s], fz[s] = 65e-6, .95
    rw2 = (r.astype(LD) ** 2).astype(real_t)
    args = dict(n=n, rd3=rd3, rw2=rw2.astype(np.float64), kpa=np.full(N, .5), vt=np.zeros(N), x=i + fx, z=k + fz)
    if dims == 3:
        args["y"] = j + fy
    C = courant_2d() if dims == 2 else courant_3d()
    box = MV.Box(nx, ny, nz, x1=float(nx), y1=float(max(ny, 1)), z1=float(nz), open_side_walls=bool(oi.open_side_walls),
                 periodic_topbot=bool(oi.periodic_topbot_walls))
    return dict(oi=oi, fields=(f(th), f(rv), f(rhod), {nm: f(v) for nm, v in C.items()}), cells=cells, args=args, box=box, dims=dims)


def permuted(case, perm):
    """the same droplets handed over in another storage order"""
    return dict(case, cells=case["cells"][perm], args={k: v[perm] for k, v in case["args"].items()})


def move_only(**kw):
    opts = lgrngn.opts_t()
    opts.coal = opts.cond = False
    opts.adve = opts.sedi = True
    for k, v in kw.items():
        assert hasattr(opts, k), k
        setattr(opts, k, v)
    return opts


def raw(prt, real_t, prefix=""):
    oi = prt.opts_init
    g = lambda nm: prt.state_real(prefix + nm).astype(real_t)
    return dict(n=prt.state_u64(prefix + "n"), ijk=prt.state_u64(prefix + "ijk").astype(np.int64), rw2=g("rw2"), rd3=prt.state_real(prefix + "rd3"),
                pos=(g("x") if oi.nx else None, g("y") if oi.ny else None, g("z") if oi.nz else None))


def aligned(b, a):
    """the state behind the step on the slots of the state ahead of it, droplets identified by rd3: (n1, ijk1, pos1 or None).  pos1 is
    there when no slot has moved (the removed droplets' last positions are still in the storage)"""
    if a["rd3"].size == b["rd3"].size and np.array_equal(a["rd3"], b["rd3"]):
        return a["n"], a["ijk"], a["pos"]
    assert np.unique(b["rd3"]).size == b["rd3"].size
    where = {v: s for s, v in enumerate(a["rd3"])}
    n1, ijk1 = np.zeros(b["n"].size, dtype=np.uint64), np.full(b["n"].size, -1, dtype=np.int64)
    for s, v in enumerate(b["rd3"]):
        if v in where:
            n1[s], ijk1[s] = a["n"][where[v]], a["ijk"][where[v]]
    return n1, ijk1, None


def start(prt, case, before_set=None):
    th, rv, rhod, C = case["fields"]
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C.items()})
    if before_set is not None:
        before_set(prt)
    prt.set_particles(**case["args"])


def one_step(prt, case, real_t, opts=None, prefix=""):
    """(state before, state after) of one step_sync + step_async that moves only; the state before is read behind step_sync"""
    th, rv, rhod, C = case["fields"]
    opts = opts if opts is not None else move_only()
    prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy())
    b = raw(prt, real_t, prefix)
    prt.step_async(opts)
    return b, raw(prt, real_t, prefix)


def reference(case, b, a, lo, rows=None):
    n1, ijk1, pos1 = aligned(b, a)
    return MV.tally(b["n"], b["ijk"], b["rw2"], b["pos"], n1, ijk1, lo, case["box"], pos1, rows)


def margins(case, a):
    """the smallest distance, in dx, of a living droplet's new position from a cell face or a wall"""
    d = np.inf
    for p in a["pos"]:
        if p is not None:
            q = p.astype(LD)[a["n"] != 0]
            d = min(d, float(np.min(np.abs(q - np.round(q)))))
    return d


@pytest.mark.parametrize("dims", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_step_on_the_oracle_makes_every_row_occur(real_t, dims):
    case = design(real_t, dims)
    occ = OCC if dims == 2 else OCC3
    N = sum(occ)
    assert N % 64 != 0
    prt = (h.oracle_particles if real_t is np.float64 else h.oracle_f32_particles)(case["oi"])
    start(prt, case)
    b, a = one_step(prt, case, real_t)
    assert np.array_equal(b["ijk"], case["cells"]) and np.unique(b["rd3"]).size == N
    assert margins(case, a) >= MARGIN, margins(case, a)
    lo = MV.bounds(THR, real_t)
    n1, ijk1, pos1 = aligned(b, a)
    assert pos1 is None, "the oracle removes what the move removed"
    gone = n1 == 0
    assert 0 < gone.sum() * 32 <= N, ("few enough are removed that the device keeps every slot where it is", int(gone.sum()))
    rows = reference(case, b, a, lo)
    ev = rows.events
    print(real_t.__name__, "%d-D" % dims, ev, "removed", int(gone.sum()), "margin", margins(case, a))
    assert ev["stay"] >= 1 and ev["moved"] >= 1 and ev["bottom"] >= 1 and ev["top"] >= 1 and ev["side"] == 0
    blk = rows.block()
    for t in range(3):
        assert (b["rw2"] >= lo[t]).any() and (t == 0 or (b["rw2"] < lo[t]).any()), "radii on both sides of the threshold"
        for w in range(10):
            assert blk[10 * t + w].sum() > 0, ("row", MV.NAMES[w], "threshold", t)
    nz = case["box"].nz
    k0, k1 = b["ijk"] % nz, ijk1 % nz
    assert ((k0 - k1 == 2) & ~gone).any(), "a droplet falls two levels in one step"
    assert (gone & (k0 == 1) & (b["pos"][2] < 2)).any(), "a droplet reaches the ground from level 1"
    empty = occ.index(0)
    assert blk[MV.IN_N, empty] > 0 and blk[MV.OUT_N, empty] == 0, "arrivals into the empty cell"
    big = [c for c, m in enumerate(occ) if m >= 63]
    assert all(blk[MV.OUT_N, c] > 0 for c in big) and blk[MV.IN_N, big].sum() > 0, "crossings in the cells of at least 63 droplets"
    i0 = b["ijk"] // (nz * max(case["box"].ny, 1))
    i1 = ijk1 // (nz * max(case["box"].ny, 1))
    assert (~gone & (np.abs(i0 - i1) == case["box"].nx - 1)).any(), "a periodic side wrap"
    if dims == 2:
        assert (blk[:, 10] == 0).all() and occ[10] > 0, "a cell with no traffic at all"
        # nobody moves by two cells or more: the exit of a removed droplet follows from where it started
        assert (np.abs(k0 - k1)[~gone] <= 2).all()
    # the budgets of the header, in integers: per cell over the move, and over the domain
    for t in range(3):
        ab0 = b["rw2"] >= lo[t]
        N0 = np.bincount(b["ijk"][ab0], weights=None, minlength=len(occ))
        before = np.array([int(b["n"][ab0 & (b["ijk"] == c)].astype(object).sum()) for c in range(len(occ))], dtype=object)
        after = np.array([int(n1[ab0 & ~gone & (ijk1 == c)].astype(object).sum()) for c in range(len(occ))], dtype=object)
        net = np.array([rows.value(10 * t + MV.IN_N, c) - rows.value(10 * t + MV.OUT_N, c) for c in range(len(occ))], dtype=object)
        assert (after - before == net).all() and N0.sum() > 0
        assert sum(rows.value(10 * t + MV.IN_N, c) for c in range(len(occ))) == sum(rows.value(10 * t + MV.OUT_N, c) for c in range(len(occ))) - rows.removed[t]
    # the ground: what the reference calls PRECIP is what the oracle's puddle received
    assert int(prt.diag_puddle()["particle_number"]) == sum(rows.value(MV.PRECIP_N, c) for c in range(len(occ))) > 0
