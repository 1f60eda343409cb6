"""CPU gate of the coalescence skip (k_coal_ranked<.., SKIP>, csrc/lcx_kernels.hpp coal_pair): how many candidate pairs, and how many
128-byte lines of their attributes, are left to read once every pair with `bound < 1 and u >= bound` is skipped -- on the droplets of the
OpenMP oracle on bench.py's fields, with k_geometric and interpolated_efficiency restated in numpy -- and the assertion that the bound is
one: prob <= bound for every pair.

    python3 tools/coal_skip_gate.py [--n 16] [--sd 64] [--workload stratocumulus|coal-stress] [--dt 1] [--steps 5,50,200] [--group 512] [--mixed] [--sparse K:R]

Two bounds per cell: "table" takes the largest efficiency of the whole table, "radius" the largest one that radii up to the cell's largest
can reach (what the kernel uses).  A line is 16 consecutive positions of the cell-sorted order, the granularity of the gathers' traffic.
The pairing is the coalescence's: a random order inside each cell, pairs at even offsets.  For coal-stress the quantiles of the bound and
the share of pairs that collide are printed as well (what tests/test_hip_coal_skip.py's time steps were chosen from).

For the workgroups that leave ahead of the ranking (k_coal_ranked<.., SKIP, EXIT>) the "radius" row also gives the share of the groups of
--group consecutive positions (a workgroup's 512) and of the cells that hold at least one kept pair.  --mixed: after init every droplet
with x < x1 / 2 gets rw2 x 1e-4 and rd3 x 1e-6 -- half of the sorted order that cannot collide next to a half that does
(tests/test_hip_coal_rank_exit.py; its figures are --workload coal-stress --dt 0.02 --mixed --steps 1,2,5,10 --group 256).  --sparse K:R: every
droplet shrunk like that except those of the cells with index % K == R, which become 100 um and 50 um drops in turn, and every
multiplicity 2.5e9 -- in the natural spectrum a kept pair collides once in two thousand times (the bound takes the box's largest
multiplicity and the cell's largest radius and velocity); here one in six does, so that at K = 8 a group of 512 positions holds ONE cell
whose one or two kept pairs often collide (the same test file's sparse box: --workload coal-stress --dt 0.05 --sparse 8:2 --steps 1,2,5,10).

--prevote: for the cells' vote ahead of the launch (k_coal_umin, k_coal_cellvote; EXPERIMENTS.md 7.13) the "radius" row also gives, side by side,
the share of the groups flagged through their cells -- every group that the stretch of a cell with a kept pair overlaps -- and the share of
the groups that hold a kept pair themselves: what the per-cell granularity costs (--steps 5,50,100,200 for the headline's table).

A step in which no pair is kept (the stratocumulus box's first) prints its rows up to the groups' shares and not the line of kept pairs
per group, with or without --prevote: there is nothing to average (that line used to end the run with numpy's error on an empty maximum).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                            # noqa: E402
import bench                                                  # noqa: E402
import _harness as h                                          # noqa: E402
from libcloudphxx_amd import lgrngn                           # noqa: E402

MARGIN = 1 + 2. ** -10


def load_table(kernel):
    a = np.fromfile(os.path.join(ROOT, "libcloudphxx_amd", "data", "kernel_eff_%d.f64" % int(kernel)))
    return a[0], a[2:2 + int(a[1])]


def kernel_index(R):
    return np.where(R <= 100, R, 100 + (R - 100) / 10.).astype(np.int64)


def vec_index(i, j):
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    return hi * (hi + 1) // 2 + lo


def interpolated_efficiency(tab, r_max, r1, r2):
    """kernel_interpolation.hpp:9-65 as csrc/lcx_kernels.hpp states it; radii in metres"""
    r1, r2 = r1 * 1e6, r2 * 1e6
    r1 = np.where(r1 >= r_max, r_max - 1e-6, r1)
    r2 = np.where(r2 >= r_max, r_max - 1e-6, r2)
    x0 = np.where(r1 >= 100, np.floor(r1 / 10) * 10, np.floor(r1)); dx = np.where(r1 >= 100, 10., 1.)
    y0 = np.where(r2 >= 100, np.floor(r2 / 10) * 10, np.floor(r2)); dy = np.where(r2 >= 100, 10., 1.)
    x1, y1 = x0 + dx, y0 + dy
    i0, i1, j0, j1 = kernel_index(x0), kernel_index(x1), kernel_index(y0), kernel_index(y1)
    w0, w1, w2, w3 = r1 - x0, x1 - r1, r2 - y0, y1 - r2
    return (tab[vec_index(i0, j0)] * w1 * w3 + tab[vec_index(i1, j0)] * w0 * w3 + tab[vec_index(i0, j1)] * w1 * w2 + tab[vec_index(i1, j1)] * w0 * w2) / dx / dy


def efficiency_maxima(tab):
    """lcx_core.hip init_kernel: emax[i] = the largest node of the rows 0 ... i + 1 of the triangular table"""
    nn = int(round((np.sqrt(8. * len(tab) + 1) - 1) / 2))
    assert nn * (nn + 1) // 2 == len(tab)
    rows = np.array([tab[a * (a + 1) // 2: a * (a + 1) // 2 + a + 1].max() for a in range(nn)])
    run = np.maximum.accumulate(rows)
    return np.array([run[min(i + 1, nn - 1)] for i in range(nn)])


def float_up(x):
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float64)


def gate(orc, oi, tab, r_max, emax, rng, label, group=512, prevote=False):
    n, rw2, vt, ijk = orc.state_u64("n").astype(np.float64), orc.get_attr("rw2"), orc.state_real("vt"), orc.state_u64("ijk").astype(np.int64)
    ncell = oi.nx * oi.ny * oi.nz
    dv = oi.dx * oi.dy * oi.dz
    order = np.lexsort((rng.random(len(n)), ijk))            # the cells in turn, a random order inside each
    c = ijk[order]
    start = np.searchsorted(c, np.arange(ncell + 1))
    cnt = np.diff(start)
    off = np.arange(len(c)) - start[c]
    first = (off % 2 == 0) & (off + 1 < cnt[c])
    pa, pb = np.nonzero(first)[0], np.nonzero(first)[0] + 1
    a, b, cell = order[pa], order[pb], c[pa]
    nn = cnt[cell].astype(np.float64)
    scl = (nn * (nn - 1) / 2) / np.floor(nn / 2)
    geom = np.pi * np.maximum(n[a], n[b]) * np.abs(vt[a] - vt[b]) * (rw2[a] + rw2[b] + 2 * np.sqrt(rw2[a] * rw2[b]))
    prob = oi.dt / dv * scl * interpolated_efficiency(tab, r_max, np.sqrt(rw2[a]), np.sqrt(rw2[b])) * geom
    u = rng.random(len(pa))
    rw2_max, vt_max = np.zeros(ncell), np.zeros(ncell)
    np.maximum.at(rw2_max, ijk, float_up(rw2)); np.maximum.at(vt_max, ijk, float_up(vt))
    assert (vt >= 0).all() and np.isfinite(rw2).all() and np.isfinite(vt).all()
    r_um = np.sqrt(rw2_max) * 1e6 * MARGIN
    x0 = np.where(r_um >= 100, np.floor(r_um / 10) * 10, np.floor(r_um))
    e_radius = np.where(r_um < r_max - 11, emax[np.minimum(kernel_index(x0), len(emax) - 1)], np.nan)
    base = oi.dt / dv * scl * n.max() * np.pi * 4 * rw2_max[cell] * vt_max[cell] * MARGIN
    n_lines = (len(c) + 15) // 16
    print("%s: %d pairs, largest pair probability %.3g, pairs that collide (u < prob) %.3g" % (label, len(pa), prob.max(), (u < prob).mean()))
    for name, e in (("table", np.full(ncell, tab.max())), ("radius", e_radius)):
        bound = base * e[cell]
        ok = ~(prob > bound)
        assert ok.all(), (name, int((~ok).sum()), float((prob / bound)[~ok].max()))
        skip = (bound < 1) & (u >= bound)
        assert not (skip & (u < prob)).any()
        kept = ~skip
        lines = np.unique(np.concatenate([pa[kept] // 16, pb[kept] // 16]))
        q = np.nanpercentile(bound, [1, 10, 50, 99])
        print("  %-6s bound: pairs kept %.5f, lines kept %.5f, skipped %.5f; bound quantiles 1 %% %.3g, 10 %% %.3g, median %.3g, 99 %% %.3g; cells with bound < 1: %.3f"
              % (name, kept.mean(), len(lines) / n_lines, skip.mean(), q[0], q[1], q[2], q[3], (bound < 1).mean()))
        if name == "radius":                                 # a pair belongs to the group of the lane that owns it: position pa or pa - 1, the same group
            groups = np.unique(pa[kept] // group)
            print("         groups of %d positions with a kept pair %.4f (%d of %d), cells with a kept pair %.4f, pairs that collide %d"
                  % (group, len(groups) / ((len(c) + group - 1) // group), len(groups), (len(c) + group - 1) // group,
                     len(np.unique(cell[kept])) / ncell, int((u < prob).sum())))
            if prevote:
                # the cells' vote: a cell is kept iff it holds a kept pair (the bound is the cell's, so that is `not (bound_c < 1 and umin_c >=
                # bound_c)` with umin_c the smallest draw of its pairs) or its bound is NaN; a kept cell flags every group its stretch overlaps
                kc = np.union1d(np.unique(cell[kept]), np.nonzero(np.isnan(e) & (cnt >= 2))[0])
                flagged = np.zeros((len(c) + group - 1) // group, dtype=bool)
                for t0, t1 in zip(start[kc] // group, (start[kc + 1] - 1) // group):
                    flagged[t0:t1 + 1] = True
                assert flagged[groups].all()                 # (the vote only errs toward keeping)
                print("         prevote: groups flagged through their cells %.4f (%d)  |  groups that hold a kept pair %.4f (%d)  |  flagged off %.4f"
                      % (flagged.mean(), flagged.sum(), len(groups) / len(flagged), len(groups), 1 - flagged.mean()))
            if not kept.any():
                continue
            per_group = np.bincount(pa[kept] // group)
            print("         kept pairs in a group that has any: mean %.2f, most %d; bound of the kept pairs' cells: median %.3g, below 1: %.3f"
                  % (per_group[per_group > 0].mean(), per_group.max(), np.median(bound[kept]), (bound[kept] < 1).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--workload", default="stratocumulus", choices=["stratocumulus", "coal-stress"])
    ap.add_argument("--dt", type=float, default=1.)
    ap.add_argument("--steps", default="5,50,200")
    ap.add_argument("--sd", type=int, default=64)
    ap.add_argument("--group", type=int, default=512)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--sparse", default=None, metavar="K:R")
    ap.add_argument("--prevote", action="store_true")
    args = ap.parse_args()
    at = sorted(int(s) for s in args.steps.split(","))
    n = args.n
    oi = bench.make_opts_init(n, n, n, args.sd, 40., 1, 1, 44, args.workload, args.dt)
    r_max, tab = load_table(oi.kernel)
    emax = efficiency_maxima(tab)
    print("kernel %s: table maximum %.4g, maximum reachable up to 15 um %.4g" % (lgrngn.kernel_t(oi.kernel).name, tab.max(), emax[15]))
    th, rv, rhod, Cx, Cy, Cz = bench.make_fields(n, n, n, 0, n, np, np.float64)
    orc = h.oracle_omp_particles(oi)
    orc.init(th, rv, rhod, Cx=Cx, Cy=Cy, Cz=Cz)
    if args.mixed:
        x, rw2, rd3 = orc.get_attr("x"), orc.get_attr("rw2"), orc.get_attr("rd3")
        low = x < 0.5 * oi.x1
        rw2[low] *= 1e-4; rd3[low] *= 1e-6
        orc.set_particles(orc.state_u64("n"), rd3, rw2, orc.get_attr("kappa"), orc.state_real("vt"), x, orc.get_attr("y"), orc.get_attr("z"))
    if args.sparse:
        K, R = (int(v) for v in args.sparse.split(":"))
        x, y, z, rw2, rd3 = orc.get_attr("x"), orc.get_attr("y"), orc.get_attr("z"), orc.get_attr("rw2"), orc.get_attr("rd3")
        cell = ((x // oi.dx).astype(np.int64) * oi.ny + (y // oi.dy).astype(np.int64)) * oi.nz + (z // oi.dz).astype(np.int64)
        low = cell % K != R
        big = np.nonzero(~low)[0]
        print("sparse: %d droplets in %d cells become drops" % (len(big), len(np.unique(cell[big]))))
        rw2[low] *= 1e-4; rd3[low] *= 1e-6
        rw2[big[0::2]], rw2[big[1::2]], rd3[big] = 100e-6 ** 2, 50e-6 ** 2, 1e-6 ** 3
        orc.set_particles(np.full(len(x), 25 * 10 ** 8, dtype=np.uint64), rd3, rw2, orc.get_attr("kappa"), orc.state_real("vt"), x, y, z)
    opts = lgrngn.opts_t()
    rng = np.random.default_rng(7)
    for step in range(1, at[-1] + 1):
        orc.step_sync(opts, th, rv, rhod, Cx, Cy, Cz)
        if step in at:                                       # what this step's coalescence will see: the droplets behind condensation, velocities fresh
            orc.stage("hskpng_Tpr"); orc.stage("hskpng_vterm_all")
            if args.sparse and step == at[0]:                # (the cell index restated above is the library's)
                x, y, z = orc.get_attr("x"), orc.get_attr("y"), orc.get_attr("z")
                mine = ((x // oi.dx).astype(np.int64) * oi.ny + (y // oi.dy).astype(np.int64)) * oi.nz + (z // oi.dz).astype(np.int64)
                assert np.array_equal(mine, orc.state_u64("ijk").astype(np.int64))
            gate(orc, oi, tab, r_max, emax, rng, "step %d" % step, args.group, args.prevote)
        orc.step_async(opts)


if __name__ == "__main__":
    main()
