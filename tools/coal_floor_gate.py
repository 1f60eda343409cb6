"""CPU gate of the floor under the cell maxima of the coalescence bound (csrc/lcx_coal_prevote.hpp coal_cmax_floor; EXPERIMENTS.md 7.21): on the
droplets of the OpenMP oracle on bench.py's fields, how many droplets rise above the floor in either word (the ones that still offer to
their cell's maxima in k_vterm_b77<.., CELLMAX>), how many waves of the pass hold one, and how many cells the vote keeps with the floor
against without it.

    python3 tools/coal_floor_gate.py [--n 16] [--sd 64] [--workload stratocumulus|coal-stress] [--dt 1] [--steps 5,50,100,200] [--eps 16,14,13,10]

The floor's words are the library's own (lcx_coal_cmax_floor in liblcx_hip.so calls the function that the device runs), for the box's cell
volume, the scale factor of --sd droplets in a cell and the largest multiplicity in the oracle's storage.  A wave of the pass covers two
stretches of 128 neighbours in storage; the gate walks the ORACLE's storage order (production re-orders its storage by cell, which puts a
wave into fewer cells: not modelled).  The bound, the draws and the pairing are those of tools/coal_skip_gate.py.
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np                                            # noqa: E402
import bench                                                  # noqa: E402
import _harness as h                                          # noqa: E402
import coal_skip_gate as g                                    # noqa: E402
from libcloudphxx_amd import _lib, lgrngn                     # noqa: E402


def library_floor(dt, dv, scl, n_max, r_max, emax, eps):
    lib = _lib.load()
    lib.lcx_coal_cmax_floor.restype = None
    lib.lcx_coal_cmax_floor.argtypes = [C.c_double] * 5 + [C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(C.c_uint)]
    e = np.ascontiguousarray(emax, dtype=np.float64)
    w = (C.c_uint * 2)()
    lib.lcx_coal_cmax_floor(dt, dv, scl, n_max, r_max, e.ctypes.data_as(C.POINTER(C.c_double)), len(e), eps, w)
    return np.array([w[0], w[1]], dtype=np.uint32).view(np.float32).astype(np.float64)


def gate(orc, oi, sd, r_max, emax, rng, eps_log2, label):
    n, rw2, vt, ijk = orc.state_u64("n").astype(np.float64), orc.get_attr("rw2"), orc.state_real("vt"), orc.state_u64("ijk").astype(np.int64)
    ncell, dv = oi.nx * oi.ny * oi.nz, oi.dx * oi.dy * oi.dz
    cnt = np.bincount(ijk, minlength=ncell).astype(np.float64)
    scl = np.where(cnt > 1, (cnt * (cnt - 1) / 2) / np.maximum(np.floor(cnt / 2), 1), 0.)
    umin = np.array([rng.random(int(c) // 2).min() if c >= 2 else np.inf for c in cnt])
    r_up, v_up = g.float_up(rw2), g.float_up(vt)
    print("%s: %d droplets, radius quantiles 50 / 99 / 100 %%: %.2f / %.2f / %.2f um" % ((label, len(n)) + tuple(np.percentile(np.sqrt(rw2), [50, 99, 100]) * 1e6)))

    def kept_cells(rm, vm):
        r_um = np.sqrt(rm) * 1e6 * g.MARGIN
        x0 = np.where(r_um >= 100, np.floor(r_um / 10) * 10, np.floor(r_um))
        e = np.where(r_um < r_max - 11, emax[np.minimum(g.kernel_index(x0), len(emax) - 1)], np.nan)
        bound = np.maximum(oi.dt / dv * scl * n.max() * np.pi * 4 * rm * vm * e * g.MARGIN, 1e-30) * g.MARGIN
        return (cnt >= 2) & ~((bound < 1) & (umin >= bound))

    rm0, vm0 = np.zeros(ncell), np.zeros(ncell)
    np.maximum.at(rm0, ijk, r_up); np.maximum.at(vm0, ijk, v_up)
    today = kept_cells(rm0, vm0)
    for e2 in eps_log2:
        rf2, vf = library_floor(oi.dt, dv, (sd * (sd - 1) / 2) / (sd // 2), n.max(), r_max, emax, 2. ** -e2)
        above = (r_up > rf2) | (v_up > vf)
        waves = np.add.reduceat(above, np.arange(0, len(above), 128)) > 0          # (a wave's two stretches taken apart: an upper bound on whole waves)
        with_floor = kept_cells(np.maximum(rm0, rf2), np.maximum(vm0, vf))
        assert not (today & ~with_floor).any()                                     # (the floor only keeps more)
        print("  eps 2^-%d: R_f %.2f um, V_f %.4g m/s; droplets above the floor %.4f, stretches of 128 with one %.3f; cells kept %.5f (today %.5f)"
              % (e2, np.sqrt(rf2) * 1e6, vf, above.mean(), waves.mean(), with_floor.mean(), today.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--workload", default="stratocumulus", choices=["stratocumulus", "coal-stress"])
    ap.add_argument("--dt", type=float, default=1.)
    ap.add_argument("--steps", default="5,50,100,200")
    ap.add_argument("--sd", type=int, default=64)
    ap.add_argument("--eps", default="16,14,13,10", help="the bounds to try, as -log2")
    args = ap.parse_args()
    at = sorted(int(s) for s in args.steps.split(","))
    n = args.n
    oi = bench.make_opts_init(n, n, n, args.sd, 40., 1, 1, 44, args.workload, args.dt)
    r_max, tab = g.load_table(oi.kernel)
    emax = g.efficiency_maxima(tab)
    th, rv, rhod, Cx, Cy, Cz = bench.make_fields(n, n, n, 0, n, np, np.float64)
    orc = h.oracle_omp_particles(oi)
    orc.init(th, rv, rhod, Cx=Cx, Cy=Cy, Cz=Cz)
    opts = lgrngn.opts_t()
    rng = np.random.default_rng(7)
    for step in range(1, at[-1] + 1):
        orc.step_sync(opts, th, rv, rhod, Cx, Cy, Cz)
        if step in at:                                       # what this step's coalescence will see: the droplets behind condensation, velocities fresh
            orc.stage("hskpng_Tpr"); orc.stage("hskpng_vterm_all")
            gate(orc, oi, args.sd, r_max, emax, rng, [int(s) for s in args.eps.split(",")], "step %d" % step)
        orc.step_async(opts)


if __name__ == "__main__":
    main()
