"""The box that tests/test_hip_cond_rates.py tallies, run on the strict CPU oracle (no GPU): one step_sync of condensation must make every
row of include/lcx_cond_rates.h's table occur, or the device test would pass on an empty case.  Judged through the long-double reference
(tests/_cond_rates_reference.py) alone.

The box: 4 x 4 cells of 1 m, dt = 1 s, occupancies OCC (527 droplets, not a multiple of 64: cell runs end inside a wave, span waves and span
a workgroup; one cell is empty), th = 289, rhod = 1.1, rv = 9.5e-3 where (i + k) is even (supersaturated) and 6.0e-3 where odd (dry).
Thresholds 1 um, 1.5 um and 25 um.  70 % of the radii sit at a threshold times 1 +- delta, delta log-uniform in [1e-6, 3e-2]; the others
are log-uniform in 0.2 ... 80 um.  n in 1 ... 2000, kappa = 0.5, rd3 = (1e-8 (1 + id / 7))^3: unique per droplet and unchanged by
condensation, so it identifies a droplet."""
import numpy as np
import pytest

import _harness as h
import _cond_rates_reference as CD
from libcloudphxx_amd import lgrngn

LD = np.longdouble
OCC = [0, 1, 2, 3, 5, 63, 64, 65, 300, 2, 2, 2, 3, 5, 8, 2]
THR = [1e-6, 1.5e-6, 25e-6]
N_CELL = 16


def design(real_t, seed=3, **kw):
    kw.setdefault("coal_switch", False)
    oi = h.box_opts(4, 0, 4, 2, dx=1., dt=1., n_sd_max=sum(OCC) + 16, sedi_switch=False, kernel=lgrngn.kernel_t.geometric,
                    terminal_velocity=lgrngn.vt_t.beard76, **kw)
    f = lambda x: np.ascontiguousarray(x, dtype=real_t)
    th, rhod = np.full((4, 4), 289.), np.full((4, 4), 1.1)
    rv = np.where((np.indices((4, 4)).sum(0) % 2) == 0, 9.5e-3, 6.0e-3)
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.arange(N_CELL), OCC)
    N = cells.size
    t = np.array(THR)[rng.integers(0, 3, N)]
    delta = np.exp(rng.uniform(np.log(1e-6), np.log(3e-2), N)) * rng.choice([-1, 1], N)
    r = t * (1 + delta)
    far = rng.random(N) < .3
    r[far] = np.exp(rng.uniform(np.log(.2e-6), np.log(80e-6), far.sum()))
    rw2 = (r.astype(LD) ** 2).astype(real_t)
    n = rng.integers(1, 2000, N).astype(np.uint64)
    rd3 = (1e-8 * (1 + np.arange(N) / 7.)) ** 3
    i, k = cells // 4, cells % 4
    args = dict(n=n, rd3=rd3, rw2=rw2.astype(np.float64), kpa=np.full(N, .5), vt=np.zeros(N), x=(i + .5) * oi.dx, z=(k + .5) * oi.dz)
    return dict(oi=oi, fields=(f(th), f(rv), f(rhod)), cells=cells, args=args)


def permuted(case, perm):
    """the same droplets handed over in another storage order"""
    out = dict(case, cells=case["cells"][perm], args={k: v[perm] for k, v in case["args"].items()})
    return out


def cond_only():
    opts = lgrngn.opts_t()
    opts.coal = opts.adve = opts.sedi = False
    opts.cond = True
    return opts


def raw(prt, real_t, prefix=""):
    return dict(n=prt.state_u64(prefix + "n"), ijk=prt.state_u64(prefix + "ijk").astype(np.int64), rw2=prt.state_real(prefix + "rw2").astype(real_t),
                rd3=prt.state_real(prefix + "rd3"))


def one_step(prt, case, real_t):
    """(state before, state after, rv before, rv after) of one step_sync of condensation"""
    th, rv, rhod = case["fields"]
    prt.init(th.copy(), rv.copy(), rhod.copy())
    prt.set_particles(**case["args"])
    before = raw(prt, real_t)
    th2, rv2 = th.copy(), rv.copy()
    prt.step_sync(cond_only(), th2, rv2, rhod.copy())
    return before, raw(prt, real_t), rv, rv2


@pytest.mark.parametrize("sstp", [1, 3], ids=["sstp1", "sstp3"])
@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_step_on_the_oracle_makes_every_row_occur(real_t, sstp):
    case = design(real_t, sstp_cond=sstp)
    prt = (h.oracle_particles if real_t is np.float64 else h.oracle_f32_particles)(case["oi"])
    b, a, rv0, rv1 = one_step(prt, case, real_t)
    assert np.array_equal(b["ijk"], a["ijk"]) and np.array_equal(b["ijk"], case["cells"]), "cells and the slot order are unchanged across the call"
    assert np.array_equal(b["rd3"], a["rd3"]) and np.array_equal(b["n"], a["n"]) and np.unique(a["rd3"]).size == a["rd3"].size
    lo = CD.bounds(THR, real_t)
    rows = CD.tally(a["n"], a["ijk"], b["rw2"], a["rw2"], lo, N_CELL)
    big = [c for c, m in enumerate(OCC) if m >= 63]
    for t in range(3):
        assert rows.up[t].sum() >= 1 and rows.down[t].sum() >= 1, (t, rows.up[t], rows.down[t])
        assert (rows.up[t] + rows.down[t])[big].sum() >= 1, ("crossings in a cell of at least 63 droplets", t)
        assert any(rows.value(5 * t + CD.ABOVE_DM3, c) != 0 for c in range(N_CELL))
    assert (rows.up.sum(0) + rows.down.sum(0) == 0).any(), "at least one cell with no crossing at all"
    two_up = (b["rw2"] < lo[0]) & (a["rw2"] >= lo[1])
    two_down = (b["rw2"] >= lo[1]) & (a["rw2"] < lo[0])
    assert two_up.sum() >= 1 and two_down.sum() >= 1, (two_up.sum(), two_down.sum())
    assert rows.up.sum(0)[8] > 0 and rows.down.sum(0)[6] > 0, "upward crossings in the 300-droplet cell, downward ones in the 64-droplet cell"
    # the total closes against the cell's change of rv (strict arithmetic: to the rounding of rv)
    pred = -(LD(4) / 3 * LD(np.pi) * 1000 * np.array([rows.value(15, c) for c in range(N_CELL)], dtype=LD) / (LD(1) * LD(1.1)))
    got = (rv1.astype(LD) - rv0.astype(LD)).ravel()
    assert np.abs(pred - got).max() <= 4 * np.finfo(real_t).eps * rv0.max()
