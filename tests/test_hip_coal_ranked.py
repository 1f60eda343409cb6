"""The coalescence kernel that ranks each cell's shuffled order for itself (k_coal_ranked) against the separate ranking kernel.

Since round 7 the in-cell order of a carried re-sort is OWED, not made: the production coalescence stages the shuffle keys of the cells its
positions touch, ranks them in LDS and pairs the droplets up from there; the ranked order is written to memory only for somebody else who
reads it (raw_sorted_id, diagnostics, a second coalescence substep, ...).  dbg_flags & NO_RANK_IN_COAL keeps rounds 1-6's form: the
ranking as a kernel of its own next to the per-cell finish.  The keys are unique, so there is ONE order: the same pairs, the same random
number by position, the same state bit for bit -- every comparison here is np.array_equal.

Which path a step took is read back from the object ("raw_coal_ranked": the coalescence launches of the last step_async that ranked for
themselves), never assumed.  The fused object is read only at the end: a read of the order in between would make it in memory.
"""
import collections

import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

STEPS = 4
NO_RANK_IN_COAL = int(lgrngn.dbg.NO_RANK_IN_COAL)


def headline_opts(nx, ny, nz, sd_conc, **kw):
    """bench.py's headline arithmetic and kernel on a small box: fast arithmetic, the lean solver, hall_pinsky_stratocumulus"""
    return h.box_opts(nx, ny, nz, sd_conc, strict_fp=False, cond_solver=0, kernel=lgrngn.kernel_t.hall_pinsky_stratocumulus, **kw)


def coal_stress_opts(nx, ny, nz, sd_conc, **kw):
    """the coal-stress set-up of bench.make_opts_init: drizzle-sized drops that do collide (expvolume spectrum, hall_davis_no_waals)"""
    oi = h.box_opts(nx, ny, nz, sd_conc, strict_fp=False, cond_solver=0, kernel=lgrngn.kernel_t.hall_davis_no_waals, **kw)
    oi.dry_distros = {(1e-10, 0.): lgrngn.expvolume(30.084e-6, 2 ** 23)}
    return oi


def ranked(prt):
    return int(prt.state_u64("raw_coal_ranked")[0])


def state_of(prt, th, rv):
    return {"n": prt.state_u64("n"), "rw2": prt.get_attr("rw2"), "rd3": prt.get_attr("rd3"), "vt": prt.state_real("vt"),
            "x": prt.get_attr("x"), "y": prt.get_attr("y"), "z": prt.get_attr("z"), "kappa": prt.get_attr("kappa"),
            "th": np.array(th, dtype=np.float64), "rv": np.array(rv, dtype=np.float64)}


def assert_same_state(a, b):
    for name in a:
        assert np.array_equal(a[name], b[name]), name


def run(oi, fields, switched, real_t=np.float64, steps=STEPS, opts=None, prepare=None, between=None):
    """`steps` full steps; returns (state, [raw_coal_ranked after every step_async], n before the first step, whatever `between` returned).
    prepare(prt): after init; between(prt, step): between step_sync and step_async"""
    oi.dbg_flags = NO_RANK_IN_COAL if switched else 0
    prt = h.hip_particles(oi, real_t)
    f = lambda a: np.array(a, dtype=real_t, order="C")      # (copies: step_sync writes th and rv in place)
    th, rv, rhod, C = fields
    th, rv, rhod, C = f(th), f(rv), f(rhod), {k: f(v) for k, v in C.items()}
    prt.init(th, rv, rhod, **C)
    if prepare:
        prepare(prt)
    n0 = prt.state_u64("n")
    opts = opts or lgrngn.opts_t()
    flags, seen = [], []
    for step in range(steps):
        prt.step_sync(opts, th, rv, rhod, **C)
        if between:
            seen.append(between(prt, step))
        prt.step_async(opts)
        flags.append(ranked(prt))
    h.assert_mode(prt, False, 0, "lean")
    assert bool(prt.mode()[3] & NO_RANK_IN_COAL) == switched
    return state_of(prt, th, rv), flags, n0, seen


def n_changed(n0, n1):
    """super-droplets whose multiplicity is not what it was (a lower bound where some were used up and left the storage)"""
    if len(n0) == len(n1):
        return int((n0 != n1).sum())
    return sum((collections.Counter(n0.tolist()) - collections.Counter(n1.tolist())).values())


# where the ranking can go wrong: hundreds of cells per workgroup with cells of 0 or 1 droplets and odd counts; the production 64; cells that
# straddle workgroups (127, 128); a 2-D box.  150 and 230 per cell: above CELLRANK_MAX / 2 = 128 droplets per cell ON AVERAGE the object
# lists no cells and orders every cell by one wave (every_cell_by_a_wave, round 5) -- such a box does not take the fused path, by the
# library's rule and not by measurement, and must say so; cells of that size in a box that does take it: the test below
SHAPES = [(1, (20, 18, 22)), (3, (9, 7, 11)), (64, (6, 5, 7)), (127, (4, 4, 4)), (128, (4, 4, 4)), (150, (5, 4, 6)), (230, (4, 4, 5)), (64, (40, 0, 30))]
CASES = [(sd, dims, np.float64) for sd, dims in SHAPES] + [(64, (6, 5, 7), np.float32), (150, (5, 4, 6), np.float32)]


@pytest.mark.parametrize("sd_conc,dims,real_t", CASES)
@pytest.mark.parametrize("setup", ["headline", "coal_stress"])
def test_coalescence_that_ranks_for_itself_gives_the_same_bits(setup, sd_conc, dims, real_t):
    """four full steps (cond + coal + adve + sedi), fused and switched: every attribute and the caller's th and rv, bit for bit; the fused
    object ranks in its coalescence kernel in every step, the switched one in none; coal-stress: droplets do collide"""
    oi = (headline_opts if setup == "headline" else coal_stress_opts)(*dims, sd_conc)
    fields = h.box_fields(oi)
    fused, f_flags, _, _ = run(oi, fields, False, real_t)
    plain, p_flags, n0, _ = run(oi, fields, True, real_t)
    print("raw_coal_ranked", f_flags, p_flags, "n changed", n_changed(n0, plain["n"]))
    assert f_flags == [1 if sd_conc <= 128 else 0] * STEPS
    assert p_flags == [0] * STEPS
    assert_same_state(fused, plain)
    if setup == "coal_stress":
        # (about 1 % of the candidate pairs per second: 6 720 pairs give about 65 collisions per step at dt = 1)
        assert n_changed(n0, plain["n"]) >= 10


@pytest.mark.parametrize("real_t", [np.float64, np.float32])
def test_cells_of_up_to_256_droplets_straddling_workgroups_are_ranked_in_the_kernel(real_t):
    """184, 230 and 256 droplets in three cells of a box of 64 per cell (none above the in-kernel ranking's limit, so none is listed): cells
    whose overhang beyond a workgroup's 512 positions is as long as the kernel's window allows -- fused in every step, the same bits"""
    oi = coal_stress_opts(6, 5, 7, 64)
    fields = h.box_fields(oi)

    def crowd(prt):
        x, y, z = prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z")
        # (cells of 64 at init: 120, 166 and 192 more droplets, taken from 35, 35 and 40 other cells' last few)
        for sl, cell in ((slice(1000, 1120), (1, 1, 1)), (slice(5000, 5166), (3, 2, 4)), (slice(9000, 9192), (5, 4, 6))):
            x[sl], y[sl], z[sl] = (cell[0] + .5) * oi.dx, (cell[1] + .5) * oi.dy, (cell[2] + .5) * oi.dz
        prt.set_particles(prt.state_u64("n"), prt.get_attr("rd3"), prt.get_attr("rw2"), prt.get_attr("kappa"), prt.state_real("vt"), x, y, z)

    opts = lgrngn.opts_t()
    opts.adve = opts.sedi = False                          # (the crowds stay together)
    fused, f_flags, _, _ = run(oi, fields, False, real_t, opts=opts, prepare=crowd)
    plain, p_flags, n0, _ = run(oi, fields, True, real_t, opts=opts, prepare=crowd)
    assert f_flags == [1] * STEPS
    assert p_flags == [0] * STEPS
    assert_same_state(fused, plain)
    assert n_changed(n0, plain["n"]) >= 10
    oi.dbg_flags = 0
    prt = h.hip_particles(oi, real_t)
    f = lambda a: np.array(a, dtype=real_t, order="C")
    th, rv, rhod, C = fields
    prt.init(f(th), f(rv), f(rhod), **{k: f(v) for k, v in C.items()})
    crowd(prt)
    cnt = np.diff(prt.state_u64("cell_start").astype(np.int64))
    assert cnt.max() <= 256 and (cnt > 128).sum() >= 3 and cnt.max() > 200


def test_crowded_cells_fall_back_to_the_separate_ranking():
    """184 droplets in one cell and 394 in another (above the limit of the in-kernel ranking: listed, sorted by one wave): the step takes
    the separate kernels, says so, and ends in the switched run's state"""
    oi = headline_opts(6, 5, 7, 64)
    fields = h.box_fields(oi)

    def crowd(prt):
        x, y, z = prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z")
        for sl, cell in ((slice(1000, 1120), (1, 1, 1)), (slice(5000, 5330), (3, 2, 4))):
            x[sl], y[sl], z[sl] = (cell[0] + .5) * oi.dx, (cell[1] + .5) * oi.dy, (cell[2] + .5) * oi.dz
        prt.set_particles(prt.state_u64("n"), prt.get_attr("rd3"), prt.get_attr("rw2"), prt.get_attr("kappa"), prt.state_real("vt"), x, y, z)

    opts = lgrngn.opts_t()
    opts.adve = opts.sedi = False                          # (the crowd stays together)
    res = []
    for switched in (False, True):
        prt_state, flags, _, _ = run(oi, fields, switched, steps=3, opts=opts, prepare=crowd)
        assert flags == [0, 0, 0]
        res.append(prt_state)
    assert_same_state(res[0], res[1])
    oi.dbg_flags = 0
    prt = h.hip_particles(oi)
    th, rv, rhod, C = fields
    prt.init(th, rv, rhod, **C)
    crowd(prt)
    cnt = np.diff(prt.state_u64("cell_start").astype(np.int64))
    assert cnt.max() > 300 and ((cnt > 150) & (cnt <= 256)).any()


def test_an_order_that_somebody_reads_is_made_in_memory():
    """raw_sorted_id read between step_sync and step_async of the second step: the order that the switched object reports, that step's
    coalescence on the separate path, the next one -- unread -- on the fused path again, the same final state"""
    oi = coal_stress_opts(6, 5, 7, 64)
    fields = h.box_fields(oi)
    read = lambda prt, step: prt.state_u64("raw_sorted_id") if step == 1 else None
    fused, f_flags, _, f_seen = run(oi, fields, False, between=read)
    plain, p_flags, _, p_seen = run(oi, fields, True, between=read)
    assert np.array_equal(f_seen[1], p_seen[1])
    assert not np.array_equal(f_seen[1], np.sort(f_seen[1]))       # (a shuffled order, not the ids ascending)
    assert f_flags == [1, 0, 1, 1]
    assert p_flags == [0] * STEPS
    assert_same_state(fused, plain)


def test_the_first_of_three_coalescence_substeps_ranks_for_itself():
    """sstp_coal = 3: the first substep's order is the owed one (fused), the later ones re-shuffle the same cells with the separate kernel"""
    oi = coal_stress_opts(6, 5, 7, 64, sstp_coal=3)
    fields = h.box_fields(oi)
    fused, f_flags, _, _ = run(oi, fields, False)
    plain, p_flags, n0, _ = run(oi, fields, True)
    assert f_flags == [1] * STEPS
    assert p_flags == [0] * STEPS
    assert_same_state(fused, plain)
    assert n_changed(n0, plain["n"]) >= 10
