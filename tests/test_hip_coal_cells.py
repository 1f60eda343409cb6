"""One wave per kept cell instead of ranking whole tiles (round 11: k_coal_cells, the list that k_coal_cellvote leaves; EXPERIMENTS.md 7.17).

The cells' vote ahead of the coalescence launch (tests/test_hip_coal_prevote.py) knows the cells that hold a kept pair.  It now appends them to
a list and counts them, and where the last polled vote kept few cells the launch is k_coal_cells: the waves of a fixed grid stride over the
list, a wave ranks its cell's keys by counting and runs the tile kernel's coal_collide on the kept pairs.  dbg_flags2 & NO_COAL_CELL_LIST
launches round 10's form (k_coal_ranked<.., TILES>): every comparison here is the list form against that twin -- np.array_equal on the bits of
n, rd3, rw2, kappa, vt, x, y, z and of the caller's th and rv, equal counts of collided pairs step by step -- in f64 and f32, fast and strict
arithmetic.  COAL_CELL_LIST_ALWAYS forces the list form from the first bound launch on; COAL_CELL_LIST_SMALL launches it on one workgroup and
ranks cells above 64 droplets by counting in memory (the path of a cell above 256, which the host never hands over).

"raw_coal_cells" of the last step_async = (launches in the list form, kept cells, cells with a pair).  The loops read it after every step,
which waits for the device: the vote's counts have then arrived when the next step_async polls them.

The boxes and helpers are those of test_hip_coal_prevote.py, test_hip_coal_rank_exit.py and test_hip_coal_skip.py.
"""
import functools

import numpy as np
import pytest

import _harness as h
import bench
from libcloudphxx_amd import lgrngn
from test_hip_coal_prevote import R_THR, off_shares, used
from test_hip_coal_rank_exit import ALWAYS as EXIT_ALWAYS, BOXES, WG, fields
from test_hip_coal_skip import ARITH, ARITH_IDS, assert_same_state, state_of

pytestmark = pytest.mark.gpu

NO_LIST = int(lgrngn.dbg2.NO_COAL_CELL_LIST)
LIST_ALWAYS = int(lgrngn.dbg2.COAL_CELL_LIST_ALWAYS)
LIST_SMALL = int(lgrngn.dbg2.COAL_CELL_LIST_SMALL)
FORCED = LIST_ALWAYS | EXIT_ALWAYS


class Run:
    pass


def all_shrunk(prt, oi):
    """no droplet can collide: every wet radius a hundredth, as the lower half of the mixed box"""
    prt.set_particles(prt.state_u64("n"), prt.get_attr("rd3") * 1e-6, prt.get_attr("rw2") * 1e-4, prt.get_attr("kappa"), prt.state_real("vt"),
                      prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z"))


# droplets per cell of the crafted box, 3 x 3 x 3 cells in the order of their index: a kept cell first (64) and last (65); empty cells in between;
# 1, 2 and 3 droplets -- the cell of 2 begins at the odd position 65, the cell of 3 at 67 and the cell of 63 behind that odd cell at 70; then
# 65, 129, 255 and 256.  945 droplets: n_part is odd.
CRAFTED = [64, 0, 1, 2, 3, 63, 0, 65, 129, 255, 256, 0, 42] + [0] * 13 + [65]


def crafted_cells(prt, oi):
    assert len(CRAFTED) == 27 and sum(CRAFTED) == 945 == len(prt.state_u64("n"))
    cell = np.repeat(np.arange(27), CRAFTED)[np.random.default_rng(7).permutation(945)]         # (arrival order inside a cell: not the ids ascending)
    x, y, z = (cell // 9 + .5) * oi.dx, (cell // 3 % 3 + .5) * oi.dy, (cell % 3 + .5) * oi.dz
    rw2 = np.where(np.arange(945) % 2 == 0, 100e-6 ** 2, 50e-6 ** 2)
    prt.set_particles(np.full(945, 10 ** 14, dtype=np.uint64), np.full(945, 1e-6 ** 3), rw2, prt.get_attr("kappa"), prt.state_real("vt"), x, y, z)
    assert np.array_equal(np.diff(prt.state_u64("cell_start").astype(np.int64)), CRAFTED)


def half_drops(prt, oi):
    """the droplets of the lower half in x become the sparse box's drops (multiplicity 2.5e9, 100 um and 50 um in turn), the rest stays as it is"""
    x = prt.get_attr("x")
    low = np.nonzero(x < 0.5 * oi.x1)[0]
    assert 0.3 < len(low) / len(x) < 0.7
    n, rw2, rd3 = prt.state_u64("n"), prt.get_attr("rw2"), prt.get_attr("rd3")
    n[low], rw2[low[0::2]], rw2[low[1::2]], rd3[low] = 25 * 10 ** 8, 100e-6 ** 2, 50e-6 ** 2, 1e-6 ** 3
    prt.set_particles(n, rd3, rw2, prt.get_attr("kappa"), prt.state_real("vt"), x, prt.get_attr("y"), prt.get_attr("z"))


PREPARE = {"all_shrunk": all_shrunk, "half_drops": half_drops, "crafted": crafted_cells}


def run(box, n, sd, real_t, strict, steps, flags2, prepare=None, still=False, change_at=-1, change=None, rates=False, restore_at=-1):
    """`steps` full steps of one of BOXES on n^3 cells x sd.  prepare / change: names in PREPARE, applied after init / between step_sync and
    step_async of step change_at.  still: no advection, no sedimentation, no condensation.  restore_at: after that step the object is replaced by a fresh one
    that restores its snapshot."""
    workload, dt, box_prepare = BOXES[box]
    oi = bench.make_opts_init(n, n, n, sd, 40., 1, 1, 44, workload, dt)
    oi.strict_fp, oi.cond_solver = bool(strict), 0
    oi.dbg_flags, oi.dbg_flags2 = 0, flags2
    prt = h.hip_particles(oi, real_t)
    f = lambda a: np.array(a, dtype=real_t, order="C")
    th, rv, rhod, C = fields(n)
    th, rv, rhod, C = f(th), f(rv), f(rhod), {k: f(v) for k, v in C.items()}
    prt.init(th, rv, rhod, **C)
    if prepare:
        PREPARE[prepare](prt, oi)
    elif box_prepare:
        box_prepare(prt, oi)
    if rates:
        prt.coal_rates_enable(R_THR)
    opts = lgrngn.opts_t()
    if still:
        opts.adve = opts.sedi = opts.cond = False
    r = Run()
    r.cells, r.pv, r.skip, r.exit_form, r.ranked, r.collided = [], [], [], [], [], []
    for step in range(steps):
        prt.step_sync(opts, th, rv, rhod, **C)
        if step == change_at:
            PREPARE[change](prt, oi)
        prt.step_async(opts)
        r.cells.append([int(v) for v in prt.state_u64("raw_coal_cells")])
        r.pv.append([int(v) for v in prt.state_u64("raw_coal_prevote")])
        r.skip.append([int(v) for v in prt.state_u64("raw_coal_skip")])
        r.exit_form.append(int(prt.state_u64("raw_coal_exit")[0]))
        r.ranked.append(int(prt.state_u64("raw_coal_ranked")[0]))
        r.collided.append(int(prt.state_u64("raw_collided")[0]))
        assert len(r.cells[-1]) == 3 and len(r.pv[-1]) == 4
        if step == restore_at:
            blob = prt.snapshot()
            prt = h.hip_particles(oi, real_t)
            prt.restore(blob)
    assert prt.mode()[0] == bool(strict) and prt.mode()[3] == 0
    r.n_part = len(prt.state_u64("raw_n"))
    r.rates = prt.coal_rates() if rates else None
    r.state = state_of(prt, th, rv)
    return r


@functools.lru_cache(maxsize=None)
def both(box, n, sd, real_t, strict, steps, flags2, **kw):
    """the list form and its NO_COAL_CELL_LIST twin, run once per case: the bits, the collisions and what the existing counters say compared"""
    on = run(box, n, sd, real_t, strict, steps, flags2, **kw)
    off = run(box, n, sd, real_t, strict, steps, (flags2 & ~(LIST_ALWAYS | LIST_SMALL)) | NO_LIST, **kw)
    print("cells", on.cells, "prevote", on.pv, "exit form", on.exit_form, "collided", on.collided)
    assert on.collided == off.collided
    assert_same_state(on.state, off.state)
    assert on.ranked == off.ranked
    if not flags2 & LIST_ALWAYS:           # (a forced launch's counts pause nothing, the twin's sample may: its later launches can be other forms)
        assert on.exit_form == off.exit_form and on.skip == off.skip and on.pv == off.pv
    assert all(c == [0, 0, 0] for c in off.cells), off.cells                 # (the twin makes no list)
    assert all(c[1] <= c[2] <= n ** 3 for c in on.cells), on.cells
    on.state = off.state = None
    return on, off


def launches(r):
    return [c[0] for c in r.cells]


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_stratocumulus_in_the_production_form(real_t, strict):
    """bench.py's stratocumulus box, 16^3 x 64, 20 steps, dbg_flags2 = 0 apart from the twin's bit.  The first bound launch knows no vote and is
    the tiles'; its vote keeps a few cells in a thousand, so from the second on the list form runs.  The existing counters read as in
    test_hip_coal_prevote.py's case of the same name: an exit-form launch handed the flags in every step, no fallback, every tile counted, at
    least 0.8 of them flagged off."""
    on, _ = both("stratocumulus", 16, 64, real_t, strict, 20, 0)
    assert launches(on) == [0] + [1] * 19, on.cells
    assert on.exit_form == [1] * 20 and on.ranked == [1] * 20
    assert used(on) == [1] * 20 and all(pv[3] == 0 for pv in on.pv), on.pv
    assert all(pv[2] == (on.n_part + WG - 1) // WG for pv in on.pv)
    assert min(off_shares(on)) >= 0.8, off_shares(on)
    assert all(c[1] * 100 <= c[2] * 6 and c[2] > 16 ** 3 * 0.9 for c in on.cells), on.cells


@pytest.mark.parametrize("box", ["mixed", "sparse"])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_collisions_in_the_forced_form(real_t, strict, box):
    """the mixed box and the sparse box, 16^3 x 64, 10 steps, the list form in every launch: the twin's bits and collided pairs (the sparse box
    at f64: 31 / 38 / 24 / 31 / 37 in the first five steps, EXPERIMENTS.md 7.10 -- a kernel that loses a kept pair or pairs up other members
    loses or changes collisions here); cells are kept in every step"""
    on, _ = both(box, 16, 64, real_t, strict, 10, FORCED)
    assert launches(on) == [1] * 10, on.cells
    assert min(c[1] for c in on.cells) > 0, on.cells
    assert sum(on.collided) >= 50, on.collided
    if box == "sparse" and real_t is np.float64 and not strict:
        assert on.collided[:5] == [31, 38, 24, 31, 37], on.collided


@pytest.mark.parametrize("small", [0, LIST_SMALL], ids=["in-lds", "by-counting-above-64"])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_cell_sizes_at_which_ranking_and_pairing_can_go_wrong(real_t, strict, small):
    """3 x 3 x 3 cells holding CRAFTED droplets each, all of them the sparse box's drops, nothing moves: cells of 1, 2, 3, 63, 64, 65, 129, 255
    and 256 (one, two, three and four entries per lane; an unpaired last droplet; padding beside the keys; multiplicity 1e14, so that
    the bound is above one in the cell of two as well, every pair is kept and a 100 um drop collects its 50 um partner; no condensation), a kept cell first in the order and
    one last, kept cells that begin at odd positions behind odd cells, empty cells in between, n_part odd.  Three steps, the form forced; and
    once more on one workgroup with the cells above 64 ranked by counting in memory, window by window."""
    on, _ = both("sparse", 3, 35, real_t, strict, 3, FORCED | small, prepare="crafted", still=True)
    assert launches(on) == [1] * 3 and on.ranked == [1] * 3, (on.cells, on.ranked)
    assert on.cells[0][1:] == [sum(s >= 2 for s in CRAFTED)] * 2 and all(c[1] > 0 for c in on.cells), on.cells
    assert on.collided[0] >= 50, on.collided


@pytest.mark.parametrize("n,small,real_t,strict", [(16, LIST_SMALL, np.float64, False), (16, LIST_SMALL, np.float32, True), (24, 0, np.float64, False)],
                         ids=["4096-cells-on-4-waves-f64", "4096-cells-on-4-waves-f32-strict", "13824-cells-on-8192-waves"])
def test_a_list_longer_than_the_waves_launched(n, small, real_t, strict):
    """the drizzle box, a kept pair in every cell, the form forced: 16^3 cells on one workgroup (1 024 entries per wave) and 24^3 cells on the
    capped grid of 2 048 workgroups.  Every listed cell is visited exactly once: the twin's collided counts and bits."""
    on, _ = both("drizzle", n, 64, real_t, strict, 4, FORCED | small)
    assert launches(on) == [1] * 4, on.cells
    assert all(c[1] > (4 if small else 8192) and c[2] == n ** 3 for c in on.cells), on.cells        # (waves launched: 4, 2 048 x 4)
    assert sum(on.collided) >= 50, on.collided


def test_the_drizzle_box_never_takes_the_list_form():
    """the drizzle box as production runs it: the first launch is the tiles', its vote keeps every cell and its sample shows no workgroup
    leaving; the launches afterwards are the twin's (round 8's form while the exit is paused), none in the list form"""
    on, _ = both("drizzle", 16, 64, np.float64, False, 6, 0)
    assert launches(on) == [0] * 6, on.cells
    assert on.cells[0][1] * 100 > on.cells[0][2] * 12 and on.cells[0][2] == 16 ** 3, on.cells
    assert on.exit_form == [1, 0, 0, 0, 0, 0] and used(on) == [1, 0, 0, 0, 0, 0], (on.exit_form, on.pv)


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_the_host_leaves_the_list_form_when_the_vote_fills_up(real_t, strict):
    """the coal-stress box at dt = 0.02, 8^3 x 64, with every droplet shrunk: the vote keeps no cell (a few in a hundred in f32, strict) and the list form runs on
    an empty or short list from the second launch on.  Between step_sync and step_async of the fifth step the droplets of the lower half in x become drops: that launch is
    still the list form (the host knows the vote before), on a list of four cells in ten; its vote is polled by the next step, and from then on
    the launches are the tiles'.  Half of the pairs are still skipped, so the bound is not paused, and the exit is held on
    (COAL_RANK_EXIT_ALWAYS), so that the vote goes on being taken.  The twin's bits throughout."""
    on, _ = both("mixed", 8, 64, real_t, strict, 8, EXIT_ALWAYS, prepare="all_shrunk", change_at=4, change="half_drops")
    assert launches(on) == [0, 1, 1, 1, 1, 0, 0, 0], on.cells
    assert used(on) == [1] * 8 and on.exit_form == [1] * 8, (on.pv, on.exit_form)
    assert all(c[1] * 100 <= c[2] * 6 for c in on.cells[:4]) and all(c[1] * 100 > c[2] * 6 for c in on.cells[4:]), on.cells
    assert sum(on.collided[4:]) >= 10 and sum(on.collided[:4]) == 0, on.collided


def test_a_restored_snapshot_starts_in_the_tiles_form():
    """stratocumulus, 16^3 x 64: after the sixth step the object is replaced by a fresh one that restores its snapshot.  The restored object
    knows no vote: its first launch is the tiles', the list form comes back with the launch after.  The twin's bits."""
    on, _ = both("stratocumulus", 16, 64, np.float64, False, 10, 0, restore_at=5)
    assert launches(on) == [0, 1, 1, 1, 1, 1, 0, 1, 1, 1], on.cells


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_with_the_collision_rates_on(real_t, strict):
    """coal_rates_enable: k_coal_cells<.., TALLY> runs coal_collide's tally as the tile kernel does.  The integer accumulators are the twin's
    byte for byte; the two M3 rows are sums of doubles added by atomics, whose order is not fixed: equal to 1e-12 (a cell's row sums at most a
    few hundred non-negative terms of relative error 2^-53 each)"""
    on, off = both("mixed", 16, 64, real_t, strict, 5, FORCED, rates=True)
    assert launches(on) == [1] * 5, on.cells
    moved = 0.
    for name in lgrngn.COAL_RATES:
        a, b = on.rates[name], off.rates[name]
        if name.endswith("_m3"):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        else:
            assert np.array_equal(a.view("u8"), b.view("u8")), name
            moved += a.sum()
    assert moved > 0
