"""The cells' vote ahead of the coalescence launch (round 10: csrc/lcx_coal_prevote.hpp, k_coal_umin, k_coal_cellvote).

k_coal_ranked<.., SKIP, EXIT> lets a workgroup leave where the bound rules out every pair of its 512 positions (tests/test_hip_coal_rank_exit.py).
The bound is the pair's cell's and the random number the pair's position's, so step_async now computes every cell's smallest draw beside the
velocity pass, one lane per cell decides whether the cell holds a kept pair and flags the tiles the cell overlaps, and a workgroup whose flag
is 0 returns on one load.  dbg_flags2 & NO_COAL_PREVOTE launches round 9's form, in which every workgroup votes for itself: every comparison
here is the change against that twin -- np.array_equal on the bits of every attribute and of the caller's th and rv, equal counts of
collided pairs step by step -- in f64 and f32, fast and strict arithmetic.

"raw_coal_prevote" of the last step_async = (launches handed the flags, tiles flagged off, tiles, launches that fell back because the draws
were made for another call, seed or set of cells); with dbg_flags2 & COAL_SKIP_COUNT no workgroup leaves on its flag, every workgroup votes
and counts as before, and a fifth number counts the workgroups flagged off whose own vote kept a pair.

The boxes and helpers are those of test_hip_coal_rank_exit.py and test_hip_coal_skip.py.
"""
import functools

import numpy as np
import pytest

import _harness as h
import bench
from libcloudphxx_amd import lgrngn
from test_hip_coal_rank_exit import ALWAYS, BOXES, WG, fields
from test_hip_coal_skip import ARITH, ARITH_IDS, COUNT, assert_same_state, state_of

pytestmark = pytest.mark.gpu

NO_PREVOTE = int(lgrngn.dbg2.NO_COAL_PREVOTE)
R_THR = 25e-6


class Run:
    pass


def shift_one_cell(prt, oi):
    """set_particles with every droplet moved one cell along x (periodic): the cells are rewritten, the droplets are the same"""
    x = (prt.get_attr("x") + oi.dx) % oi.x1
    prt.set_particles(prt.state_u64("n"), prt.get_attr("rd3"), prt.get_attr("rw2"), prt.get_attr("kappa"), prt.state_real("vt"), x, prt.get_attr("y"), prt.get_attr("z"))


def run(box, n, sd, real_t, strict, steps, prevote, count, always, sstp_coal=1, shift_at=-1, rates=False):
    workload, dt, prepare = BOXES[box]
    oi = bench.make_opts_init(n, n, n, sd, 40., 1, sstp_coal, 44, workload, dt)
    oi.strict_fp, oi.cond_solver = bool(strict), 0
    oi.dbg_flags = 0
    oi.dbg_flags2 = (COUNT if count else 0) | (ALWAYS if always else 0) | (0 if prevote else NO_PREVOTE)
    prt = h.hip_particles(oi, real_t)
    f = lambda a: np.array(a, dtype=real_t, order="C")
    th, rv, rhod, C = fields(n)
    th, rv, rhod, C = f(th), f(rv), f(rhod), {k: f(v) for k, v in C.items()}
    prt.init(th, rv, rhod, **C)
    if prepare:
        prepare(prt, oi)
    if rates:
        prt.coal_rates_enable(R_THR)
    opts = lgrngn.opts_t()
    r = Run()
    r.pv, r.skip, r.wg, r.exit_form, r.collided, r.ranked = [], [], [], [], [], []
    for step in range(steps):
        prt.step_sync(opts, th, rv, rhod, **C)
        if step == shift_at:
            shift_one_cell(prt, oi)
        prt.step_async(opts)
        pv = [int(v) for v in prt.state_u64("raw_coal_prevote")]
        assert len(pv) == (5 if count else 4)
        r.pv.append(pv)
        r.skip.append([int(v) for v in prt.state_u64("raw_coal_skip")])
        r.wg.append([int(v) for v in prt.state_u64("raw_coal_wg")])
        r.exit_form.append(int(prt.state_u64("raw_coal_exit")[0]))
        r.ranked.append(int(prt.state_u64("raw_coal_ranked")[0]))
        r.collided.append(int(prt.state_u64("raw_collided")[0]))
    assert prt.mode()[0] == bool(strict) and prt.mode()[3] == 0
    r.n_part = len(prt.state_u64("raw_n"))
    r.rates = prt.coal_rates() if rates else None
    r.state = state_of(prt, th, rv)
    return r


@functools.lru_cache(maxsize=None)
def both(box, n, sd, real_t, strict, steps, count, always, sstp_coal=1, shift_at=-1, rates=False):
    """the change and its NO_COAL_PREVOTE twin, run once per case: the bits, the collisions and the launches' forms compared"""
    on = run(box, n, sd, real_t, strict, steps, True, count, always, sstp_coal, shift_at, rates)
    off = run(box, n, sd, real_t, strict, steps, False, count, always, sstp_coal, shift_at, rates)
    print("prevote", on.pv, "wg", on.wg, "exit form", on.exit_form, "collided", on.collided)
    assert on.collided == off.collided
    assert_same_state(on.state, off.state)
    assert on.exit_form == off.exit_form and on.ranked == off.ranked
    assert [s[0] for s in on.skip] == [s[0] for s in off.skip]
    assert all(pv[:4] == [0, 0, 0, 0] for pv in off.pv)                    # (the twin makes no draws ahead and hands no flags)
    assert all(pv[4] == 0 for pv in off.pv if len(pv) == 5)
    on.state = off.state = None
    return on, off


def used(r):
    return [pv[0] for pv in r.pv]


def off_shares(r):
    return [pv[1] / max(pv[2], 1) for pv in r.pv]


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_stratocumulus_in_the_production_form(real_t, strict):
    """bench.py's stratocumulus box, 16^3 x 64, 20 steps, dbg_flags2 = 0 apart from the twin's bit: the same bits; the flags are used in every
    step -- the first included, where coal() draws the shuffle's salts first and the draws' call number is the one after the next -- and no
    launch falls back; at least 0.8 of the tiles are flagged off in every step.  (The threshold is the issue's condition: on the oracle's
    droplets tools/coal_skip_gate.py --prevote --group 512 flags 0.004 to 0.06 of the groups through their cells over the first 20 steps and
    0.13 at step 200, EXPERIMENTS.md 7.13.)"""
    on, _ = both("stratocumulus", 16, 64, real_t, strict, 20, False, False)
    assert on.exit_form == [1] * 20
    assert used(on) == [1] * 20, on.pv
    assert all(pv[3] == 0 for pv in on.pv), on.pv
    assert all(pv[2] == (on.n_part + WG - 1) // WG for pv in on.pv)
    assert min(off_shares(on)) >= 0.8, off_shares(on)


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_stratocumulus_counted(real_t, strict):
    """the same box with COAL_SKIP_COUNT: the flags are computed and handed over but no workgroup leaves on them, so the exact counters are
    the twin's; no workgroup that was flagged off keeps a pair, and no more tiles are flagged off than workgroups left"""
    on, off = both("stratocumulus", 16, 64, real_t, strict, 20, True, False)
    assert used(on) == [1] * 20 and all(pv[3] == 0 for pv in on.pv), on.pv
    assert all(pv[4] == 0 for pv in on.pv), on.pv
    assert on.skip == off.skip and on.wg == off.wg
    assert min(s[2] for s in on.skip) > 16 ** 3 * 64 // 2 * 0.9
    assert all(pv[1] <= wg[0] for pv, wg in zip(on.pv, on.wg)), (on.pv, on.wg)
    assert min(off_shares(on)) >= 0.8, off_shares(on)


@pytest.mark.parametrize("box", ["mixed", "sparse"])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_exits_and_collisions_in_one_launch(real_t, strict, box):
    """the mixed box and the sparse box, 16^3 x 64, 10 steps, the exit in every launch: the same bits and the same collided pairs as the twin
    with workgroups leaving on their flags (the sparse box at f64: 31 / 38 / 24 / 31 / 37 in the first five steps, EXPERIMENTS.md 7.10 -- a
    vote that loses a kept pair loses collisions here); some tiles are flagged off in every step; and with the counting bit no workgroup
    that was flagged off keeps a pair"""
    on, _ = both(box, 16, 64, real_t, strict, 10, False, True)
    assert used(on) == [1] * 10 and all(pv[3] == 0 for pv in on.pv), on.pv
    assert min(pv[1] for pv in on.pv) > 0, on.pv
    assert sum(on.collided) >= 50, on.collided
    if box == "sparse" and real_t is np.float64 and not strict:
        assert on.collided[:5] == [31, 38, 24, 31, 37], on.collided
    cnt, twin = both(box, 16, 64, real_t, strict, 10, True, True)
    assert used(cnt) == [1] * 10 and all(pv[3] == 0 and pv[4] == 0 for pv in cnt.pv), cnt.pv
    assert cnt.skip == twin.skip and cnt.wg == twin.wg
    assert cnt.collided == on.collided
    assert all(pv[1] <= wg[0] for pv, wg in zip(cnt.pv, cnt.wg)), (cnt.pv, cnt.wg)


@pytest.mark.parametrize("n,sd", [(2, 48), (3, 64)], ids=["one-partial-workgroup", "three-and-a-partial"])
@pytest.mark.parametrize("box", ["stratocumulus", "mixed", "drizzle"])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_edges_of_the_grid(real_t, strict, box, n, sd):
    """2 x 2 x 2 cells x 48 (384 droplets: ONE partial tile, which is also a sampled one and votes for itself in the uncounted form -- nothing
    straddles a border here, the case checks the partial tile and the sampled path) and 3 x 3 x 3 x 64 (1728: three tiles and a partial
    fourth).  5 steps of either box: the same bits with workgroups leaving on their flags, and no disagreement with the counting bit.  Cells
    across the tiles' borders: test_cells_across_tile_borders."""
    on, _ = both(box, n, sd, real_t, strict, 5, False, True)
    assert used(on) == [1] * 5 and all(pv[3] == 0 for pv in on.pv), on.pv
    assert all(pv[2] == (n ** 3 * sd + WG - 1) // WG for pv in on.pv), on.pv
    cnt, twin = both(box, n, sd, real_t, strict, 5, True, True)
    assert all(pv[4] == 0 for pv in cnt.pv), cnt.pv
    assert cnt.skip == twin.skip and cnt.wg == twin.wg
    assert all(pv[1] <= wg[0] for pv, wg in zip(cnt.pv, cnt.wg)), (cnt.pv, cnt.wg)


@pytest.mark.parametrize("box,n", [("stratocumulus", 3), ("mixed", 3), ("drizzle", 3), ("stratocumulus", 4), ("mixed", 4), ("drizzle", 4), ("sparse", 4),
                                   ("sparse", 8)])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_cells_across_tile_borders(real_t, strict, box, n):
    """48 droplets per cell and several tiles: 3^3 cells (1296 droplets, two tiles and a partial third), 4^3 (3072, six tiles) and, for the
    sparse box, 8^3 (24 576, 48 tiles).  512 is no multiple of 48, so at every border a cell lies across it (at init the cells [480, 528),
    [1008, 1056), ...) and has to flag both tiles.  The sparse box is the one that can tell: only the cells with index % 8 == 2 hold drops
    (stretches from 96 + 384 m on), so every fourth of them lies across a border ([480, 528) modulo 1536) while the only other cell of drops
    in the tile behind begins 352 positions into it.  Where such a cell is kept for one of its 8 pairs behind the border (a pair is kept once
    in twenty times: 0.34) and that other cell keeps none of its 24 (0.3), the tile is flagged by the cell that began in the tile before or
    not at all: once in ten times per border and step -- two such borders in the 4^3 box, sixteen in the 8^3 box, ten steps.  With a kept
    cell flagging only the tile of its first position the 8^3 case fails on the disagreements (EXPERIMENTS.md 7.13; the 4^3 case did not meet
    one in its 20 chances).  Same bits with workgroups leaving on their flags; with the counting bit no disagreement and the twin's exact
    counters."""
    steps = 10 if box == "sparse" else 5
    on, _ = both(box, n, 48, real_t, strict, steps, False, True)
    assert used(on) == [1] * steps and all(pv[3] == 0 for pv in on.pv), on.pv
    assert all(pv[2] == (n ** 3 * 48 + WG - 1) // WG for pv in on.pv), on.pv
    cnt, twin = both(box, n, 48, real_t, strict, steps, True, True)
    assert used(cnt) == [1] * steps and all(pv[3] == 0 for pv in cnt.pv), cnt.pv
    assert all(pv[4] == 0 for pv in cnt.pv), cnt.pv
    assert cnt.skip == twin.skip and cnt.wg == twin.wg
    assert cnt.collided == on.collided
    assert all(pv[1] <= wg[0] for pv, wg in zip(cnt.pv, cnt.wg)), (cnt.pv, cnt.wg)
    if box == "drizzle":
        assert all(pv[1] == 0 for pv in cnt.pv), cnt.pv
    if box == "sparse":
        assert sum(on.collided) > 0, on.collided


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_a_box_with_a_kept_pair_everywhere_flags_every_tile(real_t, strict):
    """the drizzle box at dt = 0.045, the exit in every launch: a kept pair in every workgroup, so every tile is flagged; the same bits"""
    on, _ = both("drizzle", 16, 64, real_t, strict, 6, False, True)
    assert used(on) == [1] * 6, on.pv
    assert all(pv[1] == 0 and pv[2] == 512 for pv in on.pv), on.pv
    assert sum(on.collided) >= 50, on.collided


def test_no_draws_are_made_while_the_exit_is_paused():
    """the drizzle box as production runs it: the first launch's sample shows no workgroup leaving, the following launches take round 8's
    form (test_a_box_in_which_no_workgroup_leaves_goes_back_to_ranking_everywhere) -- and then step_async makes no draws ahead"""
    on, _ = both("drizzle", 16, 64, np.float64, False, 6, False, False)
    assert on.exit_form == [1, 0, 0, 0, 0, 0]
    assert used(on) == [1, 0, 0, 0, 0, 0], on.pv
    assert all(pv[3] == 0 for pv in on.pv), on.pv
    assert sum(on.collided) >= 50, on.collided


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_three_coalescence_substeps(real_t, strict):
    """sstp_coal = 3 on the mixed box, 5 steps: the bound, the exit and the flags belong to the first substep alone (one launch per step is
    handed the flags, the other two pair up the order in memory); the same bits.  Pairs collide: "raw_collided" shows those of the last
    substep alone, which runs a third of the time step (the box has 8 to 16 collisions per whole step)"""
    on, _ = both("mixed", 16, 64, real_t, strict, 5, False, True, sstp_coal=3)
    assert used(on) == [1] * 5 and all(pv[3] == 0 for pv in on.pv), on.pv
    assert [s[0] for s in on.skip] == [1] * 5 and on.ranked == [1] * 5
    assert min(pv[1] for pv in on.pv) > 0, on.pv
    assert sum(on.collided) > 0, on.collided


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_the_cells_rewritten_between_step_sync_and_step_async(real_t, strict):
    """set_particles between step_sync and step_async of the third step moves every droplet one cell along x.  The draws are made inside
    step_async, from the cells as that call finds them (set_particles leaves them sorted, unshuffled: coal() then draws the salts first and
    the call number is the one after the next) -- so the flags are recomputed, the guard matches and nothing falls back.  The guard can only
    trip where coal() itself re-sorts, and step_async asks for no bound then.  The same bits."""
    on, _ = both("mixed", 16, 64, real_t, strict, 5, False, True, shift_at=2)
    assert used(on) == [1] * 5, on.pv
    assert all(pv[3] == 0 for pv in on.pv), on.pv
    assert min(pv[1] for pv in on.pv) > 0, on.pv


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_with_the_collision_rates_on(real_t, strict):
    """coal_rates_enable: the tallying form of the kernel takes the flags as well.  The integer accumulators are the twin's byte for byte;
    the two M3 rows are sums of doubles added by atomics, whose order is not fixed: equal to 1e-12 (a cell's row sums at most a few hundred
    non-negative terms of relative error 2^-53 each)"""
    on, off = both("mixed", 16, 64, real_t, strict, 5, False, True, rates=True)
    assert used(on) == [1] * 5 and min(pv[1] for pv in on.pv) > 0, on.pv
    moved = 0.
    for name in lgrngn.COAL_RATES:
        a, b = on.rates[name], off.rates[name]
        if name.endswith("_m3"):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        else:
            assert np.array_equal(a.view("u8"), b.view("u8")), name
            moved += a.sum()
    assert moved > 0
