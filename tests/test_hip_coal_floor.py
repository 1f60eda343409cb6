"""A floor under the cell maxima of the coalescence bound (round 12: lcx_coal_prevote.hpp coal_cmax_floor, k_vterm_b77<.., CELLMAX>;
EXPERIMENTS.md 7.21).

The velocity pass ahead of the coalescence collects every cell's largest rw2 and vt as the bits of floats rounded up.  The bound made of them
is monotone in both, so words above the true maxima only keep more cells: the words now start from a floor pair (R_f^2, V_f) instead of zero
and a droplet offers to them only where one of its words is above the floor's.  dbg_flags2 & NO_COAL_CMAX_FLOOR starts from zero with every
droplet offering, as before: the twin of every comparison here.  COAL_CMAX_FLOOR_HIGH puts the floor at a bound of 2^-6.

"raw_coal_cmax" = the 2 x n_cell words of the last pass that collected maxima, "raw_coal_cmax_floor" = the two words they started from.

The same round splits the vote's list of kept cells into 64 sub-lists with a cursor each ("raw_coal_kept_list": the sub-lists one behind the
other); the last test here holds them against the NO_COAL_CELL_LIST twin.

The invariant that defines the feature: word by word, floored == max(twin, floor) as unsigned integers (all ones, a poisoned cell, being the
largest).  Everything else is the twin's bits: np.array_equal on n, rd3, rw2, kappa, vt, x, y, z, th and rv, and equal collided pairs.

The boxes and helpers are those of test_hip_coal_cells.py, test_hip_coal_rank_exit.py and test_hip_coal_skip.py.
"""
import functools

import numpy as np
import pytest

import _harness as h
import bench
from libcloudphxx_amd import lgrngn
from test_hip_coal_cells import CRAFTED, FORCED, LIST_SMALL, NO_LIST, crafted_cells
from test_hip_coal_rank_exit import BOXES, fields
from test_hip_coal_skip import ARITH, ARITH_IDS, assert_same_state, state_of

pytestmark = pytest.mark.gpu

NO_FLOOR = int(lgrngn.dbg2.NO_COAL_CMAX_FLOOR)
HIGH = int(lgrngn.dbg2.COAL_CMAX_FLOOR_HIGH)
NO_SKIP = int(lgrngn.dbg.NO_COAL_SKIP)
POISON, FLT_MIN_BITS = 0xFFFFFFFF, 0x00800000


class Run:
    pass


def bits_up(x):
    """float_bits_up: the bits of x > 0 as a float rounded up, never below FLT_MIN's"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    b = f.view(np.uint32).astype(np.uint64) + (f.astype(np.float64) < x)
    return np.maximum(b, FLT_MIN_BITS)


def as_float(word):
    return float(np.array([word], dtype=np.uint32).view(np.float32)[0])


def run(box, n, sd, real_t, strict, steps, flags2, flags=0, prepare=None, still=False, keep=(), change_at=-1, change=None):
    """`steps` full steps of one of BOXES on n^3 cells x sd; prepare(prt, oi) after init, change(prt, oi) between step_sync and step_async of
    step change_at; still: no advection, sedimentation or condensation.  The maxima's words are kept behind the steps (counted from 1) in `keep`."""
    workload, dt, box_prepare = BOXES[box]
    oi = bench.make_opts_init(n, n, n, sd, 40., 1, 1, 44, workload, dt)
    oi.strict_fp, oi.cond_solver = bool(strict), 0
    oi.dbg_flags, oi.dbg_flags2 = flags, flags2
    prt = h.hip_particles(oi, real_t)
    f = lambda a: np.array(a, dtype=real_t, order="C")
    th, rv, rhod, C = fields(n)
    th, rv, rhod, C = f(th), f(rv), f(rhod), {k: f(v) for k, v in C.items()}
    prt.init(th, rv, rhod, **C)
    if prepare:
        prepare(prt, oi)
    elif box_prepare:
        box_prepare(prt, oi)
    opts = lgrngn.opts_t()
    if still:
        opts.adve = opts.sedi = opts.cond = False
    r = Run()
    r.cells, r.skip, r.collided, r.floor, r.cmax, r.lists = [], [], [], [], {}, []
    for step in range(steps):
        prt.step_sync(opts, th, rv, rhod, **C)
        if step == change_at:
            change(prt, oi)
        prt.step_async(opts)
        r.cells.append([int(v) for v in prt.state_u64("raw_coal_cells")])
        r.skip.append(int(prt.state_u64("raw_coal_skip")[0]))
        r.collided.append(int(prt.state_u64("raw_collided")[0]))
        r.floor.append([int(v) for v in prt.state_u64("raw_coal_cmax_floor")])
        r.lists.append(prt.state_u64("raw_coal_kept_list").astype(np.int64))
        if step + 1 in keep:
            r.cmax[step + 1] = prt.state_u64("raw_coal_cmax").astype(np.uint64)
    r.state = state_of(prt, th, rv)
    return r


@functools.lru_cache(maxsize=None)
def both(box, n, sd, real_t, strict, steps, flags2, keep=(), **kw):
    """the floored run and its NO_COAL_CMAX_FLOOR twin, once per case: the bits, the collisions, the launches with a bound, and the invariant"""
    on = run(box, n, sd, real_t, strict, steps, flags2, keep=keep, **kw)
    off = run(box, n, sd, real_t, strict, steps, (flags2 & ~HIGH) | NO_FLOOR, keep=keep, **kw)
    print("floor", on.floor[0], on.floor[-1], "cells", on.cells, "twin's", off.cells, "collided", on.collided)
    assert on.collided == off.collided
    assert_same_state(on.state, off.state)
    assert all(fl == [0, 0] for fl in off.floor), off.floor
    for step in keep:
        assert on.skip[step - 1] >= 1 and off.skip[step - 1] >= 1, (on.skip, off.skip)         # (both passes of that step collected maxima)
        assert_invariant(on.cmax[step], off.cmax[step], on.floor[step - 1], n ** 3)
    on.state = off.state = None
    return on, off


def assert_invariant(cmax_on, cmax_off, floor, n_cell):
    assert len(cmax_on) == len(cmax_off) == 2 * n_cell and len(floor) == 2
    want = np.maximum(cmax_off, np.tile(np.array(floor, dtype=np.uint64), n_cell))
    bad = np.nonzero(cmax_on != want)[0]
    assert len(bad) == 0, (len(bad), bad[:8], cmax_on[bad[:8]], want[bad[:8]], floor)


def has_floor(r):
    return all(fl[0] > FLT_MIN_BITS and fl[1] > FLT_MIN_BITS for fl in r.floor)


@pytest.mark.parametrize("box,n,steps,keep", [("stratocumulus", 16, 20, (1, 5, 20)), ("drizzle", 8, 3, (1,)), ("mixed", 8, 5, (1, 5))],
                         ids=["stratocumulus-16", "drizzle-8", "mixed-8"])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_the_words_are_the_twins_raised_to_the_floor(real_t, strict, box, n, steps, keep):
    """every word of every cell: the floored pass leaves max(the twin's word, the floor's word) -- a droplet above the floor that does not
    offer, a floor that the fill does not write or a pass that reads another floor than the fill shows here.  The twin's bits and collisions.
    In the stratocumulus box kept cells are never fewer than the twin's and at most 6 in a hundred of the cells with a pair."""
    on, off = both(box, n, 64, real_t, strict, steps, 0, keep=keep)
    assert has_floor(on), on.floor
    if box == "stratocumulus":
        assert all(a[1] >= b[1] and a[2] == b[2] for a, b in zip(on.cells, off.cells)), (on.cells, off.cells)
        assert all(c[1] * 100 <= c[2] * 6 and c[2] > n ** 3 * 0.9 for c in on.cells), on.cells
        words = on.cmax[20].reshape(-1, 2)
        print("cells left at the floor after 20 steps:", int(np.sum((words[:, 0] == on.floor[-1][0]) & (words[:, 1] == on.floor[-1][1]))), "of", n ** 3)


@pytest.mark.parametrize("box", ["sparse", "mixed"])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_collisions_with_the_floor_in_the_forced_list_form(real_t, strict, box):
    """the sparse and the mixed box, 16^3 x 64, 10 steps, the list form in every launch: the twin's bits and collided pairs step by step, at
    least 50 of them, and never fewer kept cells than the twin"""
    on, off = both(box, 16, 64, real_t, strict, 10, FORCED, keep=(1, 10))
    assert sum(on.collided) >= 50, on.collided
    assert all(a[1] >= b[1] for a, b in zip(on.cells, off.cells)), (on.cells, off.cells)


@functools.lru_cache(maxsize=None)
def probe_floor(box, n, sd, real_t, strict, flags2, prepare=None):
    """the floor pair that an object of this box computes in its first step"""
    r = run(box, n, sd, real_t, strict, 1, flags2, prepare=prepare, still=True)
    assert has_floor(r), r.floor
    return tuple(r.floor[0])


def below_the_floor(floor):
    """every droplet at the box's largest multiplicity, radii 0.99 R_f and 0.5 R_f in turn"""
    rf2 = as_float(floor[0])

    def prepare(prt, oi):
        n = prt.state_u64("n")
        k = np.arange(len(n))
        rw2 = np.where(k % 2 == 0, 0.99 ** 2 * rf2, 0.25 * rf2)
        prt.set_particles(np.full(len(n), n.max(), dtype=np.uint64), np.full(len(n), 1e-7 ** 3), rw2, prt.get_attr("kappa"), prt.state_real("vt"),
                          prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z"))
    return prepare


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_nothing_is_offered_and_nothing_is_lost(real_t, strict):
    """the coal-stress box at dt = 0.05, 8^3 x 64, nothing moves or condenses, the floor at a bound of 2^-6: every droplet just below the floor
    at the largest multiplicity, so that no droplet offers and every word of the first pass IS the floor -- the bound that the vote and the
    kernels work with comes from the fill alone.  Ten steps: the bits and the collided pairs of the run without any bound (NO_COAL_SKIP),
    which collides at least 50 pairs.  (Maxima cleared to zero instead would bound every pair's probability by 1e-30 and lose them all.)"""
    floor = probe_floor("drizzle", 8, 64, real_t, strict, HIGH)
    prepare = below_the_floor(floor)
    on = run("drizzle", 8, 64, real_t, strict, 10, HIGH, prepare=prepare, still=True, keep=(1,))
    ref = run("drizzle", 8, 64, real_t, strict, 10, 0, flags=NO_SKIP, prepare=prepare, still=True)
    print("floor", floor, "R_f (um)", as_float(floor[0]) ** .5 * 1e6, "collided", ref.collided, "kept cells", on.cells)
    assert sum(ref.collided) >= 50, ref.collided
    assert on.floor[0] == list(floor) and on.skip[0] >= 1
    words = on.cmax[1].reshape(-1, 2)
    assert np.all(words[:, 0] == floor[0]) and np.all(words[:, 1] == floor[1]), words[(words[:, 0] != floor[0]) | (words[:, 1] != floor[1])][:8]
    assert on.collided == ref.collided
    assert_same_state(on.state, ref.state)


def crafted_edges(floor, real_t):
    """CRAFTED droplets per cell, every one at 0.5 R_f but for: cell 0 (64) holds one droplet one float ulp above R_f^2; cell 2 (1) holds R_f^2
    exactly; cell 3 (2) a living droplet with rw2 = 0; the droplets at storage slots 0 and 1 -- one pair of neighbours for the pass, in two
    cells -- are 10 um and 12 um; slots 20 and 21 are moved into one cell (7) and are 8 um and 9 um"""
    rf2 = np.float32(as_float(floor[0]))

    def prepare(prt, oi):
        assert sum(CRAFTED) == 945 == len(prt.state_u64("n"))
        cell = np.repeat(np.arange(27), CRAFTED)[np.random.default_rng(7).permutation(945)]
        a, b = cell[20], cell[21]                           # (swap so that slots 20 and 21 lie in cell 7; the cells' sizes stay)
        for slot, was in ((20, a), (21, b)):
            other = np.nonzero((cell == 7) & (np.arange(945) > 21))[0][slot - 20]
            cell[slot], cell[other] = 7, was
        assert cell[0] != cell[1] and cell[0] not in (0, 2, 3, 7) and cell[1] not in (0, 2, 3, 7)
        assert np.array_equal(np.bincount(cell, minlength=27), CRAFTED)
        rw2 = np.full(945, 0.25 * float(rf2))
        rw2[np.nonzero(cell == 0)[0][5]] = float(np.nextafter(rf2, np.float32(np.inf)))
        rw2[np.nonzero(cell == 2)[0][0]] = float(rf2)
        rw2[np.nonzero(cell == 3)[0][1]] = 0.
        rw2[0], rw2[1], rw2[20], rw2[21] = 10e-6 ** 2, 12e-6 ** 2, 8e-6 ** 2, 9e-6 ** 2
        x, y, z = (cell // 9 + .5) * oi.dx, (cell // 3 % 3 + .5) * oi.dy, (cell % 3 + .5) * oi.dz
        prt.set_particles(np.full(945, 10 ** 14, dtype=np.uint64), np.full(945, 1e-7 ** 3), rw2, prt.get_attr("kappa"), prt.state_real("vt"), x, y, z)
        assert np.array_equal(np.diff(prt.state_u64("cell_start").astype(np.int64)), CRAFTED)
        prepare.cell, prepare.rw2 = cell, np.array(rw2, dtype=real_t).astype(np.float64)
    return prepare


def all_at_1e14(prt, oi):
    prt.set_particles(np.full(945, 10 ** 14, dtype=np.uint64), prt.get_attr("rd3"), prt.get_attr("rw2"), prt.get_attr("kappa"), prt.state_real("vt"),
                      prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z"))


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_edges_of_the_compare_on_the_crafted_box(real_t, strict):
    """3 x 3 x 3 cells of CRAFTED droplets, nothing moves, one step.  The radius words of all 27 cells against numpy: the largest
    float_bits_up(rw2) of the cell's droplets or the floor's word, whichever is larger; all ones in both words where a living droplet has
    rw2 = 0.  So: one ulp above R_f^2 carries the droplet's bits (the floor's word + 1), R_f^2 exactly carries the floor, an empty cell and a
    cell of small droplets carry the floor, two neighbours in storage that lie in two cells are each right in their own cell, and two in one
    cell leave the larger.  And the invariant against the twin in both words."""
    floor = probe_floor("sparse", 3, 35, real_t, strict, 0, prepare=all_at_1e14)
    prepare = crafted_edges(floor, real_t)
    on = run("sparse", 3, 35, real_t, strict, 1, FORCED, prepare=prepare, still=True, keep=(1,))
    off = run("sparse", 3, 35, real_t, strict, 1, FORCED | NO_FLOOR, prepare=prepare, still=True, keep=(1,))
    assert on.floor[0] == list(floor) and on.skip[0] >= 1 and off.skip[0] >= 1
    assert_invariant(on.cmax[1], off.cmax[1], floor, 27)
    assert on.collided == off.collided
    assert_same_state(on.state, off.state)
    words = on.cmax[1].reshape(-1, 2)
    want = np.full(27, floor[0], dtype=np.uint64)
    np.maximum.at(want, prepare.cell, np.where(prepare.rw2 > 0, bits_up(np.where(prepare.rw2 > 0, prepare.rw2, 1.)), np.uint64(POISON)))
    assert np.array_equal(words[:, 0], want), (words[:, 0], want)
    assert words[0, 0] == floor[0] + 1 and words[2, 0] == floor[0] and tuple(words[1]) == tuple(floor) and tuple(words[3]) == (POISON, POISON), words[:4]
    assert words[7, 0] == bits_up(9e-6 ** 2 if real_t is np.float64 else float(np.float32(9e-6 ** 2)))
    assert np.all(words[(want == floor[0]), 1] == floor[1])                # (a cell without a radius above the floor has no velocity above it either)


def times_512(prt, oi):
    prt.set_particles(prt.state_u64("n") * np.uint64(512), prt.get_attr("rd3"), prt.get_attr("rw2"), prt.get_attr("kappa"), prt.state_real("vt"),
                      prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z"))


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_the_floor_follows_the_largest_multiplicity(real_t, strict):
    """stratocumulus, 8^3 x 64: between step_sync and step_async of the third step set_particles multiplies every multiplicity by 512.  The
    largest multiplicity is recomputed and the floor with it: both words shrink, the invariant holds with the old floor in the step before
    and with the new one in that step, the twin's bits after five."""
    on, _ = both("stratocumulus", 8, 64, real_t, strict, 5, 0, keep=(2, 3), change_at=2, change=times_512)
    assert has_floor(on) and on.floor[0] == on.floor[1] and on.floor[2] == on.floor[4], on.floor
    assert on.floor[2][0] < on.floor[1][0] and on.floor[2][1] < on.floor[1][1], on.floor


@pytest.mark.parametrize("box,n,sd,steps,flags2,prepare,still", [("drizzle", 16, 64, 4, FORCED, None, False), ("drizzle", 16, 64, 4, FORCED | LIST_SMALL, None, False),
                                                                ("sparse", 3, 35, 3, FORCED, crafted_cells, True)],
                         ids=["drizzle-16", "drizzle-16-one-workgroup", "crafted-27"])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_the_sub_lists_hold_every_kept_cell_once(real_t, strict, box, n, sd, steps, flags2, prepare, still):
    """the vote's list in 64 sub-lists with a cursor each ("raw_coal_kept_list": the sub-lists one behind the other), the list form in every
    launch: in every step the list holds no cell twice, only cells of the box, and as many as "raw_coal_cells" counts kept; the bits and the
    collided pairs are those of the NO_COAL_CELL_LIST twin, which makes no list.  The drizzle box keeps every one of its 4 096 cells (64 waves of
    the vote, one per sub-list), once more with k_coal_cells on one workgroup; the crafted 27 cells are one wave of the vote, one sub-list."""
    on = run(box, n, sd, real_t, strict, steps, flags2, prepare=prepare, still=still)
    off = run(box, n, sd, real_t, strict, steps, (flags2 & ~(LIST_SMALL | int(lgrngn.dbg2.COAL_CELL_LIST_ALWAYS))) | NO_LIST, prepare=prepare, still=still)
    print("cells", on.cells, "collided", on.collided)
    for c, l in zip(on.cells, on.lists):
        assert c[0] == 1 and len(l) == c[1] > 0, (c, len(l))
        assert len(np.unique(l)) == len(l) and l.min() >= 0 and l.max() < n ** 3
    assert all(len(l) == 0 for l in off.lists)
    assert on.collided == off.collided and sum(on.collided) >= 50, (on.collided, off.collided)
    assert_same_state(on.state, off.state)
