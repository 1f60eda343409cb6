"""The coalescence kernel whose workgroups leave ahead of the ranking when the bound rules out every pair of theirs.

Since round 9 k_coal_ranked<.., SKIP, EXIT> runs the bound's test (tests/test_hip_coal_skip.py) before it loads any id of its window: the
test takes a pair's position, its cell and the cell's numbers, no id.  The workgroup votes; where no lane keeps a pair nobody would read the
ranked order, and the workgroup returns.  The others rank as before.  dbg_flags2 & NO_COAL_RANK_EXIT launches round 8's form, which ranks
in every workgroup: every comparison here is the change against that twin, np.array_equal on the bits of every attribute, of the caller's
th and rv and on the per-step counts of collided pairs, in f64 and f32, fast and strict arithmetic.

What ran is read back from the object: "raw_coal_skip" (launches with a bound, pairs skipped, pairs examined) and "raw_coal_wg" (workgroups
that left before ranking, workgroups launched), both of the last step_async and both with dbg_flags2 & COAL_SKIP_COUNT, and "raw_coal_exit"
(launches of the last step_async in the form with the exit).  A launch in which fewer than 0.24 of the workgroups leave is followed by 32
bound launches in round 8's form (a ranking workgroup pays for the vote); the comparisons set dbg_flags2 & COAL_RANK_EXIT_ALWAYS so that
every step runs the form under test, and the last test looks at the rule itself.

The mixed box (tools/coal_skip_gate.py --workload coal-stress --dt 0.02 --mixed): the drizzle spectrum, and after init every droplet of the
lower half in x shrunk to a hundredth of its wet radius -- a contiguous half of the cell-sorted order that cannot collide next to a half
that does.  On the oracle's droplets everything stays finite, the bound is below 1 in every cell, 0.50 to 0.66 of the 256-position groups
hold a kept pair over ten steps and 8 to 16 pairs collide per step.

The sparse box (the same tool, --workload coal-stress --dt 0.05 --sparse 8:2): those boxes cannot tell a vote that loses lanes from a sound
one -- where pairs collide a workgroup holds ninety kept pairs, and where it holds one, nothing collides (in the natural spectrum a kept
pair collides once in two thousand times).  Here every multiplicity is 2.5e9, the droplets of every eighth cell -- one cell per workgroup,
starting at lane 0 of the workgroup's second wave -- are 100 um and 50 um drops in turn and the rest is shrunk as above: a kept pair
collides once in six times.  On the oracle's droplets: finite, the bound at 0.045 to 0.06 in those cells, 0.77 / 0.90 / 0.93 / 0.92 of the
512-position groups hold a kept pair at steps 1 / 2 / 5 / 10 (the drops drift into neighbouring cells), 1.8 / 2.8 / 3.0 / 3.3 kept pairs
in such a group, and 31 / 33 / 15 / 25 pairs collide.  Run on the device with the vote mutated (EXPERIMENTS.md 7.10): lane 0 of every wave
left out, and the vote taken from the first wave only -- both fail this box on `n`.
"""
import functools

import numpy as np
import pytest

import _harness as h
import bench
from libcloudphxx_amd import lgrngn
from test_hip_coal_skip import ARITH, ARITH_IDS, COUNT, assert_same_state, state_of

pytestmark = pytest.mark.gpu

NO_EXIT = int(lgrngn.dbg2.NO_COAL_RANK_EXIT)
ALWAYS = int(lgrngn.dbg2.COAL_RANK_EXIT_ALWAYS)
WG = 512                                                   # positions of the cell-sorted order per workgroup (COAL_RANKED_POS)


@functools.lru_cache(maxsize=None)
def fields(n):
    """bench.py's fields on the n^3 box, made once per size (every run copies them: step_sync writes th and rv in place)"""
    th, rv, rhod, Cx, Cy, Cz = bench.make_fields(n, n, n, 0, n, np, np.float64)
    return th, rv, rhod, {"Cx": Cx, "Cy": Cy, "Cz": Cz}


def shrink_lower_half(prt, oi):
    """the mixed box: rw2 x 1e-4 and rd3 x 1e-6 for every droplet with x < x1 / 2"""
    x = prt.get_attr("x")
    low = x < 0.5 * oi.x1
    assert 0.3 < low.mean() < 0.7
    rw2, rd3 = prt.get_attr("rw2"), prt.get_attr("rd3")
    rw2[low] *= 1e-4
    rd3[low] *= 1e-6
    prt.set_particles(prt.state_u64("n"), rd3, rw2, prt.get_attr("kappa"), prt.state_real("vt"), x, prt.get_attr("y"), prt.get_attr("z"))


def sparse_drops(prt, oi):
    """the sparse box: every multiplicity 2.5e9; cells with index % 8 == 2 hold 100 um and 50 um drops in turn, the rest shrunk as in the mixed box"""
    x, y, z = prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z")
    cell = ((x // oi.dx).astype(np.int64) * oi.ny + (y // oi.dy).astype(np.int64)) * oi.nz + (z // oi.dz).astype(np.int64)
    assert np.array_equal(cell, prt.state_u64("ijk").astype(np.int64))
    big = np.nonzero(cell % 8 == 2)[0]
    assert len(big) == oi.nx * oi.ny * oi.nz // 8 * oi.sd_conc
    rw2, rd3 = prt.get_attr("rw2") * 1e-4, prt.get_attr("rd3") * 1e-6
    rw2[big[0::2]], rw2[big[1::2]], rd3[big] = 100e-6 ** 2, 50e-6 ** 2, 1e-6 ** 3
    prt.set_particles(np.full(len(x), 25 * 10 ** 8, dtype=np.uint64), rd3, rw2, prt.get_attr("kappa"), prt.state_real("vt"), x, y, z)


# name: (workload, dt, prepare).  "drizzle": test_hip_coal_skip.py's second time step, a kept pair in every workgroup
BOXES = {"stratocumulus": ("stratocumulus", 1., None), "mixed": ("coal-stress", 0.02, shrink_lower_half), "drizzle": ("coal-stress", 0.045, None),
         "sparse": ("coal-stress", 0.05, sparse_drops)}


class Run:
    pass


def run(box, n, sd, real_t, strict, steps, exits, count=True, always=True):
    workload, dt, prepare = BOXES[box]
    oi = bench.make_opts_init(n, n, n, sd, 40., 1, 1, 44, workload, dt)
    oi.strict_fp, oi.cond_solver = bool(strict), 0
    oi.dbg_flags = 0
    oi.dbg_flags2 = (COUNT if count else 0) | (0 if exits else NO_EXIT) | (ALWAYS if exits and always else 0)
    prt = h.hip_particles(oi, real_t)
    f = lambda a: np.array(a, dtype=real_t, order="C")
    th, rv, rhod, C = fields(n)
    th, rv, rhod, C = f(th), f(rv), f(rhod), {k: f(v) for k, v in C.items()}
    prt.init(th, rv, rhod, **C)
    if prepare:
        prepare(prt, oi)
    opts = lgrngn.opts_t()
    r = Run()
    r.launches, r.skipped, r.examined, r.left, r.launched, r.collided, r.exit_form = [], [], [], [], [], [], []
    for step in range(steps):
        prt.step_sync(opts, th, rv, rhod, **C)
        prt.step_async(opts)
        v, w = prt.state_u64("raw_coal_skip"), prt.state_u64("raw_coal_wg")
        assert len(v) == (3 if count else 1) and len(w) == 2
        r.launches.append(int(v[0])); r.skipped.append(int(v[1]) if count else 0); r.examined.append(int(v[2]) if count else 0)
        r.left.append(int(w[0])); r.launched.append(int(w[1]))
        r.exit_form.append(int(prt.state_u64("raw_coal_exit")[0]))
        r.collided.append(int(prt.state_u64("raw_collided")[0]))
    assert prt.mode()[0] == bool(strict) and prt.mode()[3] == 0
    r.n_part = len(prt.state_u64("raw_n"))
    r.state = state_of(prt, th, rv)
    return r


@functools.lru_cache(maxsize=None)
def both(box, n, sd, real_t, strict, steps, count=True, always=True):
    """the change and its twin, run once per case and shared by the tests that read them; the bits, the collisions and the counters compared"""
    on, off = run(box, n, sd, real_t, strict, steps, True, count, always), run(box, n, sd, real_t, strict, steps, False, count)
    print("launches", on.launches, "exit form", on.exit_form, "left", on.left, "of", on.launched, "skipped", on.skipped, "examined", on.examined,
          "collided", on.collided)
    assert on.launches == off.launches == [1] * steps                      # (a launch with a bound in every step, in both)
    assert off.exit_form == [0] * steps and (not always or on.exit_form == [1] * steps)
    assert on.collided == off.collided
    assert_same_state(on.state, off.state)
    assert off.left == [0] * steps
    if count:
        assert on.launched == off.launched and min(on.launched) >= (on.n_part + WG - 1) // WG
    else:                                                                  # (no counters without the bit, in either form)
        assert on.left == on.launched == off.launched == [0] * steps
    on.state = off.state = None                                            # (compared; the counters are what the tests go on reading)
    return on, off


def left_shares(r):
    return [a / max(b, 1) for a, b in zip(r.left, r.launched)]


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_almost_every_workgroup_leaves(real_t, strict):
    """bench.py's stratocumulus box, 16^3 x 64, 20 steps: the same bits, one launch with a bound per step, at least 0.8 of the workgroups
    leave before ranking in every step (0.94 to 0.99 on the oracle's droplets) and every pair is still examined"""
    on, _ = both("stratocumulus", 16, 64, real_t, strict, 20)
    assert min(left_shares(on)) >= 0.8, left_shares(on)
    assert min(on.examined) > 16 ** 3 * 64 // 2 * 0.9


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_exits_and_collisions_in_one_launch(real_t, strict):
    """the mixed box, 16^3 x 64, 10 steps: the same bits, between 0.2 and 0.6 of the workgroups leave in every step, pairs collide"""
    on, _ = both("mixed", 16, 64, real_t, strict, 10)
    assert all(0.2 <= s <= 0.6 for s in left_shares(on)), left_shares(on)
    assert sum(on.collided) >= 50, on.collided


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_one_or_two_kept_pairs_in_a_workgroup_and_they_collide(real_t, strict):
    """the sparse box, 16^3 x 64, 5 steps: the same bits -- a vote that loses a lane or a wave loses collisions here.  In the first step
    every workgroup has its kept pairs in the one cell of drops (0.23 of the workgroups keep none on the oracle's droplets and leave);
    at least 50 pairs collide over the five steps (the oracle: about 120)"""
    on, _ = both("sparse", 16, 64, real_t, strict, 5)
    assert 0.1 <= left_shares(on)[0] <= 0.4, left_shares(on)
    assert min(on.left) > 0
    assert sum(on.collided) >= 50 and on.collided[0] >= 10, on.collided


@pytest.mark.parametrize("n,sd", [(2, 48), (3, 64)], ids=["one-partial-workgroup", "three-and-a-partial"])
@pytest.mark.parametrize("box", ["stratocumulus", "mixed", "drizzle"])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_edges_of_the_grid(real_t, strict, box, n, sd):
    """2 x 2 x 2 cells x 48 (384 droplets: one partial workgroup, whose window ends before P0 + 512) and 3 x 3 x 3 x 64 (1728: three workgroups
    and a partial fourth, cells straddling their borders), 5 steps of either box: the same bits"""
    on, _ = both(box, n, sd, real_t, strict, 5)
    assert max(on.launched) <= n ** 3 * sd // WG + 1


@pytest.mark.parametrize("box,steps", [("stratocumulus", 20), ("mixed", 10)])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_counters_agree(real_t, strict, box, steps):
    """with and without the exit the pairs skipped and the pairs examined are equal step by step (the runs of the first two tests)"""
    on, off = both(box, 16, 64, real_t, strict, steps)
    assert on.skipped == off.skipped and on.examined == off.examined
    assert min(on.examined) > 0


@pytest.mark.parametrize("box,steps", [("stratocumulus", 20), ("mixed", 10)])
def test_the_production_form_without_the_counting_bit_gives_the_same_bits(box, steps):
    """dbg_flags2 = 0 -- the kernel as production runs it, its sample fed by every 64th workgroup, the form of each launch chosen by the
    object -- against its twin; the stratocumulus box stays in the form with the exit"""
    on, _ = both(box, 16, 64, np.float64, False, steps, count=False, always=False)
    if box == "stratocumulus":
        assert on.exit_form == [1] * steps
    if box == "mixed":
        assert sum(on.collided) >= 50, on.collided


@pytest.mark.parametrize("count", [True, False], ids=["counted", "sampled"])
def test_a_box_in_which_no_workgroup_leaves_goes_back_to_ranking_everywhere(count):
    """the drizzle box at dt = 0.045: a bound in every step and a kept pair in every workgroup.  The first launch reports that -- its
    counters, or a sample of them, polled by the next step_async -- and the following launches take round 8's form; the same bits"""
    on, _ = both("drizzle", 16, 64, np.float64, False, 6, count=count, always=False)
    assert on.exit_form == [1, 0, 0, 0, 0, 0]
    assert sum(on.collided) >= 50, on.collided
    if count:
        assert on.left == [0] * 6 and min(on.launched) >= 512
