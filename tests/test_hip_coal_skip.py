"""The coalescence kernel that leaves a pair before gathering its attributes when a per-cell bound rules the collision out.

Since round 8 k_coal_ranked compares a pair's random number u with an upper bound on the pair's collision probability, made of what the
all-droplets velocity pass just ahead has left per cell (the largest wet radius and velocity), the largest multiplicity in storage and the
largest tabulated efficiency those radii can reach.  `bound < 1 and u >= bound` means the pair cannot collide: the full path would have
found col_no = 0 and written nothing.  So a run with the skip and a run with dbg_flags & NO_COAL_SKIP are the same run: every comparison
here is np.array_equal, on every attribute and on the caller's th and rv, in f64 and f32, fast and strict arithmetic.

Whether the skip ran is read back from the object, never assumed: "raw_coal_skip" is the number of coalescence launches of the last
step_async that used a bound and, with dbg_flags2 & COAL_SKIP_COUNT, the pairs skipped and the pairs examined; "raw_collided" counts the
pairs that did collide.
"""
import numpy as np
import pytest

import _harness as h  # noqa: F401  (pins the parity mode of every opts_init_t, as in every test module)
import bench
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

NO_COAL_SKIP = int(lgrngn.dbg.NO_COAL_SKIP)
COUNT = int(lgrngn.dbg2.COAL_SKIP_COUNT)
N, SD = 16, 64
ARITH = [(np.float64, False), (np.float64, True), (np.float32, False), (np.float32, True)]
ARITH_IDS = ["f64-fast", "f64-strict", "f32-fast", "f32-strict"]
_fields = {}


def fields():
    """bench.py's fields on the 16^3 box, made once (every run copies them: step_sync writes th and rv in place)"""
    if not _fields:
        th, rv, rhod, Cx, Cy, Cz = bench.make_fields(N, N, N, 0, N, np, np.float64)
        _fields["f"] = (th, rv, rhod, {"Cx": Cx, "Cy": Cy, "Cz": Cz})
    return _fields["f"]


def box(workload, strict, dt=1., **kw):
    """bench.make_opts_init's box: "stratocumulus" (the headline: hall_pinsky_stratocumulus, almost nothing collides) or "coal-stress" (drizzle)"""
    oi = bench.make_opts_init(N, N, N, SD, 40., 1, 1, 44, workload, dt)
    oi.strict_fp, oi.cond_solver = bool(strict), 0
    for k, v in kw.items():
        assert hasattr(oi, k), k
        setattr(oi, k, v)
    return oi


def state_of(prt, th, rv):
    return {"n": prt.state_u64("n"), "rw2": prt.get_attr("rw2"), "rd3": prt.get_attr("rd3"), "vt": prt.state_real("vt"),
            "kappa": prt.get_attr("kappa"), "x": prt.get_attr("x"), "y": prt.get_attr("y"), "z": prt.get_attr("z"), "ijk": prt.state_u64("ijk"),
            "th": np.array(th, dtype=np.float64), "rv": np.array(rv, dtype=np.float64)}


def assert_same_state(a, b):
    """np.array_equal on the arrays' BITS: stricter than on their values (it tells -0 from 0), and a NaN equals itself -- the f32 strict
    drizzle box carries NaN in some forty cells from its second step on, with or without the skip, in any two runs of it"""
    for name in a:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape, name
        bits = "u%d" % x.dtype.itemsize
        assert np.array_equal(x.view(bits), y.view(bits)), name


class Run:
    pass


def run(oi, skip, real_t, steps, opts=None, prepare=None, between=None, stages=None, after=None, count=True):
    """`steps` full steps (or, stages: that list of single-stage entry points per step).  Returns the final state and, per step, the launches
    that used a bound, the skipped and the examined pairs (count: the counting bit is on), the collided pairs and the droplets in storage.
    prepare(prt): after init; between(prt, step): between step_sync and step_async; after(prt, step): behind step_async and the read-backs"""
    oi.dbg_flags = 0 if skip else NO_COAL_SKIP
    oi.dbg_flags2 = COUNT if count else 0
    prt = h.hip_particles(oi, real_t)
    f = lambda a: np.array(a, dtype=real_t, order="C")
    th, rv, rhod, C = fields()
    th, rv, rhod, C = f(th), f(rv), f(rhod), {k: f(v) for k, v in C.items()}
    prt.init(th, rv, rhod, **C)
    if prepare:
        prepare(prt)
    opts = opts or lgrngn.opts_t()
    r = Run()
    r.launches, r.skipped, r.examined, r.collided, r.n_part = [], [], [], [], []
    for step in range(steps):
        if stages:
            for s in stages:
                prt.stage(s, opts)
        else:
            prt.step_sync(opts, th, rv, rhod, **C)
            if between:
                between(prt, step)
            prt.step_async(opts)
        v = prt.state_u64("raw_coal_skip")
        assert len(v) == (3 if count else 1)
        r.launches.append(int(v[0])); r.skipped.append(int(v[1]) if count else 0); r.examined.append(int(v[2]) if count else 0)
        r.collided.append(int(prt.state_u64("raw_collided")[0]))
        r.n_part.append(len(prt.state_u64("raw_n")))
        if after:
            after(prt, step)
    assert bool(prt.mode()[3] & NO_COAL_SKIP) == (not skip)
    assert prt.mode()[0] == bool(oi.strict_fp)
    r.unused = int(prt.state_u64("raw_coal_bound_unused")[0])
    r.state = state_of(prt, th, rv)
    return r


def both(make_oi, real_t, steps, **kw):
    on, off = run(make_oi(), True, real_t, steps, **kw), run(make_oi(), False, real_t, steps, **kw)
    print("launches", on.launches, "skipped", on.skipped, "examined", on.examined, "collided", on.collided)
    assert off.launches == [0] * steps and off.skipped == [0] * steps
    assert on.collided == off.collided
    assert_same_state(on.state, off.state)
    return on


def shares(r):
    return [s / max(e, 1) for s, e in zip(r.skipped, r.examined)]


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_nothing_collides_and_almost_every_pair_is_skipped(real_t, strict):
    """bench.py's stratocumulus box, 20 steps: the same bits, one launch with a bound per step, at least nine pairs in ten left unread in
    every step (the bound's restatement in numpy on the oracle's droplets: above 0.999 through 200 steps)"""
    on = both(lambda: box("stratocumulus", strict), real_t, 20)
    assert on.launches == [1] * 20
    assert min(on.examined) > N * N * N * SD // 2 * 0.9
    assert min(shares(on)) >= 0.9, shares(on)
    assert on.unused == 0                                  # (no velocity pass collected maxima that its step did not use)


@pytest.mark.parametrize("workload,dt,steps", [("stratocumulus", 1., 20), ("coal-stress", 0.02, 10)])
def test_the_production_form_without_the_counting_bit_gives_the_same_bits(workload, dt, steps):
    """the boxes of the test above and below with dbg_flags2 = 0 -- the kernel as production runs it, no ballots and no counters in it --
    against the NO_COAL_SKIP twin: the same bits, a launch with a bound in every step"""
    on = both(lambda: box(workload, False, dt), np.float64, steps, count=False)
    assert on.launches == [1] * steps
    if workload == "coal-stress":
        assert min(on.collided) >= 10, on.collided


@pytest.mark.parametrize("dt", [0.02, 0.045])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_collisions_and_skips_in_one_launch(real_t, strict, dt):
    """the coal-stress spectrum, 10 steps at a time step that puts the bound below 1 in every cell (0.02: median 0.34) or across 1 (0.045:
    median 0.77, 99 % quantile 1.3 from the fifth step on): droplets collide AND pairs are skipped in every launch, and the bits are the
    same.  The second time step was to be 0.1; tools/coal_skip_gate.py on the oracle's droplets puts every cell's bound above 1 there in the
    first step (1 % quantile 1.37) and 15 % of the cells below 1 later, 0 to 6 % of the pairs skipped -- short of the 0.1 this test wants, so
    that it cannot pass without skipping.  0.045 is chosen from the same quantiles (the bound is proportional to dt): 1 % 0.62, median
    0.80, 99 % 1.03 in the first step.
    Mutations run on the device: with the efficiency bound divided by eight the four dt = 0.02 cases fail on `n`.  With it HALVED every
    case passes, and no test of equal bits can do otherwise: the geometric part of the bound alone, 4 rw2_max vt_max against
    |vta - vtb| (ra + rb)^2, is more than twice what any pair of radii reaches (EXPERIMENTS.md 7.7), so no probability lies between
    half the bound and the bound."""
    on = both(lambda: box("coal-stress", strict, dt), real_t, 10)
    assert on.launches == [1] * 10
    assert all(0.1 <= s <= 0.95 for s in shares(on)), shares(on)
    assert min(on.collided) >= 10, on.collided


@pytest.mark.parametrize("factor", [8, 512])
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_a_multiplicity_bound_from_before_set_particles_is_not_used(real_t, strict, factor):
    """two steps with the skip in use, so that the object holds the largest multiplicity of init; then set_particles installs `factor` x that
    maximum in every seventh droplet of the drizzle box, and five more steps: the maximum is recomputed.  Factor 8 is the case the design
    names; it cannot tell a cached maximum from a fresh one, because the bound lies 6 x and more above the largest pair probability of this
    box (with lcx_core.hip's mark in set_particles taken out it still passed).  Factor 512 can: with the cached maximum the bound stays at
    0.3 while those droplets' pairs reach probabilities above 1, and `n` differs from the NO_COAL_SKIP twin's.  With the fresh maximum
    nothing is skipped any more at 512, and the object stops collecting maxima (see the pause test below)."""
    def raise_n(prt, step):
        if step != 1:
            return
        n = prt.state_u64("n")
        n[::7] = factor * n.max()
        prt.set_particles(n, prt.get_attr("rd3"), prt.get_attr("rw2"), prt.get_attr("kappa"), prt.state_real("vt"),
                          prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z"))

    on = both(lambda: box("coal-stress", strict, 0.02), real_t, 7, after=raise_n)
    assert on.launches[:3] == [1] * 3
    assert min(on.collided) >= 10, on.collided
    assert min(on.skipped[:2]) > 0
    if factor == 8:
        assert on.launches == [1] * 7 and max(on.skipped[2:]) > 0
    assert min(on.collided[2:]) > 2 * max(on.collided[:2])         # (the raised multiplicities do collide)


@pytest.mark.parametrize("count", [True, False], ids=["counted", "sampled"])
def test_a_box_that_skips_next_to_nothing_stops_collecting_maxima(count):
    """the drizzle box at dt = 1: the bound is above 1 in all but a few cells (0.2 % of the pairs skipped on the oracle's droplets).  The
    first step's launch reports that -- its counters, or without the counting bit a sample of them, polled by the next step_async -- and
    the following steps neither collect maxima nor use a bound; the bits are the NO_COAL_SKIP twin's throughout"""
    on = both(lambda: box("coal-stress", False, 1.), np.float64, 6, count=count)
    assert on.launches == [1, 0, 0, 0, 0, 0]
    assert on.unused == 0
    assert min(on.collided) >= 500, on.collided


def src_opts():
    o = lgrngn.opts_t()
    o.src = True
    o.src_dry_distros = {(1e-10, 0.): (lgrngn.expvolume(30.084e-6, 2 ** 23), 8, 2)}      # (fires in every second step)
    return o


def rcyc_opts():
    o = lgrngn.opts_t()
    o.rcyc = True
    return o


def read_between(prt, step):
    prt.state_u64("n")
    prt.get_attr("rw2")


# name: (box keywords, opts, between, stages, launches with a bound per step).  The source, recycling and the read leave the first substep's
# launch its bound -- the velocity pass of the same step_async comes behind them -- and must leave the bits alone
WINDOW = {
    "three_substeps": (dict(sstp_coal=3), None, None, None, 1),
    "simple_source": (dict(src_type=lgrngn.src_t.simple, src_x0=80., src_x1=400., src_y0=40., src_y1=360., src_z0=120., src_z1=520.), src_opts, None, None, 1),
    "rcyc": (dict(), rcyc_opts, None, None, 1),
    "read_between": (dict(), None, read_between, None, 1),
    "khvorostyanov": (dict(terminal_velocity=lgrngn.vt_t.khvorostyanov_spherical), None, None, None, 0),
    "stage_coal": (dict(), None, None, ["hskpng_Tpr", "hskpng_vterm_all", "coal"], 0),
}


@pytest.mark.parametrize("case", list(WINDOW))
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_the_window_closes(real_t, strict, case):
    """where the bound of the velocity pass does not hold for a launch, the launch does not use it -- later substeps, a step with a source,
    recycling, a read of the state between the two halves of a step, a velocity formula whose pass leaves no maxima, a single stage -- and
    every one of these runs ends in the bits of its NO_COAL_SKIP twin"""
    kw, make_opts, between, stages, launches = WINDOW[case]
    steps = 4
    on = both(lambda: box("coal-stress", strict, 0.045, **kw), real_t, steps, opts=make_opts() if make_opts else None, between=between, stages=stages)
    assert on.launches == [launches] * steps
    assert sum(on.collided) >= 10, on.collided
    if case == "simple_source":                            # (it fires in the first and the third step: 8 droplets in each of 8 x 8 x 10 cells)
        assert on.n_part[0] >= N * N * N * SD + 5120 - 200 and on.n_part[2] >= on.n_part[1] + 5120 - 200, on.n_part
        assert on.n_part[1] <= on.n_part[0]


@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_cells_that_the_velocity_pass_cannot_evaluate_are_not_skipped(real_t, strict):
    """a few living droplets with rw2 = 0 (the pass writes no velocity for them): their cells carry no bound, the rest is skipped as before"""
    def zero_rw2(prt):
        rw2 = prt.get_attr("rw2")
        rw2[100::5003] = 0.
        prt.set_particles(prt.state_u64("n"), prt.get_attr("rd3"), rw2, prt.get_attr("kappa"), prt.state_real("vt"),
                          prt.get_attr("x"), prt.get_attr("y"), prt.get_attr("z"))

    opts = lgrngn.opts_t()
    opts.cond = False                                      # (condensation would give the droplets a radius again)
    on = both(lambda: box("coal-stress", strict, 0.02), real_t, 3, opts=opts, prepare=zero_rw2)
    plain = run(box("coal-stress", strict, 0.02), True, real_t, 1, opts=opts)
    # (without condensation a fast-arithmetic step has no kernel that carries the re-sort, and only the first coalescence ranks for itself)
    assert on.launches[0] == 1
    assert 0 < on.skipped[0] < plain.skipped[0]            # (fewer pairs skipped than without the unevaluated droplets)
    assert sum(on.collided) >= 10
