"""Collision rates per cell (include/lcx_coal_rates.h) on the device, in double and float.

1. Event by event: a 2-D box whose state, shuffle keys and random numbers are all given, the generic kernel, against the long-double walk
   of tests/_coal_rates_reference.py.  Every pair is either a free one (prob < 0.5, u = 0: one collision, u = 0.999: none) or a capped one
   (prob > 2 q: the count is q = n_big / n_small), which the walk asserts.  Numbers exact, M3 to (K + 8) eps_double sum |term|.
   Also three substeps per step over several steps, read twice with a reset between.
2. Budget closure on the production path (the tabulated kernel, own random numbers, the kernel that ranks for itself): what the state
   lost and gained per cell between two reads of the raw storage against the accumulators.
3. Nothing else moves: the same runs with the accumulators on and off, bit for bit.
4. The surface: diag_coal_rate against read, device output, every error text, enable before and after init, snapshots, the Onishi kernel.
"""
import numpy as np
import pytest

import _harness as h
import _coal_rates_reference as CR
import _vterm_coal_reference as R
import test_oracle_vterm_coal as V
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

LD = np.longdouble
R_THR = 25e-6
REALS = [np.float64, np.float32]
REAL_IDS = ["f64", "f32"]
# collide()'s bar for the merged rw2, in eps of the real type (tests/test_hip_vterm_coal.py holds it)
COLLIDE_BAR = {np.float64: 29., np.float32: 16.}
OCC = [0, 1, 2, 3, 5, 63, 64, 65, 300, 2, 2, 2, 3, 5, 8, 2]          # super-droplets per cell, nx = nz = 4
# cells whose two droplets are set by hand, one per row of the header's table: (r of the first, r of the second, multiplicity factors)
ROW_CELLS = {2: (10e-6, 12e-6, 3, 1), 9: (22e-6, 23e-6, 2, 1), 10: (10e-6, 40e-6, 3, 1), 11: (40e-6, 10e-6, 3, 1), 15: (30e-6, 60e-6, 1, 1)}
CAPPED = {3, 4, 10, 11, 12, 13, 14, 15}                               # cells in the capped regime (the large ones are free)


def lo_of(real_t):
    return real_t(np.float64(R_THR) ** 2)                             # (lcx::diag::rng_bounds: std::pow(r, 2) in double, then the object's type)


def box2d(real_t, **kw):
    oi = h.box_opts(4, 0, 4, 2, dx=1., dt=1., n_sd_max=sum(OCC) + 16, sedi_switch=False, kernel=lgrngn.kernel_t.geometric,
                    terminal_velocity=lgrngn.vt_t.beard76, **kw)
    th, rv, rhod, C = h.box_fields(oi)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    return oi, (f(th), f(rv), f(rhod), {k: f(v) for k, v in C.items()})


def design(real_t, all_free=False, seed=5):
    """the state of test 1: radii log-uniform 5 ... 80 um (clear of the threshold), velocities of beard76 in long double, and per cell
    multiplicities that put every possible pair of the cell into one regime: free cells n0 ... 2 n0 with prob <= 0.1 for the cell's
    worst pair, capped cells k * scale (k = 1, 2, 3) with n_small * prob_1 >= 8 for the cell's weakest pair"""
    oi, fields = box2d(real_t)
    th, rv, rhod, _ = fields
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.arange(16), OCC)
    N = cells.size
    capped = set() if all_free else CAPPED
    dv, dt = LD(1), LD(1)

    def draw(c, m):
        while True:
            r = np.exp(rng.uniform(np.log(5e-6), np.log(80e-6), m))
            if c in ROW_CELLS and not all_free:
                r = np.array(ROW_CELLS[c][:2])
            rw2 = (r.astype(LD) ** 2).astype(real_t)
            if (np.abs(np.sqrt(rw2.astype(np.float64)) / R_THR - 1) < 1e-3).any():
                continue
            cc = np.full(m, c)
            vt = R.vterm("beard76", rw2, th.ravel()[cc], rv.ravel()[cc], rhod.ravel()[cc], real_t).astype(real_t)
            if m < 2:
                return rw2, vt, None
            i, j = np.triu_indices(m, 1)
            one = np.ones(i.size, dtype=np.uint64)
            p1 = R.prob(dt, np.full(i.size, dv), np.full(i.size, m), R.kernel("geometric", real_t, one, one, rw2[i], rw2[j], vt[i], vt[j]))
            if c in capped and (np.abs(vt[i].astype(LD) - vt[j].astype(LD)) < LD(.05) * np.maximum(vt[i], vt[j]).astype(LD)).any():
                continue                                              # (a capped cell's weakest pair must still be a strong one)
            return rw2, vt, p1

    rw2, vt, n = np.empty(N, dtype=real_t), np.empty(N, dtype=real_t), np.ones(N, dtype=np.uint64)
    for c, m in enumerate(OCC):
        sl = slice(int(np.sum(OCC[:c])), int(np.sum(OCC[:c + 1])))
        if m == 0:
            continue
        rw2[sl], vt[sl], p1 = draw(c, m)
        if p1 is None:
            n[sl] = 1000
        elif c in capped:
            scale = int(np.ceil(LD(8) / p1.min()))
            k = np.array(ROW_CELLS[c][2:]) if c in ROW_CELLS else rng.integers(1, 4, m)
            n[sl] = (scale * k).astype(np.uint64)
            assert scale * 3 * m * 3 < 2 ** 52
        else:
            n0 = int(np.floor(LD(.05) / p1.max()))
            assert n0 >= 8, (c, n0)
            n[sl] = rng.integers(n0, 2 * n0 + 1, m).astype(np.uint64)
            if c in ROW_CELLS and not all_free:
                n[sl] = (n0 * np.array(ROW_CELLS[c][2:])).astype(np.uint64)
    rd3 = ((1e-8 * (1 + np.arange(N) / 7.)) ** 3).astype(real_t)
    i, k = cells // 4, cells % 4
    args = dict(n=n, rd3=rd3.astype(np.float64), rw2=rw2.astype(np.float64), kpa=np.full(N, .5), vt=vt.astype(np.float64),
                x=(i + .5) * oi.dx, z=(k + .5) * oi.dz)
    return dict(oi=oi, fields=fields, cells=cells, args=args, state=dict(n=n, rw2=rw2, rd3=rd3, vt=vt))


def coal_only():
    opts = lgrngn.opts_t()
    opts.cond = opts.adve = opts.sedi = False
    opts.coal = True
    return opts


def start(case, real_t, tally="after"):
    """the object with the case's particles in, fields synchronised; tally: "before" / "after" init(), or None"""
    th, rv, rhod, C = case["fields"]
    prt = h.hip_particles(case["oi"], real_t)
    if tally == "before":
        prt.coal_rates_enable(R_THR)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C.items()})
    if tally == "after":
        prt.coal_rates_enable(R_THR)
    prt.set_particles(**case["args"])
    prt.step_sync(coal_only(), th.copy(), rv.copy(), rhod.copy())
    prt.stage("hskpng_Tpr")
    assert np.array_equal(prt.state_u64("ijk"), case["cells"])
    return prt


def picker(rng):
    def pick(p, p_lo, p_hi, q):
        if q is not None and p_lo > 2 * q:
            return rng.random()                                        # capped: any number
        return 0. if (p_lo > 0 and rng.random() < .6) else .999        # free: one collision or none
    return pick


def assert_sums(got, sums, real_t, tag):
    """got: dict name -> ndarray(n_cell) of the device; numbers exact, M3 within the walk's bar"""
    for w, nm in enumerate(CR.NAMES):
        for c in range(sums.n_cell):
            want = sums.value(w, c)
            if w in CR.M3_ROWS:
                bar = CR.m3_bar(sums, w, c, real_t, COLLIDE_BAR[real_t])
                assert abs(LD(got[nm][c]) - want) <= bar, (tag, nm, "cell", c, got[nm][c], float(want), "bar", float(bar))
            else:
                assert want < 2 ** 53 and got[nm][c] == float(want), (tag, nm, "cell", c, got[nm][c], want)


def replayed_stage(real_t, tally):
    """test 1's launch: returns (object, sums of the walk, the walk's state after the launch)"""
    case = design(real_t)
    prt = start(case, real_t, tally)
    rng = np.random.default_rng(11)
    N = case["cells"].size
    keys = rng.permutation(2 ** 20)[:N].astype(np.float64)
    order = CR.cell_sorted_order(case["cells"], keys)
    sums = CR.Sums(16)
    state = {k: v.copy() for k, v in case["state"].items()}
    dv = prt.state_real("dv").astype(LD)
    u01 = CR.walk(sums, real_t, "geometric", state, case["cells"], order, None, case["oi"].dt, dv, lo_of(real_t), pick=picker(rng))
    CR.walk(CR.Sums(16), real_t, "geometric", {k: v.copy() for k, v in case["state"].items()}, case["cells"], order, u01, case["oi"].dt, dv,
            lo_of(real_t))                                             # (the walk again from the numbers pushed: the margins are asserted there)
    prt.rng_replay_push(1, keys)
    prt.rng_replay_push(0, u01)
    prt.stage("coal", coal_only())
    assert int(prt.state_u64("raw_coal_kernel")[0]) == 0
    return prt, sums, state, order


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_every_event_of_a_replayed_launch(real_t):
    prt, sums, state, order = replayed_stage(real_t, "before" if real_t is np.float64 else "after")
    assert np.array_equal(prt.state_u64("raw_sorted_id")[:order.size].astype(np.int64), order), "the order that the walk assumed"
    assert np.array_equal(prt.state_u64("n"), state["n"]), "the walk and the device must have made the same events"
    assert all(v > 0 for v in sums.rows.values()), ("every row of the table must have occurred", sums.rows)
    assert int(np.sum(state["n"] == 0)) > 0, "a donor used up (q = 1 with equal multiplicities)"
    en, r_thr, launches = prt.coal_rates_info()
    assert (en, r_thr, launches) == (True, R_THR, 1)
    got = prt.coal_rates()
    assert_sums(got, sums, real_t, "one launch")
    for c, m in enumerate(OCC):                                        # (cells without a pair)
        if m < 2:
            assert all(got[nm][c] == 0 for nm in CR.NAMES)
    assert_sums(prt.coal_rates(reset=True), sums, real_t, "read again")
    assert all((v == 0).all() for v in prt.coal_rates().values()), "reset zeroes behind the read"
    assert prt.coal_rates_info()[2] == 0


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_three_substeps_over_several_steps_with_a_reset(real_t):
    """sstp_coal = 3 through step_async, every cell free: the walk runs the substeps itself (a grown droplet's velocity from the long-double
    beard76, its radius rounded from long double: the terms it enters later carry collide()'s bar) and draws the random numbers that the
    device is then given.  Two accumulations of two steps each, the first read resets."""
    case = design(real_t, all_free=True, seed=6)
    case["oi"].sstp_coal = 3
    prt = start(case, real_t, "after")
    rng = np.random.default_rng(12)
    opts = coal_only()
    eps_t = float(np.finfo(real_t).eps)
    vt_tol = 2 * V.BARS[real_t]["vt_beard76"] * eps_t
    thc, rvc, rhodc = (prt.state_real(nm) for nm in ("th", "rv", "rhod"))
    dv = prt.state_real("dv").astype(LD)
    launches = 0
    for acc in range(2):
        sums = CR.Sums(16)
        for step in range(2):
            prt.stage("hskpng_vterm_all")
            ijk = prt.state_u64("ijk").astype(np.int64)
            state = dict(n=prt.state_u64("n"), rw2=prt.state_real("rw2").astype(real_t), rd3=prt.state_real("rd3").astype(real_t),
                         vt=prt.state_real("vt").astype(real_t))
            assert (state["n"] > 0).all() and (state["vt"] > 0).all()
            grown = np.zeros(ijk.size, dtype=bool)
            push = []
            for sub in range(3):
                redo = state["vt"] < 0                                  # grown in the last substep: the velocity is computed anew
                if redo.any():
                    cc = ijk[redo]
                    state["vt"][redo] = R.vterm("beard76", state["rw2"][redo], thc[cc], rvc[cc], rhodc[cc], real_t).astype(real_t)

                def rel(a, b):
                    va, vb = LD(state["vt"][a]), LD(state["vt"][b])
                    loose = vt_tol * (float(grown[a]) * va + float(grown[b]) * vb)
                    return 1e-4 + (float(loose / abs(va - vb)) if va != vb else 0.)
                keys = rng.permutation(2 ** 20)[:ijk.size].astype(np.float64)
                order = CR.cell_sorted_order(ijk, keys)
                u01 = CR.walk(sums, real_t, "geometric", state, ijk, order, None, case["oi"].dt / 3, dv, lo_of(real_t), rel=rel, grown=grown,
                              pick=picker(rng))
                push += [(1, keys), (0, u01)]
            for kind, arr in push:
                prt.rng_replay_push(kind, arr)
            prt.step_async(opts)
            launches += 3
            left = lambda n: np.sort(n[n > 0])                       # (the storage may have been put into another order by the step's end)
            assert np.array_equal(left(prt.state_u64("raw_n")), left(state["n"])), "the walk and the device must have made the same events"
            th, rv, rhod, _ = case["fields"]
            prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy())
        assert sum(sums.rows.values()) > 100 and sums.loose_m3.sum() > 0, sums.rows
        assert prt.coal_rates_info()[2] == 6
        assert_sums(prt.coal_rates(reset=True), sums, real_t, "accumulation %d" % acc)


# ---------------------------------------------------------------------------------------------------- 2. the production path
def production_case(real_t, onishi=False, seed=3):
    kern = lgrngn.kernel_t.onishi_hall if onishi else lgrngn.kernel_t.hall
    oi = h.box_opts(4, 4, 4, 64, dx=1., dt=1., kernel=kern, terminal_velocity=lgrngn.vt_t.beard77fast, strict_fp=False, cond_solver=0,
                    turb_coal_switch=onishi)
    if onishi:
        oi.kernel_parameters = np.array([100.])
    th, rv, rhod, C = h.box_fields(oi)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.arange(64), 64)
    N = cells.size
    r = np.exp(rng.uniform(np.log(5e-6), np.log(80e-6), N))
    # prob of a typical pair per unit of multiplicity: 63 (scale factor) pi |dvt| (ra + rb)^2 E ~ 63 * 3.14 * 0.1 * 3.6e-9 * 0.5 = 3.6e-8
    # with dt / dv = 1: multiplicities of 1.2e5 ... 5e5 make 5 % of the pairs collide in a step (the long-double kernel's estimate).  Two
    # cloud droplets make a rain drop only where both are above 25 um / 2^(1/3) = 19.9 um, and Hall's kernel gives such a pair of nearly equal
    # droplets 1e-9 per unit of multiplicity: the droplets of that band carry 400 times the multiplicity (8 % of the droplets; with them 12 % of
    # the pairs collide), or four steps of this box would see no autoconversion at all.
    n = rng.integers(125000, 500000, N).astype(np.uint64)
    n[(r > 19.9e-6) & (r < 25e-6)] *= np.uint64(400)
    i, j, k = cells // 16, (cells // 4) % 4, cells % 4
    args = dict(n=n, rd3=np.full(N, 1e-24), rw2=((r.astype(LD) ** 2).astype(real_t)).astype(np.float64), kpa=np.full(N, .5), vt=np.full(N, .1),
                x=(i + .5) * oi.dx, y=(j + .5) * oi.dy, z=(k + .5) * oi.dz)
    return dict(oi=oi, fields=(f(th), f(rv), f(rhod), {kk: f(v) for kk, v in C.items()}), cells=cells, args=args)


def class_sums(prt, real_t, n_cell):
    """per cell, from the raw storage: N and M3 = sum n r^3 of cloud and of rain (Python integers, long double), droplets per cell"""
    n = prt.state_u64("raw_n")
    rw2 = prt.state_real("raw_rw2").astype(real_t)
    ijk = prt.state_u64("raw_ijk").astype(np.int64)
    live = (n > 0) & (ijk < n_cell)
    rain = rw2 >= lo_of(real_t)
    r3 = rw2.astype(LD) * np.sqrt(rw2.astype(LD))
    out = dict(Nc=[0] * n_cell, Nr=[0] * n_cell, M3c=np.zeros(n_cell, dtype=LD), M3r=np.zeros(n_cell, dtype=LD), cnt=np.zeros(n_cell, dtype=np.int64))
    for idx in np.nonzero(live)[0]:
        c = int(ijk[idx])
        out["cnt"][c] += 1
        if rain[idx]:
            out["Nr"][c] += int(n[idx]); out["M3r"][c] += int(n[idx]) * r3[idx]
        else:
            out["Nc"][c] += int(n[idx]); out["M3c"][c] += int(n[idx]) * r3[idx]
    return out


def assert_closure(before, after, got, real_t, n_cell, tag):
    eps_t = LD(np.finfo(real_t).eps)
    for c in range(n_cell):
        assert after["Nc"][c] - before["Nc"][c] == -int(got["self_cloud_n"][c] + got["acnv_nc"][c] + got["accr_nc"][c]), (tag, "N_cloud", c)
        assert after["Nr"][c] - before["Nr"][c] == int(got["acnv_nr"][c]) - int(got["self_rain_n"][c]), (tag, "N_rain", c)
        bar = (1.5 * COLLIDE_BAR[real_t] + int(before["cnt"][c]) + 8) * eps_t * (before["M3r"][c] + after["M3r"][c])
        d = (after["M3r"][c] - before["M3r"][c]) - (LD(got["acnv_m3"][c]) + LD(got["accr_m3"][c]))
        print("%-24s cell %2d  dM3_rain - (acnv + accr): %9.2e   bar %9.2e" % (tag, c, float(d), float(bar)))
        assert abs(d) <= bar, (tag, "M3_rain", c, float(d), float(bar))
    assert (got["acnv_m3"] > 0).any() and (got["accr_m3"] > 0).any(), tag


def production_run(real_t, tally, steps=4, onishi=False, dbg_flags2=0, forms=None):
    """forms: a list that receives (launches with the bound, launches in the early-exit form) of every step"""
    case = production_case(real_t, onishi)
    case["oi"].dbg_flags2 = dbg_flags2
    th, rv, rhod, C = case["fields"]
    prt = h.hip_particles(case["oi"], real_t)
    kw = {"diss_rate": np.full(th.shape, 1e-2, dtype=real_t)} if onishi else {}
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C.items()})
    prt.set_particles(**case["args"])
    if tally:
        prt.coal_rates_enable(R_THR)
    opts = coal_only()
    opts.turb_coal = onishi
    before, ranked = None, []
    for step in range(steps):
        prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **kw)
        if step == 0:
            before = class_sums(prt, real_t, 64)
        prt.step_async(opts)
        ranked.append(int(prt.state_u64("raw_coal_ranked")[0]))
        assert int(prt.state_u64("raw_coal_kernel")[0]) == (1 if onishi else 2)
        if forms is not None:
            forms.append((int(prt.state_u64("raw_coal_skip")[0]), int(prt.state_u64("raw_coal_exit")[0])))
    return prt, before, ranked


@pytest.mark.parametrize("no_exit", [False, True], ids=["exit", "no-exit"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_budgets_close_on_the_production_path(real_t, no_exit):
    forms = []
    prt, before, ranked = production_run(real_t, True, dbg_flags2=int(lgrngn.dbg2.NO_COAL_RANK_EXIT) if no_exit else 0, forms=forms)
    # the first step's launch ranks for itself behind the probability bound, in the form with the early exit or (the twin) without
    assert forms[0] == (1, 0 if no_exit else 1), forms
    # (every step's launch was the production variant, asserted in production_run.  With nothing moving between the steps only the first one's
    # order is owed to the kernel that ranks for itself; the later ones find it in memory and take k_coal<T, false, true>: both forms are tallied)
    assert ranked[0] > 0 and len(ranked) == 4, ("the production variants must be the tallied ones", ranked)
    assert prt.coal_rates_info()[2] == 4
    after = class_sums(prt, real_t, 64)
    got = prt.coal_rates()
    assert_closure(before, after, got, real_t, 64, "production")
    moved = sum(int(got["acnv_nc"][c] + got["accr_nc"][c] + got["self_cloud_n"][c]) for c in range(64))
    assert 0 < moved < .5 * sum(before["Nc"]), "a few per cent of the pairs collide"


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_budgets_close_with_the_onishi_kernel(real_t):
    prt, before, _ = production_run(real_t, True, steps=1, onishi=True)
    assert int(prt.state_u64("raw_coal_kernel")[0]) == 1
    assert_closure(before, class_sums(prt, real_t, 64), prt.coal_rates(), real_t, 64, "onishi")


# ---------------------------------------------------------------------------------------------------- 3. nothing else moves
def raw_state(prt):
    return {nm: prt.state_u64(nm) if nm == "raw_n" else prt.state_real(nm) for nm in ("raw_n", "raw_rw2", "raw_rd3", "raw_vt")}


def modes(prt):
    return [list(prt.state_u64(nm)) for nm in ("raw_mode", "raw_coal_kernel", "raw_coal_ranked", "raw_coal_skip", "raw_coal_exit")]


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_replayed_launch_moves_nothing_else(real_t):
    on, off = replayed_stage(real_t, "after")[0], replayed_stage(real_t, None)[0]
    a, b = raw_state(on), raw_state(off)
    for nm in a:
        assert np.array_equal(a[nm], b[nm]), nm
    assert np.array_equal(on.state_real("col"), off.state_real("col"))


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_production_run_moves_nothing_else(real_t):
    on, _, ranked_on = production_run(real_t, True)
    off, _, ranked_off = production_run(real_t, False)
    a, b = raw_state(on), raw_state(off)
    for nm in a:
        assert np.array_equal(a[nm], b[nm]), nm
    assert ranked_on == ranked_off
    with pytest.raises(RuntimeError, match="not enabled"):
        off.coal_rates()
    on.coal_rates_disable()
    assert on.coal_rates_info() == (False, 0., 0)
    th, rv, rhod, _ = production_case(real_t)["fields"]
    for prt in (on, off):                                              # one more step each: a disabled object launches what a never-enabled one does
        prt.step_sync(coal_only(), th.copy(), rv.copy(), rhod.copy())
        prt.step_async(coal_only())
    assert modes(on) == modes(off)
    a, b = raw_state(on), raw_state(off)
    for nm in a:
        assert np.array_equal(a[nm], b[nm]), nm


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_random_numbers_are_what_they_were(real_t):
    """lcx_rng_dump needs tagged droplets, which take the production kernel without the in-cell ranking: its own stream, on and off"""
    dumps = []
    for tally in (True, False):
        case = production_case(real_t)
        case["oi"].dbg_flags = int(lgrngn.dbg.TAG)
        th, rv, rhod, C = case["fields"]
        prt = h.hip_particles(case["oi"], real_t)
        prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C.items()})
        prt.set_particles(**case["args"])
        if tally:
            prt.coal_rates_enable(R_THR)
        for step in range(2):
            prt.step_sync(coal_only(), th.copy(), rv.copy(), rhod.copy())
            prt.step_async(coal_only())
        dumps.append([prt.rng_dump(0, which) for which in (0, 1)] + [raw_state(prt)[nm] for nm in ("raw_n", "raw_rw2")])
        if tally:
            assert sum(v.sum() for v in prt.coal_rates().values()) > 0
    for x, y in zip(*dumps):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------- 4. the surface
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_diag_coal_rate_and_device_output(real_t):
    import torch
    prt, _, _ = production_run(real_t, True, steps=2)
    got = prt.coal_rates()
    dv, rhod = prt.state_real("dv").astype(real_t), prt.state_real("rhod").astype(real_t)
    for w, nm in enumerate(CR.NAMES):
        prt.diag_coal_rate(nm if w % 2 else w)
        out = np.frombuffer(prt.outbuf(), dtype=real_t).copy()
        want = (got[nm].astype(real_t) / dv) / rhod                    # (the division in the object's type, by dv and then by rhod)
        assert np.array_equal(out, want), nm
    buf = torch.full((7, 80), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    prt.coal_rates(out=lgrngn.DeviceArray(buf.data_ptr(), (7, 64), (80, 1)))
    host = buf.cpu().numpy()
    assert all(np.array_equal(host[w, :64], got[nm]) for w, nm in enumerate(CR.NAMES))
    assert (host[:, 64:] == -1).all(), "the elements between n_cell and the stride are not written"
    wide = np.full((7, 70), -2.)
    prt.coal_rates(out=wide[:, :64])
    assert all(np.array_equal(wide[w, :64], got[nm]) for w, nm in enumerate(CR.NAMES)) and (wide[:, 64:] == -2).all()


def test_a_parcel_is_not_divided():
    oi = lgrngn.opts_init_t()
    oi.dt, oi.sd_conc, oi.n_sd_max = 1., 64, 64
    oi.dry_distros = {(1e-10, 0.): lgrngn.expvolume(20e-6, 2 ** 30)}
    oi.kernel, oi.terminal_velocity, oi.sedi_switch = lgrngn.kernel_t.geometric, lgrngn.vt_t.beard77fast, False
    prt = h.hip_particles(oi)
    prt.init(np.array([300.]), np.array([.01]), np.array([1.1]))
    prt.coal_rates_enable(R_THR)
    opts = coal_only()
    for _ in range(3):
        prt.step_sync(opts, np.array([300.]), np.array([.01]), np.array([1.1]))
        prt.step_async(opts)
    got = prt.coal_rates()
    assert sum(v.sum() for v in got.values()) > 0
    for nm in CR.NAMES:
        prt.diag_coal_rate(nm)
        assert np.frombuffer(prt.outbuf(), dtype=np.float64)[0] == got[nm][0], nm


def test_every_error_text():
    import ctypes as C
    prt, _, _ = production_run(np.float64, False, steps=1)
    for call in (prt.coal_rates, lambda: prt.diag_coal_rate("accr_m3")):
        with pytest.raises(RuntimeError, match=r"libcloudph\+\+: coal_rates: .* while the accumulators are not enabled"):
            call()
    f = lambda name: getattr(prt._lib, "lcx_" + name)
    last = prt._f("last_error")
    last.restype = C.c_char_p
    for bad in (0., -1e-6, float("nan"), float("inf")):
        assert f("coal_rates_enable")(prt._h, C.c_double(bad)) == 1 and "r_thr must be positive and finite" in last().decode()
    assert prt.coal_rates_info()[0] is False
    prt.coal_rates_enable(R_THR)
    out = np.zeros((7, 64))
    for which in (-1, 7):
        assert f("diag_coal_rate")(prt._h, C.c_int(which)) == 1 and "which = %d is outside 0 .. 6" % which in last().decode()
    assert f("coal_rates_read")(prt._h, C.c_void_p(out.ctypes.data), C.c_size_t(63), C.c_int(0), C.c_int(0)) == 1
    assert "libcloudph++: coal_rates: stride (63) < n_cell (64)" in last().decode()
    assert f("coal_rates_read")(prt._h, None, C.c_size_t(64), C.c_int(0), C.c_int(0)) == 1 and "coal_rates: out == NULL" in last().decode()
    assert f("coal_rates_read")(prt._h, C.c_void_p(out.ctypes.data), C.c_size_t(64), C.c_int(0), C.c_int(0)) == 0


def test_a_multi_device_object_is_refused(monkeypatch):
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = h.box_opts(4, 4, 4, 16)
    oi.dev_count = 2
    prt = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert prt.dev_count == 2
    for call in (lambda: prt.coal_rates_enable(R_THR), prt.coal_rates_disable, prt.coal_rates_info, prt.coal_rates, lambda: prt.diag_coal_rate(0)):
        with pytest.raises(RuntimeError, match=r"libcloudph\+\+: coal_rates on a multi-device object is not built"):
            call()


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_a_snapshot_drops_the_accumulators_and_the_run_goes_on(real_t):
    prt, _, _ = production_run(real_t, True, steps=2)
    th, rv, rhod, C = production_case(real_t)["fields"]
    blob = prt.snapshot()
    assert prt.coal_rates_info()[0] is True, "taking a snapshot leaves the accumulators as they are"
    twin = h.hip_particles(production_case(real_t)["oi"], real_t)
    twin.coal_rates_enable(R_THR)                                      # (enabled before the load: a restored object starts disabled all the same)
    twin.restore(blob)
    assert twin.coal_rates_info() == (False, 0., 0)
    with pytest.raises(RuntimeError, match="not enabled"):
        twin.coal_rates()
    for p in (prt, twin):
        for _ in range(2):
            p.step_sync(coal_only(), th.copy(), rv.copy(), rhod.copy())
            p.step_async(coal_only())
    a, b = raw_state(prt), raw_state(twin)
    for nm in a:
        assert np.array_equal(a[nm], b[nm]), nm
    assert prt.coal_rates_info()[2] == 4 and sum(v.sum() for v in prt.coal_rates().values()) > 0
