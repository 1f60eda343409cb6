"""Condensation rates per cell (include/lcx_cond_rates.h) on the device, in double and float.

1. Droplet by droplet: the box of tests/test_cond_rates_design.py (which shows on the CPU oracle that every row of the table occurs in it),
   the raw storage read before and after one step_sync of condensation, the rows of tests/_cond_rates_reference.py against cond_rates().
   Numbers exact, M3 rows to (K_c + 8) eps_double S.  Strict, default and fast arithmetic, one and three substeps (the fused substep
   kernel), per-particle substeps, interleaved storage (runs of one lane), dead slots in the middle, several steps with a reset.
2. Closure against diag_wet_rng + diag_wet_mom on the path nobody steered (API defaults, 4 x 4 x 4 x 64).
3. TOTAL_DM3 against the call's change of rv.
4. Nothing else moves: state, fields, order and the next coalescence with the tally on and off, bit for bit; launch counts.
5. With the collision rates: the integer budget of the number of rain drops over steps of condensation and coalescence.
6. The surface.
"""
import ctypes as C

import numpy as np
import pytest

import _harness as h
import _cond_rates_reference as CD
import test_cond_rates_design as D
import test_hip_coal_rates as TCR
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

LD = np.longdouble
REALS = [np.float64, np.float32]
REAL_IDS = ["f64", "f32"]
THR = D.THR
RHO_W = 1e3
MODES = {"strict": dict(strict_fp=True, cond_solver=0), "default": None, "fast": dict(strict_fp=False, cond_solver=0)}


def set_mode(oi, mode):
    if MODES[mode] is None:
        h.api_default_opts(oi)
    else:
        oi.strict_fp, oi.cond_solver = MODES[mode]["strict_fp"], MODES[mode]["cond_solver"]
    return oi


def start(case, real_t, thr=THR, when="after"):
    th, rv, rhod = case["fields"]
    prt = h.hip_particles(case["oi"], real_t)
    if thr is not None and when == "before":
        prt.cond_rates_enable(thr)
    prt.init(th.copy(), rv.copy(), rhod.copy())
    if thr is not None and when == "after":
        prt.cond_rates_enable(thr)
    prt.set_particles(**case["args"])
    return prt


def step(prt, case, opts=None):
    th, rv, rhod = case["fields"]
    th2, rv2 = th.copy(), rv.copy()
    prt.step_sync(opts if opts is not None else D.cond_only(), th2, rv2, rhod.copy())
    return th2, rv2


def tallied_step(prt, case, real_t, lo, rows=None, n_cell=D.N_CELL):
    """one step_sync with the raw storage read before and after it; returns the reference's rows and the fields that came out"""
    b = D.raw(prt, real_t, "raw_")
    th2, rv2 = step(prt, case)
    a = D.raw(prt, real_t, "raw_")
    assert np.array_equal(b["ijk"], a["ijk"]) and np.array_equal(b["rd3"], a["rd3"]) and np.array_equal(b["n"], a["n"]), "slots do not move in step_cond"
    return CD.tally(a["n"], a["ijk"], b["rw2"], a["rw2"], lo, n_cell, rows), th2, rv2, b, a


def assert_rows(got, rows, tag):
    """got: (5 K + 1, n_cell) doubles of the device"""
    assert got.shape == (rows.n_rows, rows.n_cell)
    worst = 0.
    for w in range(rows.n_rows):
        for c in range(rows.n_cell):
            want = rows.value(w, c)
            if rows.is_number(w):
                assert want < 2 ** 53 and got[w, c] == float(want), (tag, "row", w, "cell", c, got[w, c], want)
            else:
                bar = CD.m3_bar(rows, w, c)
                err = abs(LD(got[w, c]) - want)
                if bar > 0:
                    worst = max(worst, float(err / bar))
                assert err <= bar, (tag, "row", w, "cell", c, got[w, c], float(want), "bar", float(bar))
    print("%-40s worst |M3 - reference| / bar: %.3f" % (tag, worst))


def as_block(prt):
    got = prt.cond_rates()
    k = len(prt.cond_rates_info()[1])
    out = np.zeros((5 * k + 1, got["total_dm3"].size))
    for w, nm in enumerate(lgrngn.COND_RATES):
        assert got[nm].shape == (k, out.shape[1])
        out[w:5 * k:5] = got[nm]
    out[5 * k] = got["total_dm3"]
    return out


def occurred(rows):
    """the case is not an empty one: crossings both ways at every threshold"""
    return all(rows.up[t].sum() >= 1 and rows.down[t].sum() >= 1 for t in range(rows.n_thr))


# ---------------------------------------------------------------------------------------------------- 1. droplet by droplet
@pytest.mark.parametrize("sstp", [1, 3], ids=["sstp1", "sstp3"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_every_droplet_of_one_step(real_t, mode, sstp):
    case = D.design(real_t, sstp_cond=sstp)
    set_mode(case["oi"], mode)
    prt = start(case, real_t, when="before" if sstp == 1 else "after")
    assert np.array_equal(prt.state_u64("raw_ijk"), case["cells"])
    rows, _, _, _, _ = tallied_step(prt, case, real_t, CD.bounds(THR, real_t))
    sfp, solver, ck, _ = prt.mode()
    print("mode", mode, "strict_fp", sfp, "cond_solver", solver, "kernel", ck.name)
    if mode == "strict":
        h.assert_mode(prt, True, 0, "strict")
    elif sstp == 3:
        h.assert_mode(prt, False, None, "substeps")                    # the fused substep kernel
    else:
        h.assert_mode(prt, False)
    assert occurred(rows), (rows.up, rows.down)
    assert prt.cond_rates_info() == (True, tuple(THR), 1)
    assert_rows(as_block(prt), rows, "%s %s sstp %d" % (real_t.__name__, mode, sstp))
    for c, m in enumerate(D.OCC):
        if m == 0:
            assert (as_block(prt)[:, c] == 0).all()


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_per_particle_substeps(real_t):
    case = D.design(real_t, sstp_cond=3, exact_sstp_cond=True)
    prt = start(case, real_t)
    rows, _, _, _, _ = tallied_step(prt, case, real_t, CD.bounds(THR, real_t))
    h.assert_mode(prt, True, None, "per_particle")
    assert occurred(rows)
    assert_rows(as_block(prt), rows, "%s exact_sstp_cond" % real_t.__name__)


def interleaved(case):
    cells = case["cells"]
    rank = np.arange(cells.size) - np.concatenate(([0], np.cumsum(D.OCC)))[cells]
    return D.permuted(case, np.lexsort((cells, rank)))


@pytest.mark.parametrize("mode", ["strict", "default"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_cells_interleaved_in_storage(real_t, mode):
    """the same droplets, stored by their rank in the cell first: adjacent slots lie in different cells, so runs have length 1"""
    case = interleaved(set_mode_case(D.design(real_t), mode))
    assert (np.diff(case["cells"][:100]) != 0).all()
    prt = start(case, real_t)
    assert np.array_equal(prt.state_u64("raw_ijk"), case["cells"])
    rows, _, _, _, _ = tallied_step(prt, case, real_t, CD.bounds(THR, real_t))
    assert occurred(rows)
    assert_rows(as_block(prt), rows, "%s %s interleaved" % (real_t.__name__, mode))


def set_mode_case(case, mode):
    set_mode(case["oi"], mode)
    return case


@pytest.mark.parametrize("mode", ["strict", "default"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_dead_slots_in_the_middle_of_the_storage(real_t, mode):
    case = set_mode_case(D.design(real_t), mode)
    dead = np.zeros(case["cells"].size, dtype=bool)
    dead[5::37] = True
    dead[200:203] = True
    case["args"]["n"] = np.where(dead, 0, case["args"]["n"]).astype(np.uint64)
    prt = start(case, real_t)
    assert np.array_equal(prt.state_u64("raw_n") == 0, dead), "set_particles keeps the n = 0 entries where they are"
    rows, _, _, b, a = tallied_step(prt, case, real_t, CD.bounds(THR, real_t))
    lo = CD.bounds(THR, real_t)
    print("dead slots whose radius went across a threshold (they must not count):", sum(int(((b["rw2"] < l) != (a["rw2"] < l))[dead].sum()) for l in lo))
    assert occurred(rows)
    assert_rows(as_block(prt), rows, "%s %s dead slots" % (real_t.__name__, mode))


@pytest.mark.parametrize("mode", ["strict", "default"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_three_steps_read_once_and_with_a_reset_in_between(real_t, mode):
    lo = CD.bounds(THR, real_t)
    idle = D.cond_only()
    idle.cond = False
    blocks = []
    for reset_after_first in (False, True):
        case = set_mode_case(D.design(real_t, sstp_cond=3), mode)
        prt = start(case, real_t)
        refs = [CD.Rows(3, D.N_CELL), CD.Rows(3, D.N_CELL)]
        whole = CD.Rows(3, D.N_CELL)
        reads = []
        for s in range(3):
            b = D.raw(prt, real_t, "raw_")
            step(prt, case)
            a = D.raw(prt, real_t, "raw_")
            assert np.array_equal(b["rd3"], a["rd3"])
            for r in (whole, refs[0 if s == 0 else 1]):
                CD.tally(a["n"], a["ijk"], b["rw2"], a["rw2"], lo, D.N_CELL, r)
            prt.step_async(idle)
            if reset_after_first and s == 0:
                assert prt.cond_rates_info()[2] == 1
                out = np.zeros((16, D.N_CELL))
                reads.append(prt.cond_rates(reset=True, out=out))
                assert prt.cond_rates_info()[2] == 0
        if reset_after_first:
            assert prt.cond_rates_info()[2] == 2
            reads.append(as_block(prt))
            assert_rows(reads[0], refs[0], "%s %s first step" % (real_t.__name__, mode))
            assert_rows(reads[1], refs[1], "%s %s steps two and three" % (real_t.__name__, mode))
            blocks.append(reads[0] + reads[1])
        else:
            assert prt.cond_rates_info()[2] == 3
            blocks.append(as_block(prt))
            assert_rows(blocks[0], whole, "%s %s three steps" % (real_t.__name__, mode))
    once, summed = blocks
    for w in range(16):
        if whole.is_number(w):
            assert np.array_equal(once[w], summed[w]), w
        else:
            for c in range(D.N_CELL):
                assert abs(LD(once[w, c]) - LD(summed[w, c])) <= 2 * CD.m3_bar(whole, w, c), (w, c)


# ---------------------------------------------------------------------------------------------------- 2. closure against the classic calls
THR4 = [0.1e-6, 0.5e-6, 1e-6, 25e-6]


def default_box(real_t, thr=THR4, when="after"):
    oi = h.api_default_opts(h.box_opts(4, 4, 4, 64))
    th, rv, rhod, Cc = h.box_fields(oi)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    fields = (f(th), f(rv), f(rhod), {k: f(v) for k, v in Cc.items()})
    prt = h.hip_particles(oi, real_t)
    if thr is not None and when == "before":
        prt.cond_rates_enable(thr)
    prt.init(fields[0].copy(), fields[1].copy(), fields[2].copy(), **{k: v.copy() for k, v in fields[3].items()})
    if thr is not None and when == "after":
        prt.cond_rates_enable(thr)
    return prt, fields


def classic(prt, real_t, r, k):
    prt.diag_wet_rng(r, 1)
    prt.diag_wet_mom(k)
    return np.frombuffer(prt.outbuf(), dtype=real_t).astype(LD)


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_budgets_close_against_diag_wet_rng_moments_on_the_default_path(real_t):
    prt, (th, rv, rhod, Cc) = default_box(real_t)
    scale = prt.state_real("dv").astype(LD) * rhod.astype(LD).ravel()
    cnt = np.bincount(prt.state_u64("raw_ijk").astype(np.int64), minlength=64)
    before = {(t, k): classic(prt, real_t, r, k) * scale for t, r in enumerate(THR4) for k in (0, 3)}
    prt.step_sync(lgrngn.opts_t(), th.copy(), rv.copy(), rhod.copy())
    sfp, solver, ck, flags = prt.mode()
    print("the default path: strict_fp", sfp, "cond_solver", solver, "kernel", ck.name)
    assert not sfp and solver == h.API_DEFAULTS["cond_solver"] and int(flags) == 0
    after = {(t, k): classic(prt, real_t, r, k) * scale for t, r in enumerate(THR4) for k in (0, 3)}
    got = prt.cond_rates()
    eps_t = LD(np.finfo(real_t).eps)
    crossed = 0
    for t in range(4):
        crossed += int(got["up_n"][t].sum() + got["down_n"][t].sum())
        budget = {0: got["up_n"][t].astype(LD) - got["down_n"][t].astype(LD),
                  3: got["above_dm3"][t].astype(LD) + got["up_m3"][t].astype(LD) - got["down_m3"][t].astype(LD)}
        for k in (0, 3):
            bar = (cnt + 8) * eps_t * (before[t, k] + after[t, k])
            d = (after[t, k] - before[t, k]) - budget[k]
            with np.errstate(all="ignore"):
                print("threshold %d moment %d  worst |change - budget| / bar: %.3f" % (t, k, float(np.nanmax(np.where(bar > 0, np.abs(d) / bar, 0)))))
            assert (np.abs(d) <= bar).all(), (t, k, np.abs(d).astype(float), bar.astype(float))
    assert crossed > 0 and (got["total_dm3"] != 0).all()


# ---------------------------------------------------------------------------------------------------- 3. rv
# How far the long-double total of the raw state (not the accumulators) lies from the device's own change of rv on the design box, in
# eps_T * rv, worst cell, as measured on an MI355X (EXPERIMENTS.md 7.12); the fast modes sum the cell's water in fixed point, so this is
# measured, not derived.  The bar is 8 times the measured value and never below 16 eps_T rv.
RV_MEASURED = {("float64", "strict"): .393, ("float64", "default"): .393, ("float64", "fast"): .387,
               ("float32", "strict"): .327, ("float32", "default"): .327, ("float32", "fast"): .325}       # 8 x these < 16: the bar is 16 eps_T rv


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_total_dm3_is_the_cells_change_of_rv(real_t, mode):
    case = set_mode_case(D.design(real_t), mode)
    prt = start(case, real_t)
    rows, _, rv2, _, _ = tallied_step(prt, case, real_t, CD.bounds(THR, real_t))
    rv = case["fields"][1]
    got = prt.cond_rates()["total_dm3"].astype(LD)
    dv, rhod = prt.state_real("dv").astype(LD), case["fields"][2].astype(LD).ravel()
    c = LD(4) / 3 * LD(np.pi) * LD(RHO_W)
    drv = (rv2.astype(LD) - rv.astype(LD)).ravel()
    unit = LD(np.finfo(real_t).eps) * rv.astype(LD).ravel()
    ref = np.array([rows.value(15, cc) for cc in range(D.N_CELL)], dtype=LD)
    measured = float(np.max(np.abs(-c * ref / (dv * rhod) - drv) / unit))
    dist = float(np.max(np.abs(-c * got / (dv * rhod) - drv) / unit))
    print("rv closure %s %s: reference total against the device's rv change %.3f eps_T rv, the tally against it %.3f" % (real_t.__name__, mode, measured, dist))
    bar = max(16., 8 * RV_MEASURED[(real_t.__name__, mode)])
    assert dist <= bar, (dist, bar)


# ---------------------------------------------------------------------------------------------------- 4. nothing else moves
def whole_state(prt, order=True):
    """order: with the sorted order (behind a step_async its re-sort may be left to the next condensation: not readable then)"""
    names = ("raw_n", "raw_rw2", "raw_rd3", "raw_ijk", "th", "rv") + (("raw_sorted_id",) if order else ())
    return {nm: prt.state_u64(nm) if nm in ("raw_n", "raw_sorted_id", "raw_ijk") else prt.state_real(nm) for nm in names}


@pytest.mark.parametrize("sstp", [1, 3], ids=["sstp1", "sstp3"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_design_step_moves_nothing_else(real_t, mode, sstp):
    res = []
    for thr in (THR, None):
        case = set_mode_case(D.design(real_t, sstp_cond=sstp), mode)
        prt = start(case, real_t, thr)
        th2, rv2 = step(prt, case)
        res.append(dict(whole_state(prt), th_out=th2, rv_out=rv2))
    for nm in res[0]:
        assert np.array_equal(res[0][nm], res[1][nm]), nm


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_default_box_moves_nothing_else_and_the_next_coalescence_is_the_same(real_t):
    res = []
    for thr in (THR4, None):
        prt, (th, rv, rhod, Cc) = default_box(real_t, thr)
        opts = lgrngn.opts_t()
        out = {}
        for s in range(2):
            th2, rv2 = th.copy(), rv.copy()
            prt.step_sync(opts, th2, rv2, rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
            out["after_sync_%d" % s] = dict(whole_state(prt), th_out=th2, rv_out=rv2)
            prt.step_async(opts)                                        # coalescence, advection and sedimentation of the API's defaults
            out["after_async_%d" % s] = whole_state(prt, order=False)
        res.append(out)
        if thr is not None:
            assert prt.cond_rates_info()[2] == 2
    for key in res[0]:
        for nm in res[0][key]:
            assert np.array_equal(res[0][key][nm], res[1][key][nm]), (key, nm)
    a, b = res[0]["after_sync_0"]["raw_n"], res[0]["after_async_1"]["raw_n"]
    assert a.size != b.size or not np.array_equal(a, b), "the coalescence did collide"


def launches_of_three_steps(prt, fields):
    th, rv, rhod, Cc = fields
    opts = lgrngn.opts_t()
    per_step = []
    for s in range(3):
        n0 = int(prt.state_u64("raw_launches")[0])
        prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
        n1 = int(prt.state_u64("raw_launches")[0])
        prt.step_async(opts)
        per_step.append((n1 - n0, int(prt.state_u64("raw_launches")[0]) - n1))
    return per_step


def test_launch_counts():
    never, fields = default_box(np.float64, None)
    n_never = launches_of_three_steps(never, fields)
    gone, fields = default_box(np.float64, THR4)
    gone.cond_rates_disable()
    assert gone.cond_rates_info() == (False, (), 0)
    n_gone = launches_of_three_steps(gone, fields)
    on, fields = default_box(np.float64, [25e-6])
    n_on = launches_of_three_steps(on, fields)
    print("launches per (step_sync, step_async): never enabled", n_never, "disabled", n_gone, "enabled", n_on)
    assert n_never == n_gone, "a disabled object launches what a never-enabled one does"
    for (s_on, a_on), (s_off, a_off) in zip(n_on, n_never):
        assert s_off + 1 <= s_on <= s_off + 2 and a_on == a_off, "at most two more launches per tallied step_cond (the copy is none)"


# ---------------------------------------------------------------------------------------------------- 5. with the collision rates
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_number_of_rain_drops_closes_in_integers_with_the_collision_rates(real_t):
    case = TCR.production_case(real_t)
    th, rv, rhod, Cc = case["fields"]
    prt = h.hip_particles(case["oi"], real_t)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    prt.set_particles(**case["args"])
    prt.cond_rates_enable(TCR.R_THR)
    prt.coal_rates_enable(TCR.R_THR)
    opts = lgrngn.opts_t()
    opts.adve = opts.sedi = False
    before = TCR.class_sums(prt, real_t, 64)
    for s in range(3):
        prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy())
        prt.step_async(opts)
    after = TCR.class_sums(prt, real_t, 64)
    cd, cl = prt.cond_rates(), prt.coal_rates()
    assert prt.cond_rates_info()[2] == 3 and prt.coal_rates_info()[2] == 3
    for c in range(64):
        want = int(cd["up_n"][0][c]) - int(cd["down_n"][0][c]) + int(cl["acnv_nr"][c]) - int(cl["self_rain_n"][c])
        assert after["Nr"][c] - before["Nr"][c] == want, (c, after["Nr"][c] - before["Nr"][c], want)
    print("crossed up", int(cd["up_n"][0].sum()), "down", int(cd["down_n"][0].sum()), "autoconverted", int(cl["acnv_nr"].sum()),
          "self-collected", int(cl["self_rain_n"].sum()))
    assert cd["up_n"][0].sum() + cd["down_n"][0].sum() > 0, "condensation carried droplets across the threshold"
    assert cl["acnv_nr"].sum() + cl["self_rain_n"].sum() > 0, "and collisions changed the number of rain drops"


# ---------------------------------------------------------------------------------------------------- 6. the surface
def test_every_error_text():
    case = D.design(np.float64)
    prt = h.hip_particles(case["oi"], np.float64)
    f = lambda name: getattr(prt._lib, "lcx_" + name)
    last = prt._f("last_error")
    last.restype = C.c_char_p
    arr = lambda *v: (C.c_double * len(v))(*v)
    for call in (prt.cond_rates, lambda: prt.diag_cond_rate("up_n"), lambda: prt.diag_cond_rate(0)):
        with pytest.raises(RuntimeError, match=r"libcloudph\+\+: cond_rates: .* while the tally is not enabled"):
            call()
    for k in (0, 5, -1):
        assert f("cond_rates_enable")(prt._h, arr(1e-6, 2e-6, 3e-6, 4e-6, 5e-6), C.c_int(k)) == 1
        assert "libcloudph++: cond_rates: n_thr = %d is outside 1 .. 4" % k in last().decode()
    for bad in (0., -1e-6, float("nan"), float("inf")):
        assert f("cond_rates_enable")(prt._h, arr(1e-6, bad), C.c_int(2)) == 1
        assert "libcloudph++: cond_rates: every threshold must be positive and finite" in last().decode()
    for bad in ((2e-6, 1e-6), (1e-6, 1e-6)):
        assert f("cond_rates_enable")(prt._h, arr(*bad), C.c_int(2)) == 1
        assert "libcloudph++: cond_rates: the thresholds must be strictly increasing" in last().decode()
    assert prt.cond_rates_info() == (False, (), 0)
    prt.cond_rates_enable(THR)                                          # before init()
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: cond_rates: diag_cond_rate before init\(\)"):
        prt.diag_cond_rate("total_dm3")
    th, rv, rhod = case["fields"]
    prt.init(th.copy(), rv.copy(), rhod.copy())
    out = np.zeros((16, 16))
    for row in (-1, 16):
        assert f("diag_cond_rate")(prt._h, C.c_int(row)) == 1 and "libcloudph++: cond_rates: row = %d is outside 0 .. 15" % row in last().decode()
    assert f("cond_rates_read")(prt._h, C.c_void_p(out.ctypes.data), C.c_size_t(15), C.c_int(0), C.c_int(0)) == 1
    assert "libcloudph++: cond_rates: stride (15) < n_cell (16)" in last().decode()
    assert f("cond_rates_read")(prt._h, None, C.c_size_t(16), C.c_int(0), C.c_int(0)) == 1 and "libcloudph++: cond_rates: out == NULL" in last().decode()
    assert f("cond_rates_read")(prt._h, C.c_void_p(out.ctypes.data), C.c_size_t(16), C.c_int(0), C.c_int(0)) == 0
    # two radii that differ in double and whose squares are one float
    close = (1e-6, 1e-6 * (1 + 1e-9))
    prt.cond_rates_enable(close)
    assert prt.cond_rates_info()[1] == close
    p32 = h.hip_particles(D.design(np.float32)["oi"], np.float32)
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: cond_rates: the bounds r_thr\^2 of thresholds 0 and 1 are not strictly increasing in the object's real type"):
        p32.cond_rates_enable(close)
    assert p32.cond_rates_info()[0] is False


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_enable_again_disable_and_a_call_without_condensation(real_t):
    case = D.design(real_t)
    prt = start(case, real_t, when="before")
    lo = CD.bounds(THR, real_t)
    tallied_step(prt, case, real_t, lo)
    assert (as_block(prt) != 0).any()
    idle = D.cond_only()
    idle.cond = False
    prt.step_async(idle)
    block = as_block(prt)
    step(prt, case, idle)                                               # opts.cond == False: rows and calls stay
    prt.step_async(idle)
    assert np.array_equal(as_block(prt), block) and prt.cond_rates_info()[2] == 1
    prt.cond_rates_enable(25e-6)                                        # other thresholds on an enabled object: zeroed, K = 1
    assert prt.cond_rates_info() == (True, (25e-6,), 0)
    assert as_block(prt).shape == (6, 16) and (as_block(prt) == 0).all()
    rows, _, _, _, _ = tallied_step(prt, case, real_t, lo[2:])
    assert_rows(as_block(prt), rows, "%s K = 1" % real_t.__name__)
    prt.step_async(idle)
    four = [1e-6, 1.5e-6, 25e-6, 30e-6]
    prt.cond_rates_enable(four)                                         # K = 4
    rows, _, _, _, _ = tallied_step(prt, case, real_t, CD.bounds(four, real_t))
    assert as_block(prt).shape == (21, 16)
    assert_rows(as_block(prt), rows, "%s K = 4" % real_t.__name__)
    prt.cond_rates_disable()
    assert prt.cond_rates_info() == (False, (), 0)
    with pytest.raises(RuntimeError, match="not enabled"):
        prt.cond_rates()


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_diag_cond_rate_and_device_output(real_t):
    import torch
    case = D.design(real_t)
    prt = start(case, real_t)
    step(prt, case)
    got = as_block(prt)
    assert (got[[1, 3, 6, 8, 11, 13]].sum(1) > 0).all()
    dv, rhod = prt.state_real("dv").astype(real_t), prt.state_real("rhod").astype(real_t)
    for row in range(16):
        if row == 15:
            prt.diag_cond_rate("total_dm3")
        elif row % 2:
            prt.diag_cond_rate(lgrngn.COND_RATES[row % 5], row // 5)
        else:
            prt.diag_cond_rate(row)
        out = np.frombuffer(prt.outbuf(), dtype=real_t).copy()
        want = (got[row].astype(real_t) / dv) / rhod                   # (the division in the object's type, by dv and then by rhod)
        assert np.array_equal(out, want), row
    buf = torch.full((16, 24), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    prt.cond_rates(out=lgrngn.DeviceArray(buf.data_ptr(), (16, 16), (24, 1)))
    host = buf.cpu().numpy()
    assert np.array_equal(host[:, :16], got)
    assert (host[:, 16:] == -1).all(), "the elements between n_cell and the stride are not written"
    wide = np.full((16, 20), -2.)
    prt.cond_rates(out=wide[:, :16])
    assert np.array_equal(wide[:, :16], got) and (wide[:, 16:] == -2).all()


def test_a_parcel_is_not_divided():
    oi = lgrngn.opts_init_t()
    oi.dt, oi.sd_conc, oi.n_sd_max = 1., 64, 64
    oi.dry_distros = {(.61, 0.): h.lgrngn_bimodal()}
    oi.coal_switch = oi.sedi_switch = False
    prt = h.hip_particles(oi)
    prt.init(np.array([300.]), np.array([.010]), np.array([1.1]))
    prt.cond_rates_enable([0.05e-6])
    prt.step_sync(D.cond_only(), np.array([300.]), np.array([.012]), np.array([1.1]))      # moister air than the droplets were in equilibrium with
    got = as_block(prt)
    assert got[5, 0] > 0 and got[0, 0] + got[2, 0] > 0, got[:, 0]
    for row in range(6):
        prt.diag_cond_rate(row)
        assert np.frombuffer(prt.outbuf(), dtype=np.float64)[0] == got[row, 0], row


def test_a_multi_device_object_is_refused(monkeypatch):
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = h.box_opts(4, 4, 4, 16)
    oi.dev_count = 2
    prt = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert prt.dev_count == 2
    for call in (lambda: prt.cond_rates_enable(THR), prt.cond_rates_disable, prt.cond_rates_info, prt.cond_rates, lambda: prt.diag_cond_rate(0)):
        with pytest.raises(RuntimeError, match=r"libcloudph\+\+: cond_rates on a multi-device object is not built"):
            call()


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_a_snapshot_drops_the_tally_and_the_run_goes_on(real_t):
    prt, (th, rv, rhod, Cc) = default_box(real_t)
    opts = lgrngn.opts_t()
    kw = lambda: {k: v.copy() for k, v in Cc.items()}
    prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **kw())
    prt.step_async(opts)
    blob = prt.snapshot()
    assert prt.cond_rates_info() == (True, tuple(THR4), 1), "taking a snapshot leaves the tally as it is"
    twin = h.hip_particles(h.api_default_opts(h.box_opts(4, 4, 4, 64)), real_t)
    twin.cond_rates_enable(THR)                                         # (enabled before the load: a restored object starts disabled all the same)
    twin.restore(blob)
    assert twin.cond_rates_info() == (False, (), 0)
    with pytest.raises(RuntimeError, match="not enabled"):
        twin.cond_rates()
    for p in (prt, twin):
        p.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **kw())
        p.step_async(opts)
    a, b = whole_state(prt, order=False), whole_state(twin, order=False)
    for nm in a:
        assert np.array_equal(a[nm], b[nm]), nm
    assert prt.cond_rates_info()[2] == 2 and (prt.cond_rates()["total_dm3"] != 0).any()
