"""The collision log (include/lcx_coal_log.h) on the device, in double and float.

1. Replay identity of one launch: a 4 x 4 box of crafted cell occupancies (around the wave, the ranked cell's window and the ranked tile),
   the raw state before and after stage("coal") against the events, item by item (tests/_coal_log_reference.py replay_one_launch).
2. The same through step_async in every launch form of lcx_coal_plan.hpp, forced by the debug toggles and asserted from the raw_coal_*
   counters; all forms must log the same set of events.  The kernels that rank for themselves take no order with a cell above 256 droplets
   in it (lcx_core.hip cells_rankable), so the forms run on the box OCC_RANKABLE; the box of test 1 goes through step_async as well and is
   asserted to take the PAIRS form.  The Onishi kernel with turb_coal; three substeps.
3. The log reduces to the collision rates by the table of include/lcx_coal_rates.h.
4. The filter and the overflow: three twins of one box.
5. Nothing else moves: state, fields, counters, random numbers, the rates, launches and host waits, log on and off.
6. Slots are the caller's: a dump between step_sync and step_async joins to the step's events.
7. Scope and errors.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _harness as h
import _coal_log_reference as CL
import _coal_rates_reference as CR
from libcloudphxx_amd import lgrngn
from test_hip_coal_rates import COLLIDE_BAR, coal_only, production_case

pytestmark = pytest.mark.gpu

LD = np.longdouble
R_25 = 25e-6
REALS = [np.float64, np.float32]
REAL_IDS = ["f64", "f32"]
ARITH = [(np.float64, False), (np.float64, True), (np.float32, False), (np.float32, True)]
ARITH_IDS = ["f64", "f64-strict", "f32", "f32-strict"]
D2, DBG = lgrngn.dbg2, lgrngn.dbg
# name: (dbg_flags, dbg_flags2, the form of the first step's launch, of the second step's).  The second step's order is owed again by the first
# one's re-sort, but no velocity pass has armed a bound for it: the plain RANKED form, unless the list form is forced
FORMS = {
    "default": (0, 0, "RANKED_TILES", "RANKED"),
    "no-rank-exit": (0, int(D2.NO_COAL_RANK_EXIT), "RANKED_SKIP", "RANKED"),
    "rank-exit-always": (0, int(D2.COAL_RANK_EXIT_ALWAYS), "RANKED_TILES", "RANKED"),
    "no-prevote": (0, int(D2.NO_COAL_PREVOTE), "RANKED_EXIT", "RANKED"),
    "no-cell-list": (0, int(D2.NO_COAL_CELL_LIST), "RANKED_TILES", "RANKED"),
    "cell-list-always": (0, int(D2.COAL_CELL_LIST_ALWAYS) | int(D2.COAL_RANK_EXIT_ALWAYS), "CELLS", "CELLS"),
    "cell-list-small": (0, int(D2.COAL_CELL_LIST_ALWAYS) | int(D2.COAL_RANK_EXIT_ALWAYS) | int(D2.COAL_CELL_LIST_SMALL), "CELLS", "CELLS"),
    "no-bound": (int(DBG.NO_COAL_SKIP), 0, "RANKED", "RANKED"),
    "no-rank-in-coal": (int(DBG.NO_RANK_IN_COAL), 0, "PAIRS", "PAIRS"),
}


def lo_of(real_t, r=R_25):
    return real_t(np.float64(r) ** 2)                                 # (lcx::diag::rng_bounds: the square in double, then the object's type)


def fields_of(oi, real_t):
    th, rv, rhod, C_ = h.box_fields(oi)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    return f(th), f(rv), f(rhod), {k: f(v) for k, v in C_.items()}


def make(occ, real_t, strict=False, flags=0, flags2=0, seed=1, **kw):
    """a 4 x 4 box holding occ[c] droplets in cell c, the tabulated kernel and beard77fast: (object, case, fields)"""
    oi = h.box_opts(4, 0, 4, 2, dx=1., dt=1., n_sd_max=sum(occ) + 16, kernel=lgrngn.kernel_t.hall, terminal_velocity=lgrngn.vt_t.beard77fast,
                    strict_fp=bool(strict), cond_solver=0, **kw)
    oi.dbg_flags, oi.dbg_flags2 = flags, flags2
    case = CL.occupancy_case(occ, real_t, seed)
    F = fields_of(oi, real_t)
    prt = h.hip_particles(oi, real_t)
    prt.init(F[0].copy(), F[1].copy(), F[2].copy(), **{k: v.copy() for k, v in F[3].items()})
    prt.set_particles(**case["args"])
    return prt, case, F


def raw(prt):
    st = {nm: prt.state_real("raw_" + nm) for nm in ("rw2", "rd3", "vt", "kappa")}
    st["n"], st["ijk"] = prt.state_u64("raw_n"), prt.state_u64("raw_ijk").astype(np.int64)
    return st


def carried_back(before, after):
    """the state `after` a step by the slots of `before`: the storage may have been re-ordered at the step's end, and droplets are matched by
    their kappa, unique in CL.occupancy_case (their positions are unique too, but the move's periodic wrap may round them in the last bit)"""
    where = {k: i for i, k in enumerate(after["kappa"].tolist())}
    assert len(where) == len(after["n"])
    idx = np.array([where.get(k, -1) for k in before["kappa"].tolist()], dtype=np.int64)
    out = {nm: after[nm][np.maximum(idx, 0)] for nm in ("n", "rw2", "rd3", "vt")}
    out["gone"] = idx < 0                                               # (used up and compacted away by the step's end)
    return out


def signature(prt):
    g = lambda nm: [int(v) for v in prt.state_u64(nm)]
    return dict(ranked=g("raw_coal_ranked")[0], skip=g("raw_coal_skip")[0], exit=g("raw_coal_exit")[0], flags=g("raw_coal_prevote")[0],
                cells=g("raw_coal_cells")[0], kernel=g("raw_coal_kernel")[0])


def form_of(s):
    """the launch form of lcx_coal_plan.hpp that a step with one coalescence launch took, from the counters"""
    if s["ranked"] == 0:
        return "PAIRS"
    if s["skip"] == 0:
        return "RANKED"
    if s["exit"] == 0:
        return "RANKED_SKIP"
    if s["cells"]:
        return "CELLS"
    return "RANKED_TILES" if s["flags"] else "RANKED_EXIT"


def step(prt, F, opts=None, **kw):
    opts = opts or coal_only()
    prt.step_sync(opts, F[0].copy(), F[1].copy(), F[2].copy(), **kw)
    prt.step_async(opts)


# ---------------------------------------------------------------------------------------------------- 1. one launch
@pytest.mark.parametrize("real_t,strict", ARITH, ids=ARITH_IDS)
def test_replay_identity_of_one_launch(real_t, strict):
    prt, case, F = make(CL.OCC, real_t, strict)
    prt.step_sync(coal_only(), F[0].copy(), F[1].copy(), F[2].copy())
    prt.stage("hskpng_Tpr")
    prt.stage("hskpng_vterm_all")
    prt.coal_log_enable(4096)
    before = raw(prt)
    assert np.array_equal(before["ijk"], case["cells"]) and (before["vt"] > 0).all()
    prt.stage("coal", coal_only())
    after = raw(prt)
    en, cap, r_min, held, seen, launches = prt.coal_log_info()
    assert (en, cap, r_min, launches) == (True, 4096, 0., 1)
    ev = prt.coal_log()
    assert set(ev) == set(lgrngn.COAL_LOG_FIELDS) and all(v.dtype == np.float64 and v.shape == (held,) for v in ev.values())
    assert (ev["launch"] == 0).all()
    E = CL.replay_one_launch(ev, before, after, real_t, strict, COLLIDE_BAR[real_t], "stage(coal) %s" % real_t.__name__)
    assert seen == held == E
    assert np.array_equal(ev["cell"], before["ijk"][ev["slot_r"].astype(np.int64)]) and np.array_equal(ev["cell"], before["ijk"][ev["slot_d"].astype(np.int64)])
    print("events", E, "of", case["pairs"], "pairs; used up", int((ev["n_d"] == ev["col_no"] * ev["n_r"]).sum()), "col_no > 1", int((ev["col_no"] > 1).sum()))
    assert 3 * E >= case["pairs"], "a third of the pairs or more collide"
    equal = ev["n_d"] == ev["n_r"]
    assert (equal & (ev["n_d"] == ev["col_no"] * ev["n_r"])).any(), "a donor used up in the capped regime with equal multiplicities"
    assert len(set(ev["cell"].tolist())) >= 10, "the cells with pairs log"
    assert prt.coal_log_info()[3:5] == (E, E), "a read without reset leaves the log as it is"


# ---------------------------------------------------------------------------------------------------- 2. every launch form
@functools.lru_cache(maxsize=None)
def form_run(name, real_t, occ_name="OCC_RANKABLE", steps=2):
    """`steps` steps of the box under FORMS[name]: per step the form that ran, its counters and its events (replayed against the state)"""
    flags, flags2 = FORMS[name][:2]
    prt, case, F = make(getattr(CL, occ_name), real_t, False, flags, flags2)
    prt.coal_log_enable(1 << 12)
    out = []
    for s in range(steps):
        prt.step_sync(coal_only(), F[0].copy(), F[1].copy(), F[2].copy())
        before = raw(prt)
        prt.step_async(coal_only())
        sig = signature(prt)
        ev = prt.coal_log(reset=True)
        after = carried_back(before, raw(prt))
        assert (ev["launch"] == s).all(), "one launch per step, counted from enable on"
        # (VT_* are the velocity pass's of this step_async, which the state before it does not hold yet: compared with the donors' afterwards)
        E = CL.replay_one_launch(ev, before, after, real_t, False, COLLIDE_BAR[real_t], "%s %s step %d %s" % (occ_name, name, s, real_t.__name__), vt="after")
        out.append(dict(form=form_of(sig), sig=sig, ev=CL.sort_events(ev), E=E, pairs=case["pairs"]))
    assert prt.coal_log_info()[3:] == (0, 0, steps)
    return out


@pytest.mark.parametrize("name", list(FORMS))
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_every_launch_form_logs_the_same_events(real_t, name):
    got, ref = form_run(name, real_t), form_run("no-rank-in-coal", real_t)
    print(name, [(g["form"], g["sig"], g["E"]) for g in got])
    assert got[0]["form"] == FORMS[name][2], got[0]["sig"]
    assert got[1]["form"] == FORMS[name][3] and got[1]["sig"]["kernel"] == 2, got[1]["sig"]
    for s in range(2):
        assert got[s]["E"] > 0 and (s > 0 or 3 * got[s]["E"] >= got[s]["pairs"])
        CL.assert_same_events(got[s]["ev"], ref[s]["ev"], "%s step %d" % (name, s))


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_cells_above_the_ranked_window_go_through_step_async_in_the_pairs_form(real_t):
    """the box of test 1 (cells of 257, 511, 513 and 1030 droplets): no kernel ranks such an order for itself, whatever the toggles say, and
    the production k_coal logs it -- several workgroups of it, cells across their edges"""
    a, b = form_run("default", real_t, "OCC"), form_run("cell-list-always", real_t, "OCC")
    for s in range(2):
        assert a[s]["form"] == b[s]["form"] == "PAIRS" and a[s]["sig"]["kernel"] == 2, (a[s]["sig"], b[s]["sig"])
        CL.assert_same_events(a[s]["ev"], b[s]["ev"], "step %d" % s)
    assert 3 * a[0]["E"] >= a[0]["pairs"]


def production(real_t, log=None, rates=False, steps=4, onishi=False, sstp_coal=1, flags=0, dump_first=None):
    """the production case of the collision rates (4 x 4 x 4 cells x 64): log = (capacity, r_min) or None; returns (object, fields)"""
    case = production_case(real_t, onishi)
    case["oi"].sstp_coal = sstp_coal
    case["oi"].dbg_flags = flags
    th, rv, rhod, C_ = case["fields"]
    prt = h.hip_particles(case["oi"], real_t)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C_.items()})
    prt.set_particles(**case["args"])
    if rates:
        prt.coal_rates_enable(R_25)
    if log:
        prt.coal_log_enable(*log)
    opts = coal_only()
    opts.turb_coal = onishi
    kw = {"diss_rate": np.full(th.shape, 1e-2, dtype=real_t)} if onishi else {}
    for s in range(steps):
        prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **kw)
        if dump_first is not None and s == 0:
            dump_first.append(prt.dump(fields=("slot", "n", "rw2")))
        prt.step_async(opts)
    return prt, (th, rv, rhod, kw)


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_onishi_kernel_with_turb_coal(real_t):
    case = production_case(real_t, True)
    th, rv, rhod, C_ = case["fields"]
    prt = h.hip_particles(case["oi"], real_t)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C_.items()})
    prt.set_particles(**case["args"])
    prt.coal_log_enable(4096)
    opts = coal_only()
    opts.turb_coal = True
    prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), diss_rate=np.full(th.shape, 1e-2, dtype=real_t))
    before = raw(prt)
    prt.step_async(opts)
    assert int(prt.state_u64("raw_coal_kernel")[0]) == 1 and int(prt.state_u64("raw_coal_ranked")[0]) == 0
    ev = prt.coal_log()
    after = raw(prt)
    CL.assert_key_unique(ev)
    D, Rr = ev["slot_d"].astype(np.int64), ev["slot_r"].astype(np.int64)
    assert len(ev["launch"]) > 50 and len(set(np.concatenate([D, Rr]).tolist())) == 2 * len(D)
    # (this box's droplets carry no unique mark: the events are held to the state before by slot, and to the state after as a multiset)
    assert np.array_equal(ev["n_d"].astype(np.uint64), before["n"][D]) and np.array_equal(ev["n_r"].astype(np.uint64), before["n"][Rr])
    for f in ("rw2", "rd3"):
        assert np.array_equal(CL.bits(ev[f + "_d"]), CL.bits(before[f][D])) and np.array_equal(CL.bits(ev[f + "_r"]), CL.bits(before[f][Rr])), f
    assert np.array_equal(ev["cell"], before["ijk"][D]) and np.array_equal(ev["cell"], before["ijk"][Rr])
    assert (ev["vt_d"] > 0).all() and (ev["vt_r"] > 0).all()
    assert CL.live_multiset(*CL.expected_after(before, ev)) == CL.live_multiset(after["n"], after["rw2"])


# ---------------------------------------------------------------------------------------------------- 3. the log reduces to the rates
@pytest.mark.parametrize("sstp_coal", [1, 3])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_log_reduces_to_the_collision_rates(real_t, sstp_coal):
    prt, _ = production(real_t, (64 * 64 * 4 * sstp_coal, 0.), True, 4, sstp_coal=sstp_coal)
    en, cap, r_min, held, seen, launches = prt.coal_log_info()
    assert launches == 4 * sstp_coal == prt.coal_rates_info()[2] and held == seen > 0
    ev = prt.coal_log()
    CL.assert_key_unique(ev)
    assert sorted(set(ev["launch"].tolist())) == list(range(4 * sstp_coal))
    sums = CL.reduce_to_rates(ev, lo_of(real_t), 64)
    got = prt.coal_rates()
    for w, nm in enumerate(CR.NAMES):
        for c in range(64):
            want = sums.value(w, c)
            if w in CR.M3_ROWS:
                bar = CR.m3_bar(sums, w, c, real_t, COLLIDE_BAR[real_t])
                assert abs(LD(got[nm][c]) - want) <= bar, (nm, "cell", c, got[nm][c], float(want), "bar", float(bar))
            else:
                assert want < 2 ** 53 and got[nm][c] == float(want), (nm, "cell", c, got[nm][c], want)
    print("events", held, "rows", sums.rows)
    assert sums.rows["cc->r"] > 0 and sums.rows["cr"] + sums.rows["rc"] > 0, ("autoconversion and accretion both occurred", sums.rows)
    assert got["acnv_nr"].sum() > 0 and got["accr_nc"].sum() > 0


# ---------------------------------------------------------------------------------------------------- 4. filter and overflow
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_filter_and_the_overflow(real_t):
    (A, FA), (B, _), (Cc, _) = (production(real_t, log, steps=2) for log in ((1 << 14, 0.), (1 << 14, R_25), (5, 0.)))
    a, b, c = A.coal_log(), B.coal_log(), Cc.coal_log()
    ia, ib, ic = A.coal_log_info(), B.coal_log_info(), Cc.coal_log_info()
    lo = float(lo_of(real_t))
    keep = a["rw2_new"] >= lo
    assert 0 < keep.sum() < len(keep), "the threshold must split the events"
    assert ib[3] == ib[4] == int(keep.sum()) and ib[2] == R_25
    CL.assert_same_events({f: a[f][keep] for f in CL.FIELDS}, b, "r_min = 25 um")
    assert ia[3] == ia[4] == len(keep) and ic[3:5] == (5, ia[4]) and ic[1] == 5
    assert all(len(c[f]) == 5 for f in CL.FIELDS)
    CL.assert_key_unique(c)
    CL.subset_rows(c, a)
    for nm in ("raw_n", "raw_rw2", "raw_rd3", "raw_vt"):
        get = (lambda p: p.state_u64(nm)) if nm == "raw_n" else (lambda p: CL.bits(p.state_real(nm)))
        assert np.array_equal(get(A), get(Cc)) and np.array_equal(get(A), get(B)), nm
    # a resetting read empties the log, and the next step fills it from index 0
    again = Cc.coal_log(reset=True)
    CL.assert_same_events(again, c, "the resetting read returns what was held")
    assert Cc.coal_log_info()[3:] == (0, 0, 2) and all(len(v) == 0 for v in Cc.coal_log().values())
    A.coal_log(reset=True)
    for p in (A, Cc):
        step(p, FA)
    a3, c3 = A.coal_log(), Cc.coal_log()
    assert (a3["launch"] == 2).all() and (c3["launch"] == 2).all() and len(c3["launch"]) == 5 and Cc.coal_log_info()[4] == len(a3["launch"]) > 5
    CL.subset_rows(c3, a3)


# ---------------------------------------------------------------------------------------------------- 5. nothing else moves
def everything(prt, F):
    st = {nm: CL.bits(prt.state_real(nm)) for nm in ("raw_rw2", "raw_rd3", "raw_vt", "raw_x", "raw_y", "raw_z", "raw_kappa", "th", "rv")}
    st.update({nm: prt.state_u64(nm) for nm in ("raw_n", "raw_ijk", "raw_mode", "raw_coal_kernel", "raw_coal_ranked", "raw_coal_skip", "raw_coal_exit",
                                                "raw_coal_prevote", "raw_coal_cells", "raw_collided")})
    return st


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_nothing_else_moves(real_t):
    """full steps (condensation, advection, sedimentation, coalescence with the rates on) of the production box, log on and off: the whole
    raw state, th and rv, the mode and launch counters, the collision rates; n_part, launches and host waits of a step"""
    res = []
    for log in ((1 << 14, 0.), None):
        case = production_case(real_t)
        th, rv, rhod, C_ = case["fields"]
        prt = h.hip_particles(case["oi"], real_t)
        prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C_.items()})
        prt.set_particles(**case["args"])
        prt.coal_rates_enable(R_25)
        if log:
            prt.coal_log_enable(*log)
        opts = lgrngn.opts_t()
        tha, rva = th.copy(), rv.copy()
        counts = []
        for s in range(4):
            prt.step_sync(opts, tha, rva, rhod.copy(), **{k: v.copy() for k, v in C_.items()})
            l0 = prt.state_u64("raw_launches")
            prt.step_async(opts)
            l1 = prt.state_u64("raw_launches")
            counts.append((int(l1[0] - l0[0]), int(l1[1] - l0[1]), int(prt.n_part)))
        res.append((everything(prt, None), {k: CL.bits(v) for k, v in prt.coal_rates().items()}, counts, CL.bits(tha), CL.bits(rva), prt))
    on, off = res
    for nm in on[0]:
        assert np.array_equal(on[0][nm], off[0][nm]), nm
    numbers = [nm for w, nm in enumerate(CR.NAMES) if w not in CR.M3_ROWS]
    for nm in numbers:
        assert np.array_equal(on[1][nm], off[1][nm]), nm
    m3 = [nm for w, nm in enumerate(CR.NAMES) if w in CR.M3_ROWS]
    # The two M3 rows are sums of positive terms added by floating-point atomics: their last bits depend on the arrival order and may differ
    # between two runs of the same state, log or no log (include/lcx_coal_rates.h: each within K 2^-52 sum |term| of the exact sum, K the cell's
    # events: at most 32 pairs x 4 steps here).  Two runs are therefore held to 2 K 2^-52 of each other, and the printout says whether they were equal.
    for nm in m3:
        a, b = on[1][nm].view(np.float64), off[1][nm].view(np.float64)
        print(nm, "bitwise equal with and without the log:", bool(np.array_equal(a, b)))
        assert (np.abs(a - b) <= 2 * 128 * 2.0 ** -52 * np.maximum(a, b)).all(), nm
    assert on[2] == off[2], ("launches, host waits and n_part of every step", on[2], off[2])
    assert np.array_equal(on[3], off[3]) and np.array_equal(on[4], off[4]), "the caller's th and rv"
    assert on[5].coal_log_info()[4] > 0 and sum(v.view(np.float64).sum() for v in on[1].values()) > 0


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_random_numbers_are_what_they_were(real_t):
    """lcx_rng_dump needs tagged droplets, which take the production kernel without the in-cell ranking: its own stream, log on and off"""
    dumps = []
    for log in ((1 << 14, 0.), None):
        prt, _ = production(real_t, log, steps=2, flags=int(DBG.TAG))
        dumps.append([prt.rng_dump(0, which) for which in (0, 1)] + [prt.state_u64("raw_n"), prt.state_real("raw_rw2")])
        if log:
            assert prt.coal_log_info()[4] > 0
    for x, y in zip(*dumps):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------- 6. slots are the caller's
@pytest.mark.parametrize("sstp_coal", [1, 3])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_a_dump_before_step_async_joins_to_the_events_by_slot(real_t, sstp_coal):
    dumped = []
    prt, _ = production(real_t, (1 << 14, 0.), steps=1, sstp_coal=sstp_coal, dump_first=dumped)
    d = dumped[0]
    slot = d["slot"].astype(np.int64)
    n_of, rw2_of = np.zeros(slot.max() + 1), np.full(slot.max() + 1, np.nan)
    n_of[slot], rw2_of[slot] = d["n"], d["rw2"]
    ev = prt.coal_log()
    CL.assert_key_unique(ev)
    first = ev["launch"] == 0
    assert first.sum() > 0 and set(ev["launch"].tolist()) <= set(range(sstp_coal))
    D, Rr = ev["slot_d"][first].astype(np.int64), ev["slot_r"][first].astype(np.int64)
    assert np.array_equal(n_of[D], ev["n_d"][first]) and np.array_equal(n_of[Rr], ev["n_r"][first])
    assert np.array_equal(CL.bits(rw2_of[D]), CL.bits(ev["rw2_d"][first])) and np.array_equal(CL.bits(rw2_of[Rr]), CL.bits(ev["rw2_r"][first]))
    # later substeps: the slots still name the same droplets (nothing is re-ordered inside step_async's coalescence), grown or thinned since
    later = ~first
    if later.any():
        assert (ev["n_d"][later] <= n_of[ev["slot_d"][later].astype(np.int64)]).all()
        assert (ev["rw2_r"][later] >= rw2_of[ev["slot_r"][later].astype(np.int64)]).all()


# ---------------------------------------------------------------------------------------------------- 7. scope and errors
def test_every_error_text_and_each_state_of_info():
    case = production_case(np.float64)
    th, rv, rhod, C_ = case["fields"]
    prt = h.hip_particles(case["oi"], np.float64)
    assert prt.coal_log_info() == (False, 0, 0., 0, 0, 0)
    prt.coal_log_disable()                                              # (no error if the log is not enabled)
    prt.coal_log_enable(100, R_25)                                      # before init()
    assert prt.coal_log_info() == (True, 100, R_25, 0, 0, 0)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in C_.items()})
    prt.set_particles(**case["args"])
    step(prt, (th, rv, rhod))
    first = prt.coal_log_info()
    assert first[:3] == (True, 100, R_25) and first[4] > 0 and first[5] == 1
    prt.coal_log_enable(4096)                                           # again, after init(): re-allocated and cleared
    assert prt.coal_log_info() == (True, 4096, 0., 0, 0, 0)
    step(prt, (th, rv, rhod))
    held = prt.coal_log_info()[3]
    assert held > 8
    f = lambda name: getattr(prt._lib, "lcx_coal_log_" + name)
    last = prt._f("last_error")
    last.restype = C.c_char_p
    sz, i32 = C.c_size_t, C.c_int
    out = np.full((14, held), -1.)
    ptr = C.c_void_p(out.ctypes.data)
    read = lambda p, stride, cap_ev: f("read")(prt._h, p, sz(stride), sz(cap_ev), i32(0), i32(1), None, None)
    assert read(None, held, held) == 1 and last().decode() == "libcloudph++: coal_log: out == NULL"
    assert read(ptr, held - 1, held) == 1 and last().decode() == "libcloudph++: coal_log: field_stride (%d) < cap_events (%d)" % (held - 1, held)
    assert read(ptr, held, held - 1) == 1 and last().decode() == "libcloudph++: coal_log: cap_events (%d) < held (%d)" % (held - 1, held)
    assert read(ptr, held, 0) == 1 and last().decode() == "libcloudph++: coal_log: cap_events (0) < held (%d)" % held
    assert (out == -1).all() and prt.coal_log_info()[3:] == (held, held, 1), "a failed read writes nothing and resets nothing"
    for cap, r, text in ((0, 0., "capacity == 0"), (8, -1e-6, "r_min must be non-negative and finite"), (8, float("nan"), "r_min must be non-negative and finite"),
                         (8, float("inf"), "r_min must be non-negative and finite"),
                         (2 ** 64 - 1, 0., "capacity = %d: a list of 14 rows has more bytes than size_t holds" % (2 ** 64 - 1))):
        assert f("enable")(prt._h, sz(cap), C.c_double(r)) == 1 and last().decode() == "libcloudph++: coal_log: " + text
    huge = 2 ** 44                                                      # (1.8e15 bytes: no device holds them)
    assert f("enable")(prt._h, sz(huge), C.c_double(0.)) == 1
    assert last().decode().startswith("libcloudph++: coal_log: the device allocation of %d bytes failed" % (huge * 14 * 8)), last().decode()
    assert prt.coal_log_info() == (True, 4096, 0., held, held, 1), "a failed enable leaves the object as it was"
    n_w, seen = sz(), C.c_ulonglong()
    assert f("read")(prt._h, ptr, sz(held), sz(held), i32(0), i32(0), C.byref(n_w), C.byref(seen)) == 0 and (n_w.value, seen.value) == (held, held)
    assert (out != -1).all()
    prt.coal_log_disable()
    assert prt.coal_log_info() == (False, 0, 0., 0, 0, 0)
    assert read(ptr, held, held) == 1 and last().decode() == "libcloudph++: coal_log: read while the log is not enabled (lcx_coal_log_enable)"
    with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: coal_log: read while the log is not enabled"):
        prt.coal_log()
    step(prt, (th, rv, rhod))                                           # a disabled object runs on


def test_device_output_equals_host_output():
    import torch
    prt, _ = production(np.float64, (1 << 14, 0.), steps=2)
    host = prt.coal_log()
    held = len(host["launch"])
    buf = torch.full((14, held + 16), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res = prt.coal_log(out=lgrngn.DeviceArray(buf.data_ptr(), (14, held + 5), (held + 16, 1)))
    assert res == {"n_written": held, "seen": held}
    dev = buf.cpu().numpy()
    assert (dev[:, held:] == -1).all(), "elements at and beyond held, and between the rows, are not written"
    CL.assert_same_events({f: dev[i, :held] for i, f in enumerate(CL.FIELDS)}, host, "device output")
    small = torch.full((14, held - 1), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"cap_events \(%d\) < held \(%d\)" % (held - 1, held)):
        prt.coal_log(out=lgrngn.DeviceArray(small.data_ptr(), (14, held - 1), (held - 1, 1)))
    assert (small.cpu().numpy() == -1).all()


def test_a_multi_device_object_is_refused(monkeypatch):
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = h.box_opts(4, 4, 4, 16)
    oi.dev_count = 2
    prt = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert prt.dev_count == 2
    for call in (lambda: prt.coal_log_enable(64), prt.coal_log_disable, prt.coal_log_info, prt.coal_log):
        with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: coal_log on a multi-device object is not built$"):
            call()


def test_a_slab_with_neighbours_logs_its_own_events():
    oi = h.box_opts(6, 0, 5, 24, dx=20., kernel=lgrngn.kernel_t.hall)
    oi.n_sd_max = 24 * 6 * 5 * 3
    th, rv, rhod, Cc = h.box_fields(oi)
    ring = h.LocalRing(oi, 2, h.hip_particles, h.dev_alloc)
    ring.init(th.copy(), rv.copy(), rhod.copy(), **Cc)
    for prt in ring.prts:                                               # drizzle: 100 um and 50 um drops by turns, many of each
        N = len(prt.state_u64("n"))
        prt.set_particles(np.full(N, 10 ** 9, dtype=np.uint64), prt.get_attr("rd3"), np.where(np.arange(N) % 2 == 0, 100e-6 ** 2, 50e-6 ** 2),
                          prt.get_attr("kappa"), prt.state_real("vt"), prt.get_attr("x"), None, prt.get_attr("z"))
        prt.coal_log_enable(4096)
    opts = lgrngn.opts_t()
    opts.cond = False
    for it in range(2):
        ring.step(opts, th.copy(), rv.copy(), rhod.copy(), **Cc)
    for prt in ring.prts:
        assert prt.opts_init.bcond_lft == 1 and prt.opts_init.bcond_rgt == 1, "a slab with neighbours on both sides"
        en, cap, r_min, held, seen, launches = prt.coal_log_info()
        assert en and launches == 2 and held == seen > 0
        ev = prt.coal_log()
        CL.assert_key_unique(ev)
        assert (ev["cell"] < 6 * 5).all() and (ev["slot_d"] != ev["slot_r"]).all() and (ev["n_d"] >= ev["n_r"]).all() and (ev["rw2_new"] > ev["rw2_r"]).all()


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_a_restored_snapshot_has_the_log_disabled_and_the_run_goes_on(real_t):
    prt, F = production(real_t, (1 << 14, 0.), steps=2)
    blob = prt.snapshot()
    assert prt.coal_log_info()[0] is True, "taking a snapshot leaves the log as it is"
    twin = h.hip_particles(production_case(real_t)["oi"], real_t)
    twin.coal_log_enable(64)                                            # (enabled before the load: a restored object starts disabled all the same)
    twin.restore(blob)
    assert twin.coal_log_info() == (False, 0, 0., 0, 0, 0)
    with pytest.raises(RuntimeError, match="not enabled"):
        twin.coal_log()
    for p in (prt, twin):
        for _ in range(2):
            step(p, F)
    for nm in ("raw_n", "raw_rw2", "raw_rd3", "raw_vt"):
        get = (lambda p: p.state_u64(nm)) if nm == "raw_n" else (lambda p: CL.bits(p.state_real(nm)))
        assert np.array_equal(get(prt), get(twin)), nm
    assert prt.coal_log_info()[5] == 4 and prt.coal_log_info()[4] > 0


def test_a_parcel_logs_with_cell_0():
    oi = lgrngn.opts_init_t()
    oi.dt, oi.sd_conc, oi.n_sd_max = 1., 64, 64
    oi.dry_distros = {(1e-10, 0.): lgrngn.expvolume(20e-6, 2 ** 30)}
    oi.kernel, oi.terminal_velocity, oi.sedi_switch = lgrngn.kernel_t.geometric, lgrngn.vt_t.beard77fast, False
    prt = h.hip_particles(oi)
    prt.init(np.array([300.]), np.array([.01]), np.array([1.1]))
    prt.coal_log_enable(256)
    opts = coal_only()
    for _ in range(3):
        prt.step_sync(opts, np.array([300.]), np.array([.01]), np.array([1.1]))
        prt.step_async(opts)
    ev = prt.coal_log()
    assert len(ev["cell"]) > 0 and (ev["cell"] == 0).all() and set(ev["launch"].tolist()) <= {0., 1., 2.}
    CL.assert_key_unique(ev)
