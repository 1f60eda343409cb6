"""The budget of tracked super-droplets (include/lcx_track_budget.h) on the device, in double and float, in the default arithmetic and
with strict_fp = 1, against tests/_track_budget_reference.py (numpy long double over raw states read around each pass).

1. Condensation alone: everything tracked, four steps, the fused and the per-particle substeps, and a box with RH on both sides of 1.
2. Coalescence alone: gains, gives and used-up donors (cells of equal multiplicity), per step and in total.
3. Everything on, sstp_coal 1 and 3, droplets leaving through the bottom: the closure between consecutive samples.
4. Through what moves storage: deaths, compaction, re-ordering, a source, recycling; `scans` rises only where storage was permuted.
5. Nothing else moves: the whole state after every step, the snapshot; a restored object reports the budget disabled.
6. Launch counts.
7. Rows and reading.  8. Every error text, refusals, a 0-D parcel with coalescence.

Bars: the three integer fields exactly; a sum of K terms to (K + 8) 2^-52 S, S the sum of c(w1) + c(w0) (of d1 + d0) over the terms
(_track_budget_reference.py derives it).  In the closures of 3 and 4 the samples and one raw state behind step_sync give the values
around condensation and around ALL coalescence substeps of a step; coalescence never shrinks a droplet, so the sum over the two spans
is a LOWER bound of S (it is S where one substep changed the droplet) and the bar that the tests use is no wider than the stated one."""
import ctypes as C

import numpy as np
import pytest

import _harness as h
import _track_budget_reference as B
import _track_reference as TR
import test_hip_chemistry as THC
import test_hip_move_rates as TMV
import test_hip_track as THT
import test_oracle_cond as TOC
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

LD = np.longdouble
REALS, REAL_IDS = THT.REALS, THT.REAL_IDS
STRICT, STRICT_IDS = [False, True], ["default", "strict_fp"]
NF = len(B.FIELDS)


def reset_particles(prt, dims, mult):
    """the droplets as they are stored, with other multiplicities (every mark is emptied: call it ahead of the selection)"""
    st = TR.raw_state(prt)
    pos = dict(x=st["x"], z=st["z"])
    if dims == 3:
        pos["y"] = st["y"]
    prt.set_particles(n=mult(st), rd3=st["rd3"], rw2=st["rw2"], kpa=st["kappa"], vt=st["vt"], **pos)


def track_everything(prt, dims, budget=True, capacity=8, mult=None):
    """kills five droplets in the middle of the storage (the tracked set is then no multiple of 64), marks all others"""
    def kill(st):
        n = (mult(st) if mult else st["n"]).copy()
        n[np.arange(3, n.size, n.size // 5)[:5]] = 0
        return n
    reset_particles(prt, dims, kill)
    n_alive = int((prt.state_u64("raw_n") > 0).sum())
    prt.track_enable(n_alive + 100, capacity=capacity)
    if budget:
        prt.track_budget_enable()
    assert prt.track_select([("all",)]) == n_alive and n_alive % 64 != 0 and n_alive > 256
    return n_alive


def sync(prt, fields, opts):
    th, rv, rhod, Cc = fields
    prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})


def some_opts(**kw):
    o = lgrngn.opts_t()
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


# ---------------------------------------------------------------------------------------------------- 1. condensation alone
COND = {"sstp1": (2, dict(sstp_cond=1)), "sstp3": (3, dict(sstp_cond=3)), "exact2": (2, dict(sstp_cond=2, exact_sstp_cond=True)), "crafted": (3, {})}


@pytest.mark.parametrize("case", list(COND))
@pytest.mark.parametrize("strict", STRICT, ids=STRICT_IDS)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_condensation_alone(real_t, strict, case):
    dims, kw = COND[case]
    prt, fields, oi = THT.rainy(real_t, dims, 8 if dims == 2 else 6, strict=strict, **kw)
    h.assert_mode(prt, strict_fp=strict)
    if case == "crafted":                                                     # RH 0.80 .. 1.03 by level: droplets grow above, evaporate below
        (th0, rv0), (th1, rv1), rhod, Cc = TOC.crafted_fields(oi, real_t, .80, 1.03, 3)
        fields = (th1, rv1, rhod, Cc)
    nt = track_everything(prt, dims)
    opts = some_opts(coal=False, adve=False, sedi=False)
    ref = B.Budget()
    for s in range(4):
        before = B.raw(prt)
        sync(prt, fields, opts)
        ref.add("cond", before, B.raw(prt), nt)
        prt.step_async(opts)
    bud = prt.track_budget()
    now = bud["now"]
    worst = B.assert_matches(now, ref.snapshot(), (real_t.__name__, strict, case))
    terms = int(ref.K["cond_dr3"].sum())
    print(real_t.__name__, STRICT_IDS[strict], case, "tracked", nt, "terms", terms, "worst error / bar %.3f" % worst)
    assert terms > 2 * nt, "most droplets changed in most passes"
    assert prt.track_budget_info() == dict(enabled=1, cond_passes=4, chem_passes=0, coal_passes=0)
    assert all((now[f] == 0).all() for f in B.FIELDS[1:]), "every other field is exactly 0"
    assert all(bud[f].shape == (0, nt) for f in B.FIELDS), "no sample was taken"
    if case == "crafted":
        assert (now["cond_dr3"] > 0).sum() > 50 and (now["cond_dr3"] < 0).sum() > 50, "terms of both signs"


# ---------------------------------------------------------------------------------------------------- 2. coalescence alone
@pytest.mark.parametrize("dims", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("strict", STRICT, ids=STRICT_IDS)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_coalescence_alone(real_t, strict, dims):
    prt, fields, oi = THT.rainy(real_t, dims, 8 if dims == 2 else 6, strict=strict)
    h.assert_mode(prt, strict_fp=strict)

    def equal_in_every_third_cell(st):                                        # there every collision uses up its donor
        n = st["n"].copy()
        n[st["cell"] % 3 == 0] = 400000
        return n
    nt = track_everything(prt, dims, mult=equal_in_every_third_cell)
    opts = some_opts(cond=False, adve=False, sedi=False)                      # nothing leaves the box
    ref, snaps = B.Budget(), []
    for s in range(6):
        sync(prt, fields, opts)
        before = B.raw(prt)
        prt.step_async(opts)
        ref.add("coal", before, B.raw(prt), nt)
        prt.track_sample()
        snaps.append(ref.snapshot())
    bud = prt.track_budget()
    tag = (real_t.__name__, strict, dims)
    worst = max(B.assert_matches({f: bud[f][s] for f in B.FIELDS}, snaps[s], tag + ("row", s)) for s in range(6))
    B.assert_matches(bud["now"], snaps[-1], tag + ("now",))
    now = bud["now"]
    gains, gives = int(now["coal_gains"].sum()), int(now["coal_gives"].sum())
    print(real_t.__name__, STRICT_IDS[strict], dims, "tracked", nt, "gains", gains, "gives", gives, "used-up donors", ref.used_up, "worst error / bar %.3f" % worst)
    assert gains >= 20 and gives >= 20 and ref.used_up >= 1
    info = prt.track_budget_info()
    assert info == dict(enabled=1, cond_passes=0, chem_passes=0, coal_passes=6)
    assert (now["coal_gains"] + now["coal_gives"] <= info["coal_passes"]).all()
    assert (now["cond_dr3"] == 0).all() and (now["chem_drd3"] == 0).all()
    rows = {f: np.concatenate([np.zeros((1, nt)), bud[f]]) for f in ("coal_gains", "coal_gives")}
    dg, dv = np.diff(rows["coal_gains"], axis=0), np.diff(rows["coal_gives"], axis=0)
    assert ((dg >= 0) & (dv >= 0) & (dg + dv <= 1)).all(), "one pair per pass at most: no index gains and gives in one step"


# ---------------------------------------------------------------------------------------------------- 3. and 4.: the closure
def closure(rec, bud, mids, s, sstp_coal, exact_n, tag):
    """between the samples s - 1 and s, with mids = B.values behind the step_sync in between.  Returns (alive at both, left out, the
    worst error in units of the bar)."""
    n0, n1 = rec["n"][s - 1], rec["n"][s]
    both, left_out = (n0 > 0) & (n1 > 0), (n0 > 0) & (n1 == 0)
    d = {f: bud[f][s].astype(LD) - bud[f][s - 1].astype(LD) for f in B.FIELDS}
    known = ~np.isnan(bud["coal_dn"][s - 1])                                  # (NaN: selected after that sample)
    assert known[n0 > 0].all() and not np.isnan(bud["coal_dn"][s][known]).any()
    for f in B.INT_FIELDS:
        assert (d[f][known] >= 0).all() and np.array_equal(bud[f][s][known], np.floor(bud[f][s][known])), (tag, s, f, "non-decreasing whole numbers")
    gone = known & (n0 == 0)
    for f in B.FIELDS:
        assert (d[f][gone] == 0).all(), (tag, s, f, "an index without a droplet keeps its values")
    nb, wb, db = (np.concatenate([v, np.zeros(n0.size - v.size, dtype=v.dtype)]) for v in mids)          # (indices selected later: absent)
    assert (nb[both] > 0).all()
    wa, wc, da, dc = rec["rw2"][s - 1][both], rec["rw2"][s][both], rec["rd3"][s - 1][both], rec["rd3"][s][both]
    wb, db = wb[both], db[both]
    assert np.array_equal(da, db), "without chemistry step_sync leaves rd3 alone"
    worst = 0.
    # rw2: one condensation pass and sstp_coal coalescence passes
    S = np.where(wa != wb, B.cube(wa) + B.cube(wb), 0) + np.where(wb != wc, B.cube(wb) + B.cube(wc), 0)
    err, lim = np.abs((B.cube(wc) - B.cube(wa)) - (d["cond_dr3"] + d["coal_dr3"])[both]), B.bar(1 + sstp_coal, S)
    assert (err <= lim).all(), (tag, s, "rw2 closure", np.flatnonzero(err > lim)[:8], err[err > lim][:4], lim[err > lim][:4])
    if (S > 0).any():
        worst = max(worst, float((err[S > 0] / lim[S > 0]).max()))
    # rd3: the coalescence passes (no chemistry here)
    S = np.where(db != dc, db.astype(LD) + dc.astype(LD), 0)
    err, lim = np.abs((dc.astype(LD) - da.astype(LD)) - (d["coal_drd3"] + d["chem_drd3"])[both]), B.bar(sstp_coal, S)
    assert (err <= lim).all(), (tag, s, "rd3 closure", np.flatnonzero(err > lim)[:8], err[err > lim][:4], lim[err > lim][:4])
    if (S > 0).any():
        worst = max(worst, float((err[S > 0] / lim[S > 0]).max()))
    if exact_n:
        assert np.array_equal((n0 - n1)[both].astype(LD), d["coal_dn"][both]), (tag, s, "n closure")
    events = (d["coal_gains"] + d["coal_gives"])[known]
    assert (events <= sstp_coal).all(), (tag, s, "a droplet is in one pair per pass at most")
    return both, left_out, worst


@pytest.mark.parametrize("sstp_coal", [1, 3])
@pytest.mark.parametrize("dims", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("strict", STRICT, ids=STRICT_IDS)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_everything_on_closes_between_samples(real_t, strict, dims, sstp_coal):
    prt, fields, oi = THT.rainy(real_t, dims, 8 if dims == 2 else 6, strict=strict, sstp_coal=sstp_coal)
    h.assert_mode(prt, strict_fp=strict)
    nt = track_everything(prt, dims)
    opts = lgrngn.opts_t()                                                    # condensation, coalescence, advection, sedimentation
    prt.track_sample()
    mids = []
    for s in range(6):
        sync(prt, fields, opts)
        mids.append(B.values(B.raw(prt), nt))
        prt.step_async(opts)
        prt.track_sample()
    rec, bud = prt.track(), prt.track_budget()
    assert rec["n"].shape == (7, nt) and all(bud[f].shape == (7, nt) for f in B.FIELDS)
    assert all((bud[f][0] == 0).all() for f in B.FIELDS), "selected, nothing has passed yet"
    tag, worst, left, closed = (real_t.__name__, strict, dims, sstp_coal), 0., 0, 0
    for s in range(1, 7):
        both, left_out, w = closure(rec, bud, mids[s - 1], s, sstp_coal, True, tag)
        worst, left, closed = max(worst, w), left + int(left_out.sum()), closed + int(both.sum())
    info = prt.track_budget_info()
    now = bud["now"]
    print(real_t.__name__, STRICT_IDS[strict], dims, "sstp_coal", sstp_coal, "tracked", nt, "left out", left, "closed (index, interval) pairs", closed,
          "gains", int(now["coal_gains"].sum()), "gives", int(now["coal_gives"].sum()), "worst error / bar %.3f" % worst)
    assert info == dict(enabled=1, cond_passes=6, chem_passes=0, coal_passes=6 * sstp_coal)
    assert 0 < left <= nt // 2, "some droplets leave through the bottom (left out of the closure from then on), at most half of the set"
    assert (rec["n"][-1] > 0).sum() > 0 and now["coal_gains"].sum() > 0 and (now["cond_dr3"] != 0).sum() > nt // 4
    assert all(np.array_equal(now[f], bud[f][-1]) for f in B.FIELDS), "nothing has passed since the last sample"


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_through_everything_that_moves_storage(real_t):
    """the scenario of test_hip_track.py's identity test with the budget on throughout.  A checkpoint is taken right behind every sample,
    from raw_ getters alone: `scans` and the tags per storage slot.  Between two checkpoints lie the compaction that the test's own
    reads of "T", "RH" and "rv" cause, a step and a sample; the tags show whether storage was permuted or rewritten in between."""
    n, key = 6, (.61, 0.)
    prt, fields, oi = THT.rainy(real_t, 2, n, per_cell=32, cz=-.6, dbg_flags=int(lgrngn.dbg.TAG), reorder_every=2, src_type=lgrngn.src_t.simple,
                                src_x0=0., src_x1=float(n), src_z0=2., src_z1=4., n_sd_max=4096)
    prt.track_enable(256, capacity=16)
    prt.track_budget_enable()
    n_bot = prt.track_select([("all",)], box=(0., n, 0., 0., 0., 1.), max_count=40)
    n_top = prt.track_select([("all",)], box=(0., n, 0., 0., n - 1., n), max_count=40)
    assert n_bot > 30 and n_top > 30
    opts = lgrngn.opts_t()
    opts.src = True
    opts.src_dry_distros = {key: (h.lognormal_fn(.05e-6, 1.5, 60e6), 8, 2)}
    n_tr = n_bot + n_top
    prt.track_sample()
    check = lambda: (prt.track_info()["scans"], prt.state_real("raw_tag"))
    scans, tags = check()
    st = TR.raw_state(prt)
    n_tags, mids, n_at, permuted_n, newcomers = int(tags.max()) + 1, [], [n_tr], 0, 0
    for s in range(5):
        if s == 3:                                                            # the donors of step 4's recycling
            big = np.argsort(-prt.state_u64("raw_n").astype(np.int64), kind="stable")[:12]
            n_tr += prt.track_select_slots(big)
            assert n_tr > n_bot + n_top
            opts.rcyc, opts.src = True, False
        sync(prt, fields, opts)
        mids.append(B.values(B.raw(prt), n_tr))
        prt.step_async(opts)
        prt.track_sample()
        scans1, tags1 = check()
        m = min(tags.size, tags1.size)
        permuted = tags1.size < tags.size or not np.array_equal(tags[:m], tags1[:m])
        permuted_n += int(permuted)
        assert (scans1 > scans) == permuted and scans1 - scans <= 4, ("step", s, "scans", scans, scans1, "permuted", permuted)
        scans, tags = scans1, tags1
        st = TR.raw_state(prt)                                                # (compacts; read for the newcomers and for step 3's donors)
        new = tags1 >= n_tags
        newcomers += int(new.sum())
        assert (st["track"][new] == 0).all(), "a newcomer has no mark, so no accumulators"
        n_tags = max(n_tags, int(tags1.max()) + 1)
        n_at.append(n_tr)
    rec, bud = prt.track(), prt.track_budget()
    assert prt.track_info()["n_tracked"] == n_tr and rec["n"].shape == (6, n_tr)
    assert np.isnan(bud["coal_dn"][:4, n_bot + n_top:]).all() and not np.isnan(bud["coal_dn"][4:]).any(), "NaN in the rows ahead of a selection"
    worst = closed = 0
    for s in range(1, 6):
        both, left_out, w = closure(rec, bud, mids[s - 1], s, 1, s < 4, (real_t.__name__, "storage"))        # (steps 4 and 5 recycle: that halves donors)
        worst, closed = max(worst, w), closed + int(both.sum())
    print(real_t.__name__, "tracked", n_tr, "closed", closed, "permuted intervals", permuted_n, "scans", scans, "newcomers", newcomers, "worst error / bar %.3f" % worst)
    assert newcomers >= 96 and permuted_n >= 3 and closed > 100
    assert (rec["n"][-1][:n_bot] == 0).all() and (rec["n"][0][:n_bot] > 0).any(), "the lowest level's droplets have left"
    died = np.flatnonzero((rec["n"][0][:n_bot] > 0) & (rec["n"][2][:n_bot] == 0))
    assert died.size > 10
    for f in B.FIELDS:
        assert all(np.array_equal(bud[f][s][died], bud[f][2][died]) for s in range(3, 6)), "a dead droplet's index keeps its last values in every later row"


# ---------------------------------------------------------------------------------------------------- 5. nothing else moves
_twins = {}


def twin_runs(real_t, case):
    """two objects from the same options and seed, both tracking with every = 1, one with the budget: five steps each, made once per
    parameter set; only results are kept"""
    key = (real_t.__name__, case)
    if key in _twins:
        return _twins[key]
    res, blobs, extra = [], [], {}
    for budget in (True, False):
        prt, fields, oi = THT.make_case(real_t, case)
        h.assert_mode(prt, strict_fp=(case == "strict"))
        prt.track_enable(500, capacity=8, every=1)
        assert prt.track_select([("all",)], max_count=300) > 100
        if budget:
            prt.track_budget_enable()
        opts, out = lgrngn.opts_t(), []
        for s in range(5):
            THT.step(prt, fields, opts)
            out.append(THT.whole_state(prt))
        res.append(out)
        blobs.append(bytes(prt.snapshot()))
        if budget:
            extra = dict(info=prt.track_budget_info(), bud=prt.track_budget(), track=prt.track_info(), oi=oi)
    _twins[key] = (res, blobs, extra)
    return _twins[key]


@pytest.mark.parametrize("case", THT.CASES)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_nothing_else_moves(real_t, case):
    res, blobs, extra = twin_runs(real_t, case)
    for s in range(5):
        assert set(res[0][s]) == set(res[1][s])
        for nm in res[0][s]:
            assert np.array_equal(res[0][s][nm], res[1][s][nm]), (case, "step", s, nm)
    assert blobs[0] == blobs[1], "the snapshot of an object with the budget is that of the same run with tracking alone, byte for byte"
    info, bud = extra["info"], extra["bud"]
    assert info["enabled"] == 1 and info["cond_passes"] == 5 and info["coal_passes"] == 5 and extra["track"]["n_samples"] == 5
    assert (bud["now"]["cond_dr3"] != 0).sum() > 50, "the budget did run"
    if case == "colliding":
        assert bud["now"]["coal_gains"].sum() > 0
    twin = h.hip_particles(extra["oi"], real_t)
    twin.track_enable(16)
    twin.track_budget_enable()                                                # (enabled before the load: a restored object has none all the same)
    twin.restore(np.frombuffer(blobs[0], dtype=np.uint8))
    assert twin.track_budget_info() == dict(enabled=0, cond_passes=0, chem_passes=0, coal_passes=0) and twin.track_info()["enabled"] == 0
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: track budget: enable while tracking is not enabled"):
        twin.track_budget_enable()


# ---------------------------------------------------------------------------------------------------- 6. launch counts
def counted_steps(prt, fields, steps=3):
    """per step: (launches of step_sync, of step_async, scans of step_sync, of step_async)"""
    opts, out = lgrngn.opts_t(), []
    L = lambda: int(prt.state_u64("raw_launches")[0])
    Sc = lambda: prt.track_info()["scans"]
    for s in range(steps):
        n0, s0 = L(), Sc()
        sync(prt, fields, opts)
        n1, s1 = L(), Sc()
        prt.step_async(opts)
        out.append((n1 - n0, L() - n1, s1 - s0, Sc() - s1))
    return out


@pytest.mark.parametrize("sstp_cond, sstp_coal", [(1, 1), (3, 1), (1, 3)])
def test_launch_counts(sstp_cond, sstp_coal):
    def make(budget, select=True, disable=False, track=True):
        prt, fields, _ = TMV.rainy_box(np.float64, None, sstp_cond=sstp_cond, sstp_coal=sstp_coal)
        if track:
            prt.track_enable(1000)
            if select:
                assert prt.track_select([("rng", "wet", 10e-6, 1.)]) > 100
        if budget:
            prt.track_budget_enable()
        if disable:
            prt.track_budget_disable()
        return counted_steps(prt, fields)
    plain, on, empty, empty_plain, gone = make(False), make(True), make(True, select=False), make(False, select=False), make(True, disable=True)
    print("sstp_cond", sstp_cond, "sstp_coal", sstp_coal, "(sync, async, scans in sync, scans in async) per step: tracking alone", plain, "budget on", on,
          "budget on, nothing tracked", empty, "enabled then disabled", gone)
    assert all(p[2] == 0 and p[3] == 0 for p in plain), "tracking without a sample scans nothing"
    for (s_on, a_on, sc_s, sc_a), (s_off, a_off, _, _) in zip(on, plain):
        assert 0 < s_on - s_off - sc_s <= 2, "two launches per condensation pass, and the scan that a sample would owe as well"
        assert 0 < a_on - a_off - sc_a <= sstp_coal + 1, "one launch ahead of the coalescence substeps, one behind each"
    assert sum(p[2] + p[3] for p in on) >= 1
    assert [p[:2] for p in empty] == [p[:2] for p in empty_plain] and all(p[2] == 0 and p[3] == 0 for p in empty), "nothing tracked: no launch more"
    assert gone == plain, "enabled then disabled: what a never-enabled budget launches"


def test_launch_counts_of_a_sample_and_of_chemistry():
    # a sample: one launch more
    per = []
    for budget in (False, True):
        prt, fields, _ = TMV.rainy_box(np.float64, None)
        prt.track_enable(1000)
        assert prt.track_select([("rng", "wet", 10e-6, 1.)]) > 100
        if budget:
            prt.track_budget_enable()
        prt.track_sample()                                                    # (the scan that enable owes)
        n0 = int(prt.state_u64("raw_launches")[0])
        prt.track_sample()
        per.append(int(prt.state_u64("raw_launches")[0]) - n0)
    print("launches of a sample: tracking alone", per[0], "with the budget", per[1])
    assert per == [1, 2]
    # chemistry: two launches more per chemistry pass, and CHEM_DRD3 is what the raw states around the pass say
    counts, kept = [], None
    for budget in (False, True):
        box = THC.Box((3, 4), 24, np.float64, cond_steps=2, mode="fast")
        p = box.p
        p.track_enable(400)
        nt = p.track_select([("all",)])
        assert nt > 250
        if budget:
            p.track_budget_enable()
        o = box.opts(cond=True, chem_dsl=True, chem_dsc=True, chem_rct=True)
        ref, per = B.Budget(), []
        for s in range(3):
            before = B.raw(p)
            n0, s0 = int(p.state_u64("raw_launches")[0]), p.track_info()["scans"]
            box.step(o, async_=False)
            per.append((int(p.state_u64("raw_launches")[0]) - n0, p.track_info()["scans"] - s0))
            after = B.raw(p)
            ref.grow(nt)                                                      # condensation and chemistry in one call: rw2 is condensation's, rd3 chemistry's
            ref.add("cond", before, after, nt)
            ref.add("chem", before, after, nt)
            p.step_async(o)
        counts.append(per)
        if budget:
            kept = (p.track_budget()["now"], ref.snapshot(), p.track_budget_info())
    print("chemistry, launches of step_sync (and scans): tracking alone", counts[0], "with the budget", counts[1])
    for (on, sc), (off, _) in zip(counts[1], counts[0]):
        assert 0 < on - off - sc <= 4
    now, snap, info = kept
    assert info == dict(enabled=1, cond_passes=3, chem_passes=3, coal_passes=0)
    worst = B.assert_matches(now, snap, "chemistry")
    print("chemistry: indices whose rd3 changed", int((now["chem_drd3"] != 0).sum()), "worst error / bar %.3f" % worst)
    assert (now["chem_drd3"] != 0).sum() > 0 and (now["cond_dr3"] != 0).sum() > 50


# ---------------------------------------------------------------------------------------------------- 7. rows and reading
def test_rows_and_reading():
    oi = h.api_default_opts(h.box_opts(4, 0, 4, 16))
    th, rv, rhod, Cc = h.box_fields(oi)
    fields = (th, rv, rhod, Cc)
    prt = h.hip_particles(oi, np.float64)
    prt.track_enable(100, capacity=3, every=2)
    prt.track_budget_enable()                                                 # before init()
    assert prt.track_budget_info() == dict(enabled=1, cond_passes=0, chem_passes=0, coal_passes=0)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    opts = some_opts(coal=False, sedi=False)
    assert prt.track_select_slots(np.arange(0, 200, 5)) == 40
    ref, snaps = B.Budget(), {}
    for s in range(10):
        before = B.raw(prt)
        sync(prt, fields, opts)
        ref.add("cond", before, B.raw(prt), 40)
        prt.step_async(opts)
        snaps[s + 1] = ref.snapshot()
    info = prt.track_info()
    assert (info["n_samples"], info["dropped"]) == (3, 2), "a full buffer drops the samples and their rows"
    bud = prt.track_budget()
    assert all(bud[f].shape == (3, 40) for f in B.FIELDS)
    for i, stp in enumerate((2, 4, 6)):
        B.assert_matches({f: bud[f][i] for f in B.FIELDS}, snaps[stp], ("automatic row", stp))
    B.assert_matches(bud["now"], snaps[10], "now")
    assert (bud["now"]["cond_dr3"] != 0).sum() > 30 and not np.array_equal(bud["cond_dr3"][0], bud["cond_dr3"][2])
    prt.track(reset=True)
    again = prt.track_budget()
    assert all(again[f].shape == (0, 40) for f in B.FIELDS) and all(np.array_equal(again["now"][f], bud["now"][f]) for f in B.FIELDS), "reset empties the rows, not the accumulators"
    prt.track_sample()
    assert prt.track_select_slots(np.arange(1, 200, 5)) == 40                 # selected between two samples
    for s in range(10, 12):
        before = B.raw(prt)
        sync(prt, fields, opts)
        ref.add("cond", before, B.raw(prt), 80)
        prt.step_async(opts)                                                  # step 12 ends in a sample
    bud = prt.track_budget()
    assert all(bud[f].shape == (2, 80) for f in B.FIELDS)
    for f in B.FIELDS:
        assert np.isnan(bud[f][0, 40:]).all() and not np.isnan(bud[f][0, :40]).any() and not np.isnan(bud[f][1]).any(), "NaN in the row ahead of the selection"
    B.assert_matches({f: bud[f][0, :40] for f in B.FIELDS}, {k: {f: v[:40] for f, v in t.items()} for k, t in snaps[10].items()}, "the row of step 10")
    B.assert_matches({f: bud[f][1] for f in B.FIELDS}, ref.snapshot(), "the row of step 12: zeros from the selection on, then two passes")
    assert (ref.K["cond_dr3"][40:] <= 2).all() and ref.K["cond_dr3"][40:].sum() > 40 and ref.K["cond_dr3"][:40].sum() > 400
    # track_enable on an enabled object starts over and switches the budget off
    prt.track_enable(8)
    assert prt.track_budget_info() == dict(enabled=0, cond_passes=0, chem_passes=0, coal_passes=0)
    # one tracked droplet
    prt.track_budget_enable()
    assert prt.track_select_slots([7]) == 1
    before = B.raw(prt)
    sync(prt, fields, opts)
    one = B.Budget()
    one.add("cond", before, B.raw(prt), 1)
    prt.step_async(opts)
    prt.track_sample()
    bud = prt.track_budget()
    assert bud["cond_dr3"].shape == (1, 1) and bud["now"]["cond_dr3"].shape == (1,) and bud["now"]["cond_dr3"][0] != 0
    B.assert_matches(bud["now"], one.snapshot(), "one droplet")
    # disable and enable again: zero, and the samples held read NaN
    prt.track_budget_disable()
    prt.track_budget_enable()
    bud = prt.track_budget()
    assert np.isnan(bud["cond_dr3"]).all() and bud["cond_dr3"].shape == (1, 1) and all((bud["now"][f] == 0).all() for f in B.FIELDS)


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_device_output_with_padded_strides(real_t):
    import torch
    prt, fields, oi = THT.rainy(real_t, 2, 6)
    prt.track_enable(64, capacity=4)
    prt.track_budget_enable()
    nt = prt.track_select([("rng", "wet", THT.F32(15e-6), 1.)], max_count=50)
    assert nt > 20
    opts = lgrngn.opts_t()
    for s in range(3):
        THT.step(prt, fields, opts)
        prt.track_sample()
    host = prt.track_budget()
    fs, ss = nt + 3, NF * (nt + 3) + 5
    buf = torch.full((3 * ss,), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    got = prt.track_budget(out=lgrngn.DeviceArray(buf.data_ptr(), (3, NF, nt), (ss, fs, 1)))
    assert set(got) == {"now"} and all(np.array_equal(got["now"][f], host["now"][f]) for f in B.FIELDS)
    flat = buf.cpu().numpy()
    seen = np.zeros(flat.size, dtype=bool)
    for s in range(3):
        for f, nm in enumerate(B.FIELDS):
            lo = s * ss + f * fs
            assert np.array_equal(flat[lo:lo + nt], host[nm][s], equal_nan=True), (s, nm)
            seen[lo:lo + nt] = True
    assert (flat[~seen] == -1).all(), "the padding is untouched"
    assert (host["cond_dr3"][-1] != 0).any()
    # the accumulators on the device as well, through the C entry point
    now = torch.full((NF * fs,), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = prt._f("track_budget_read")(prt._h, None, C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), None, C.c_void_p(now.data_ptr()), C.c_size_t(fs), C.c_int(1))
    assert rc == 0
    flat = now.cpu().numpy().reshape(NF, fs)
    assert all(np.array_equal(flat[f, :nt], host["now"][nm]) for f, nm in enumerate(B.FIELDS)) and (flat[:, nt:] == -1).all()


# ---------------------------------------------------------------------------------------------------- 8. errors, refusals, a parcel
def test_every_error_text():
    oi = h.api_default_opts(h.box_opts(4, 0, 4, 16))
    th, rv, rhod, Cc = h.box_fields(oi)
    prt = h.hip_particles(oi, np.float64)
    f = lambda name: getattr(prt._lib, "lcx_track_budget_" + name)
    last = prt._f("last_error")
    last.restype = C.c_char_p
    sz, i32 = C.c_size_t, C.c_int
    refused = lambda rc, text: (rc == 1 and last().decode() == text) or pytest.fail("%r, not %r" % (last().decode(), text))
    got, out, now = sz(), np.zeros((4, NF, 8)), np.zeros((NF, 8))
    outp, nowp = C.c_void_p(out.ctypes.data), C.c_void_p(now.ctypes.data)
    read = lambda o, ss, fs, cap, nw, ns: f("read")(prt._h, o, sz(ss), sz(fs), sz(cap), C.byref(got), nw, sz(ns), i32(0))
    assert prt.track_budget_info() == dict(enabled=0, cond_passes=0, chem_passes=0, coal_passes=0)
    refused(f("enable")(prt._h), "libcloudph++: track budget: enable while tracking is not enabled (lcx_track_enable)")
    prt.track_enable(8, capacity=4)
    refused(f("disable")(prt._h), "libcloudph++: track budget: disable while the budget is not enabled (lcx_track_budget_enable)")
    refused(read(outp, NF * 8, 8, 4, nowp, 8), "libcloudph++: track budget: read while the budget is not enabled (lcx_track_budget_enable)")
    assert prt.track_budget_info()["enabled"] == 0
    assert f("enable")(prt._h) == 0
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    assert prt.track_select_slots([0, 1, 2]) == 3
    prt.track_sample()
    prt.track_sample()
    refused(read(outp, NF * 8, 2, 4, nowp, 8), "libcloudph++: track budget: field_stride (2) < n_tracked (3)")
    refused(read(outp, NF * 8, 8, 4, nowp, 2), "libcloudph++: track budget: now_stride (2) < n_tracked (3)")
    refused(read(outp, NF * 8 - 1, 8, 4, nowp, 8), "libcloudph++: track budget: sample_stride (%d) < %d * field_stride (8)" % (NF * 8 - 1, NF))
    refused(read(outp, NF * 8, 8, 1, nowp, 8), "libcloudph++: track budget: cap_samples (1) < the samples held (2)")
    refused(read(None, NF * 8, 8, 4, None, 8), "libcloudph++: track budget: out == NULL and now == NULL")
    assert prt.track_budget_info()["enabled"] == 1 and (out == 0).all() and (now == 0).all(), "a failed call leaves everything as it was"
    out[:], now[:] = -1, -1
    assert read(outp, NF * 8, 8, 4, nowp, 8) == 0 and got.value == 2
    assert (out[:2, :, :3] == 0).all() and (out[:2, :, 3:] == -1).all() and (out[2:] == -1).all() and (now[:, :3] == 0).all() and (now[:, 3:] == -1).all()
    assert read(None, 0, 0, 0, nowp, 3) == 0 and read(outp, NF * 3, 3, 2, None, 0) == 0, "either may be NULL"
    prt.track_disable()
    assert prt.track_budget_info()["enabled"] == 0, "lcx_track_disable switches the budget off"


def test_a_multi_device_object_is_refused(monkeypatch):
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = h.box_opts(4, 4, 4, 16)
    oi.dev_count = 2
    prt = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert prt.dev_count == 2
    for call in (prt.track_budget_enable, prt.track_budget_disable, prt.track_budget_info, prt.track_budget):
        with pytest.raises(RuntimeError, match=r"libcloudph\+\+: track on a multi-device object is not built"):
            call()


def test_a_slab_with_neighbours_is_refused():
    oi = h.box_opts(4, 4, 4, 16)
    oi.bcond_lft = oi.bcond_rgt = 1
    prt = h.hip_particles(oi)
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: track on a decomposed domain is not built"):
        prt.track_budget_enable()
    assert prt.track_budget_info()["enabled"] == 0


def test_a_parcel_with_coalescence():
    oi = lgrngn.opts_init_t()
    oi.dt, oi.sd_conc, oi.n_sd_max = 1., 64, 64
    oi.dry_distros = {(.61, 0.): h.lgrngn_bimodal()}
    oi.sedi_switch = False
    oi.kernel, oi.terminal_velocity = lgrngn.kernel_t.geometric, lgrngn.vt_t.beard77fast
    prt = h.hip_particles(oi)
    prt.init(np.array([300.]), np.array([.010]), np.array([1.1]))
    prt.track_enable(64, capacity=4, every=1)
    prt.track_budget_enable()
    nt = prt.track_select([("all",)])
    assert nt > 32
    opts = some_opts(sedi=False, adve=False)
    ref = B.Budget()
    for s in range(3):
        before = B.raw(prt)
        prt.step_sync(opts, np.array([300.]), np.array([.012]), np.array([1.1]))
        mid = B.raw(prt)
        ref.add("cond", before, mid, nt)
        prt.step_async(opts)
        ref.add("coal", mid, B.raw(prt), nt)
    bud = prt.track_budget()
    assert prt.track_budget_info() == dict(enabled=1, cond_passes=3, chem_passes=0, coal_passes=3) and bud["cond_dr3"].shape == (3, nt)
    B.assert_matches(bud["now"], ref.snapshot(), "parcel")
    B.assert_matches({f: bud[f][-1] for f in B.FIELDS}, ref.snapshot(), "parcel, the last row")
    assert (bud["now"]["cond_dr3"] != 0).sum() > nt // 2
