"""Aqueous chemistry in the arithmetic a caller gets, from an object nobody has read, behind condensation and through coalescence.

tests/test_hip_chemistry.py holds the chemistry kernels to numpy restatements of the reference's formulas, always in the parity
arithmetic (strict_fp = 1) and always from an object that the test has just read -- i.e. compacted and freshly sorted.  This file uses
the same restatement (imported, not copied) where that file does not look:

A  every object here runs one of three arithmetic modes -- strict, toms (the API default: strict_fp = 0, cond_solver = 1) and fast
   (strict_fp = 0, cond_solver = 0, what bench.py runs) -- and what it runs is read back from it (h.assert_mode) after its first
   condensation step, kernel name included;
B  chem_step() entered straight after a step_async that moved, sedimented and coalesced droplets and left dead slots and an unfinished
   sort behind (the twin test);
C  which temperature chemistry sees when condensation runs in the same step_sync (the reference runs no hskpng_Tpr between the two);
D  the eight masses of each droplet through coalescence, not their totals;
E  ambient_chem as contiguous, strided and device arrays.

Bars are those of tests/test_hip_chemistry.py: rtol 1e-12 for a double object, for a float one four times the largest relative
difference of the restatement evaluated in float32 and in float64 on the same inputs (bar_for); per-cell sums relative to the sum of
the absolute terms (sum_bar).  The H+ root is held to the bisection's at TOL_ROOT; where dissolution runs ahead of the dissociation in
the same step of a FLOAT object the masses that the root is a function of carry the float bar already, so there the root's bar is
TOL_ROOT plus four times the relative difference of the bisection's roots on the float32 and the float64 restatement's masses.  What
follows the dissociation in a step (the oxidation reads H+) is restated from the library's own root, so that it keeps the closed-form
bars instead of inheriting the root finder's tolerance."""
import numpy as np
import pytest

import _harness as h
import test_hip_chemistry as c
from libcloudphxx_amd import lgrngn
from test_hip_chemistry import Box, MODES, NAMES, GASES, SP, REALS, TOL_ROOT, bar_for, both_classes, rel, sum_bar, substep

pytestmark = pytest.mark.gpu

MODE_NAMES = ["strict", "toms", "fast"]
DEAD = 0xFFFFFFFF


def kernel_of(mode, sstp_cond=1, exact=False):
    """the condensation kernel that an object of this mode launches (lgrngn.cond_kernel names)"""
    if exact and sstp_cond > 1:
        return "per_particle"
    if mode == "strict":
        return "strict"
    if sstp_cond > 1:
        return "substeps"
    return "fold_toms748" if mode == "toms" else "lean"


def check_mode(b):
    """A: the arithmetic, the solver and the kernel of the last condensation launch, read back from the object"""
    h.assert_mode(b.p, *MODES[b.mode], kernel=kernel_of(b.mode, int(b.oi.sstp_cond), bool(b.oi.exact_sstp_cond)))


def by_tag(p):
    tag = p.state_real("tag").astype(np.int64)
    order = np.argsort(tag, kind="stable")
    assert np.all(np.diff(tag[order]) > 0)                   # (unique: nothing recycles here)
    return tag[order], order


def eps_of(real_t):
    return float(np.finfo(real_t).eps)


# ------------------------------------------------------------------------------------------ one step of chemistry against the restatement
def measure(st, got, real_t, dsl, dsc, rct, dt=1.):
    """The figures of one step_sync of chemistry: `st` is the state that the step started from (masses, rd3, T ... in one droplet order,
    rw2 as the step's chemistry saw it), `got` the library's state after it in the same order (m, rd3, amb, flag).  Returns a list of
    (name, error, bar) and the selection's statistics; nothing is asserted here, so that a negative control can use it as well.
    st["T32"], if there: the temperature as the float32 restatement is to take it (where T itself is restated from th, it is evaluated
    in both precisions like the rest of the restatement)."""
    st32 = dict(st, T=st["T32"]) if "T32" in st else st
    figs = []
    is_f32 = np.dtype(real_t) == np.float32
    root_bar = TOL_ROOT
    H_lib = got["m"][c.H] if dsc else None
    if dsc:                                                 # the root by bisection, on the restatement's masses ahead of the dissociation
        r64, _, _, _, fl = substep(st, dt, dsl, True, False, np.float64)
        if is_f32 and dsl:
            r32, _, _, _, fl32 = substep(st32, dt, dsl, True, False, np.float32)
            ok = fl & fl32
            root_bar = TOL_ROOT + 4 * rel(r32[c.H][ok], r64[c.H][ok])
    info = {}
    m64, rd64, a64, _, flag = substep(st, dt, dsl, dsc, rct, np.float64, info=info, H_after_dsc=H_lib)
    m32, rd32, a32, _, flag32 = substep(st32, dt, dsl, dsc, rct, np.float32, H_after_dsc=H_lib)
    same = flag == flag32
    sel = same if is_f32 else np.ones(flag.shape, dtype=bool)
    stats = dict(left_out=float(np.mean(~same)), flag=flag, sel=sel)
    if dsc:
        figs.append(("H+ root", rel(got["m"][c.H][flag & sel], r64[c.H][flag & sel]), root_bar))
        # (the concentrated droplets keep the bits of their H+: nothing of a step changes it there)
        figs.append(("H+ kept", rel(got["m"][c.H][~flag & sel], np.asarray(st["m"][c.H], dtype=np.float64)[~flag & sel]), 0.))
    # (a bar per species, as in tests/test_hip_chemistry.py's case of the rate limiters: in float the O3 left by the oxidation is a
    # difference of nearly equal terms, whose bar would hide the other species behind it)
    for sp in range(8):
        if not (dsc and sp == c.H):
            figs.append((NAMES[sp], rel(got["m"][sp][sel], m64[sp][sel]), bar_for(real_t, [m32[sp][same]], [m64[sp][same]])))
    figs.append(("rd3", rel(got["rd3"][sel], rd64[sel]), bar_for(real_t, [rd32[same]], [rd64[same]])))
    stats["bars"] = {name: b_ for name, _, b_ in figs}
    stats["bar_min"] = min(b_ for _, _, b_ in figs if b_ > 0)
    stats["flag_agrees"] = bool(np.array_equal(got["flag"][sel], flag[sel]))
    if dsl:
        cnt_max = int(np.bincount(st["ijk"], minlength=st["T"].size).max())
        for g in GASES:
            scale = np.abs(st["amb"][g]) + info["abs_terms"][g]
            err = float(np.max(np.abs(got["amb"][g] - a64[g]) / scale))
            # (n (m_new - m_old) two roundings, the sum, four factors and the subtraction from c: tests/test_hip_chemistry.py, case 2)
            abar = 1e-12 if not is_f32 else max(sum_bar(real_t, cnt_max, 7), 4 * float(np.max(np.abs(a32[g].astype(np.float64) - a64[g]) / scale)))
            figs.append(("ambient " + NAMES[g], err, abar))
    return figs, stats


def worst(figs):
    return max((e / b_ if b_ > 0 else (np.inf if e > 0 else 0.)) for _, e, b_ in figs)


def hold(figs, what=""):
    for name, e, b_ in figs:
        print("%-24s %-14s error %.3e bar %.3e" % (what, name, e, b_))
    for name, e, b_ in figs:
        assert e <= b_, (what, name, e, b_)


def read(b, order=None):
    """the library's state in the order `order` of the droplets (default: storage order)"""
    s = b.state()
    s["flag"] = b.p.state_real("chem_flag") != 0
    if order is not None:
        for k_ in ("n", "ijk", "rw2", "rd3", "flag"):
            s[k_] = s[k_][order]
        s["m"] = [x[order] for x in s["m"]]
    return s


# ------------------------------------------------------------------------------------------ B: the twins
N_LOW_EVERY = 3           # every third droplet of the lowest row becomes a rain drop
RAIN_R, RAIN_N = 1e-3, 1000


def make_twin(mode, real_t, reorder_every, steps=4):
    """A 3 x 4 box of 32 per cell with the Courant numbers of h.box_fields: a condensation spin-up, then every third droplet of the lowest
    row is made a rain drop (1 mm at a multiplicity of 1000: it falls 6 m per step, collects cloud droplets on its way and weighs too
    little to disturb the cell's vapour), then `steps` steps of adve, sedi, coal, cond and the three chemistry processes.  Returns the
    box as its last step_async left it -- unread -- and the multiplicities by tag that the steps started from."""
    b = Box((3, 4), 32, real_t, mode=mode, courant=True, sedi_switch=True, coal_switch=True, dbg_flags=int(lgrngn.dbg.TAG),
            reorder_every=reorder_every, cond_steps=4)
    check_mode(b)
    s = b.state()
    x, z = b.p.state_real("x"), b.p.state_real("z")
    low = (z < 40.) & (np.arange(z.size) % N_LOW_EVERY == 0)
    n0 = np.where(low, float(RAIN_N), s["n"])
    b.p.set_particles(n0, s["rd3"], np.where(low, RAIN_R ** 2, s["rw2"]), b.p.state_real("kappa"), b.p.state_real("vt"), x=x, z=z)
    o = b.opts(adve=True, sedi=True, coal=True, cond=True, chem_dsl=True, chem_dsc=True, chem_rct=True)
    for _ in range(steps):
        b.step(o)
    return b, n0, low


TWIN_VARIANTS = {"chem": dict(cond=False, chem_dsl=True, chem_dsc=True, chem_rct=True),
                 "cond_chem": dict(cond=True, chem_dsl=True, chem_dsc=True, chem_rct=True),
                 "cond_chem_no_dsl": dict(cond=True, chem_dsl=False, chem_dsc=True, chem_rct=True)}
TWIN_CASES = [(m, re_, v) for m in MODE_NAMES for re_ in (0, 1, -1) for v in ("chem", "cond_chem")] + [(m, 0, "cond_chem_no_dsl") for m in MODE_NAMES]


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("mode,reorder_every,variant", TWIN_CASES)
def test_chemistry_entered_from_an_object_nobody_has_read(mode, reorder_every, variant, real_t):
    """B.  Two objects from identical options, seeds and inputs go through the same steps (make_twin; the run is reproducible bit for bit,
    tests/test_hip_chemistry.py::test_sulfur_is_conserved_and_the_run_is_reproducible).  Twin 1 is then read in full, which compacts and
    sorts it.  Twin 2 is touched by no getter, diag_* or n_part: it goes straight into one more step_sync -- chemistry alone, or
    condensation and chemistry -- and is read only after it.  What twin 2 must hold comes from the restatement, matched by tag: the
    masses and rd3 of twin 1, rw2 / n / ijk / rhod / dv of twin 2 after the step (chemistry changes none of them), the caller's ambient
    arrays, and T of twin 1's read (chemistry alone: nothing between that read and the step changes it) or T_of(th as passed in)
    (behind condensation with sstp_cond = 1: test_temperature_behind_one_condensation_substep).  Then twin 1 takes the same step: per
    droplet the twins agree bit for bit without chem_dsl, within the bar with it -- each species' bar_for, and for H+, which has no
    closed form, the root's TOL_ROOT in double objects as well (a root finder's stopping decision may flip on an input's last bit).

    That the scenario is what it claims: super-droplets fell out (n_part), multiplicities changed (collisions), and in the toms and
    fast modes at reorder_every = 0 a third twin shows through the raw_ getters, which change no state, that the last step_async left
    the re-sort unfinished ("has not been finished yet") or dead slots in the storage (raw_n longer than n_part).  At most 1 % of the
    droplets may be left out for a dilute flag that differs between the float32 and the float64 restatement, and both classes of
    droplets must remain."""
    ov = TWIN_VARIANTS[variant]
    dsl = ov["chem_dsl"]
    b1, n0, low = make_twin(mode, real_t, reorder_every)
    n_rain = int(low.sum())
    b2, _, _ = make_twin(mode, real_t, reorder_every)
    if mode != "strict" and reorder_every == 0:
        b3, _, _ = make_twin(mode, real_t, reorder_every)
        try:
            b3.p.state_u64("raw_sorted_id")
            unfinished = False
        except RuntimeError as e:
            assert "has not been finished yet" in str(e), str(e)
            unfinished = True
        n_slots = b3.p.state_u64("raw_n").size
        dead = n_slots - b3.p.n_part
        print("re-sort unfinished", unfinished, "dead slots", dead)
        assert unfinished or dead > 0
    # twin 1, read in full
    tag1, o1 = by_tag(b1.p)
    s1 = read(b1, o1)
    assert n0.size - b1.p.n_part >= 3 and n_rain >= 6                                    # (rain drops fell out)
    changed = int(np.sum(s1["n"] != n0[tag1]))
    print("left", n0.size - tag1.size, "of", n_rain, "rain drops; multiplicities changed", changed)
    assert changed >= 3                                                              # (droplets collided)
    gone = np.setdiff1d(np.arange(n0.size), tag1)
    assert np.all(low[gone])                                                         # (what vanished are rain drops of the lowest row)
    # twin 2, straight into the step
    th_in, gas_in = b2.th.copy(), [g.copy() for g in b2.gas]
    o = b2.opts(**ov)
    b2.step(o, async_=False)
    tag2, o2 = by_tag(b2.p)
    assert np.array_equal(tag1, tag2)
    s2 = read(b2, o2)
    rhod = b2.rhod.ravel().astype(np.float64)
    T = h.T_of(th_in.ravel().astype(np.float64), rhod) if ov["cond"] else s1["T"]
    st = dict(n=s2["n"], ijk=s2["ijk"], rw2=s2["rw2"], rd3=s1["rd3"], m=s1["m"], T=T, rhod=s2["rhod"], dv=s2["dv"],
              amb=[g.ravel().astype(np.float64) for g in gas_in])
    if ov["cond"] and real_t is np.float32:
        # (T_of in float32 arithmetic, as a float object evaluates it: measured 1.2e-4 K, four units in the last place, between the
        # library's float T and the double T_of rounded -- enough to move Henry's constants by more than the rest of the float bar)
        st["T32"] = h.T_of(th_in.ravel(), b2.rhod.ravel()).astype(np.float64)
        assert th_in.dtype == np.float32 and b2.rhod.dtype == np.float32
    assert np.array_equal(s2["n"], s1["n"]) and np.array_equal(s2["ijk"], s1["ijk"])
    if not ov["cond"]:
        assert np.array_equal(s2["rw2"], s1["rw2"]) and np.array_equal(s2["T"], s1["T"])
    figs, stats = measure(st, s2, real_t, dsl, True, True)
    print("left out", stats["left_out"])
    assert stats["left_out"] <= 0.01
    both_classes(stats["flag"][stats["sel"]])
    assert stats["flag_agrees"]
    hold(figs, "%s %s" % (mode, variant))
    if dsl:
        for g in GASES:
            assert np.array_equal(b2.gas[g].ravel().astype(np.float64), s2["amb"][g])   # (the caller's arrays were written)
    # twin 1 takes the same step after having been read
    b1.step(b1.opts(**ov), async_=False)
    tag1b, o1b = by_tag(b1.p)
    assert np.array_equal(tag1b, tag2)
    s1b = read(b1, o1b)
    for name, a, b_ in [(NAMES[sp], s1b["m"][sp], s2["m"][sp]) for sp in range(8)] + [("rd3", s1b["rd3"], s2["rd3"])]:
        if dsl:
            assert rel(a, b_) <= stats["bars"].get(name, TOL_ROOT), name
        else:
            assert np.array_equal(a, b_), name


# ------------------------------------------------------------------------------------------ C: which temperature chemistry sees
BUMP = 1.06               # the caller's rv times this ahead of the step under test: a burst of condensation that moves T by tenths of a kelvin
C_DT = 10.                # with a time step of the order of the droplets' phase relaxation time, so that most of it condenses within the step


def activating_box(mode, real_t, **kw):
    """a box with activated droplets that hold dissolved gases (condensation spin-up, three steps of dissolution and dissociation with
    everything else off -- the last step_async ran neither sedi, coal nor cond); the caller then raises rv"""
    b = Box((3, 4), 24, real_t, mode=mode, dt=C_DT, **kw)
    check_mode(b)
    for _ in range(3):
        b.step(b.opts(chem_dsl=True, chem_dsc=True))
    return b


def cond_and_chem_step(b):
    """raises rv, runs one step_sync of cond + chem_dsc + chem_rct; returns the state before, after and th as passed in"""
    b.rv *= b.f(BUMP)
    s = read(b)
    th_in = b.th.copy()
    b.step(b.opts(cond=True, chem_dsc=True, chem_rct=True), async_=False)
    return s, read(b), th_in


def T_fields(b, th_in):
    rhod = b.rhod.ravel().astype(np.float64)
    return h.T_of(th_in.ravel().astype(np.float64), rhod), h.T_of(b.th.ravel().astype(np.float64), rhod)


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_temperature_behind_one_condensation_substep(mode, real_t):
    """C, sstp_cond = 1.  The reference runs hskpng_Tpr ahead of the condensation substep and not again before chemistry
    (particles_step.ipp:244, 269-271), so chemistry sees T of th AS PASSED IN, not the heated one.  The restatement fed
    T_of(th_in, rhod) must match at the per-droplet bars; fed the temperature after condensation it must miss by more than 100 bars
    (the negative half, which says that the step tells the two apart: T must have moved by 1e4 x the bar, in kelvin)."""
    b = activating_box(mode, real_t)
    s, t, th_in = cond_and_chem_step(b)
    check_mode(b)
    T_in, T_out = T_fields(b, th_in)
    st = dict(s, rw2=t["rw2"], T=T_in)
    figs, stats = measure(st, t, real_t, False, True, True, C_DT)
    moved = float(np.max(np.abs(T_out - T_in)))
    print("T moved by", moved, "K; bar", stats["bar_min"], "; T state - T_in", float(np.max(np.abs(t["T"] - T_in))))
    assert moved >= 1e4 * stats["bar_min"]
    both_classes(stats["flag"][stats["sel"]])
    assert stats["left_out"] <= 0.01 and stats["flag_agrees"]
    hold(figs, mode)
    wrong, _ = measure(dict(st, T=T_out), t, real_t, False, True, True, C_DT)
    print("fed the temperature after condensation: worst error / bar", worst(wrong))
    assert worst(wrong) > 100


@pytest.mark.parametrize("real_t", REALS)
def test_temperature_behind_per_cell_substeps(real_t):
    """C, sstp_cond = 4 with per-cell substeps.  The reference's T is that of the start of the LAST substep, which a test cannot
    restate; the strict path launches k_cell_cond_pre per substep and so has it by construction.  The T state read after the step in
    the toms and fast modes (all substeps in one launch) must agree with the strict one's to 10 x cond_bars(False)[0] (the bar that one
    step of condensation in fast arithmetic is held to in th, tests/_harness.py, with a factor for the spin-up's seven steps), and in
    every mode the restatement fed that T state must match the masses.  That state is neither T_of(th_in) nor T_of(th_out): it
    differs from both by more than 100 times that margin."""
    margin = 10 * h.cond_bars(False)[0]
    T_state = {}
    for mode in MODE_NAMES:
        b = activating_box(mode, real_t, sstp_cond=4)
        s, t, th_in = cond_and_chem_step(b)
        check_mode(b)
        T_state[mode] = t["T"]
        T_in, T_out = T_fields(b, th_in)
        d_in, d_out = float(np.max(np.abs(t["T"] - T_in) / T_in)), float(np.max(np.abs(t["T"] - T_out) / T_out))
        print(mode, "T state against T_of(th_in)", d_in, "against T_of(th_out)", d_out, "margin", margin)
        assert d_in > 100 * margin and d_out > 100 * margin
        figs, stats = measure(dict(s, rw2=t["rw2"], T=t["T"]), t, real_t, False, True, True, C_DT)
        both_classes(stats["flag"][stats["sel"]])
        assert stats["left_out"] <= 0.01 and stats["flag_agrees"]
        hold(figs, mode)
    for mode in ("toms", "fast"):
        d = rel(T_state[mode], T_state["strict"])
        print(mode, "T state against strict", d)
        assert d <= margin


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_temperature_behind_per_particle_substeps(mode, real_t):
    """C, exact_sstp_cond with sstp_cond = 4.  The reference runs no hskpng_Tpr in step_sync at all then, so chemistry sees what the
    previous step_async left: the T state keeps its bits through the step, although condensation heated the air, and the restatement
    fed it matches."""
    b = activating_box(mode, real_t, sstp_cond=4, exact_sstp_cond=True)
    s, t, th_in = cond_and_chem_step(b)
    check_mode(b)
    assert np.array_equal(t["T"], s["T"])
    _, T_out = T_fields(b, th_in)
    figs, stats = measure(dict(s, rw2=t["rw2"]), t, real_t, False, True, True, C_DT)
    moved = float(np.max(np.abs(T_out - s["T"])))
    print("T_of(th_out) - T state", moved, "K; bar", stats["bar_min"])
    assert moved >= 1e4 * stats["bar_min"]
    both_classes(stats["flag"][stats["sel"]])
    assert stats["left_out"] <= 0.01 and stats["flag_agrees"]
    hold(figs, mode)


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_temperature_without_condensation(mode, real_t):
    """C, cond off.  T is what the previous step_async computed (the reference's step_async runs hskpng_Tpr whatever the options,
    particles_step.ipp:375; here that step_async ran with sedi, coal and cond all off).  The caller's th is 1 K warmer in the step
    under test: chemistry must not see that -- the T state keeps its bits, the restatement fed it matches, and fed T_of(the new th)
    it misses by more than 100 bars.  After the step_async that follows, which again runs none of the three, it does see it."""
    b = activating_box(mode, real_t)
    s = read(b)
    b.th += b.f(1.)
    b.step(b.opts(chem_dsc=True, chem_rct=True), async_=False)
    t = read(b)
    assert np.array_equal(t["T"], s["T"])
    figs, stats = measure(s, t, real_t, False, True, True, C_DT)
    both_classes(stats["flag"][stats["sel"]])
    assert stats["left_out"] <= 0.01 and stats["flag_agrees"]
    hold(figs, mode)
    T_new = h.T_of(b.th.ravel().astype(np.float64), b.rhod.ravel().astype(np.float64))
    assert float(np.min(np.abs(T_new - s["T"]))) > 0.5
    wrong, _ = measure(dict(s, T=T_new), t, real_t, False, True, True, C_DT)
    print("fed T of the new th: worst error / bar", worst(wrong))
    assert worst(wrong) > 100
    # the step_async that follows runs neither sedi, coal nor cond and recomputes T all the same -- from the th of its step_sync: the
    # next step's chemistry matches the restatement fed T_of(th + 1 K) (evaluated in both precisions for a float object: T itself
    # is restated here) and misses by more than 100 bars fed the old T
    b.p.step_async(b.opts(chem_dsc=True, chem_rct=True))
    s2 = read(b)
    b.step(b.opts(chem_dsc=True, chem_rct=True), async_=False)
    t2 = read(b)
    st2 = dict(s2, T=T_new)
    if real_t is np.float32:
        st2["T32"] = h.T_of(b.th.ravel(), b.rhod.ravel()).astype(np.float64)
    figs, stats = measure(st2, t2, real_t, False, True, True, C_DT)
    assert stats["left_out"] <= 0.01 and stats["flag_agrees"]
    hold(figs, mode + " next step")
    wrong, _ = measure(dict(s2, T=s["T"]), t2, real_t, False, True, True, C_DT)
    print("next step fed the old T: worst error / bar", worst(wrong))
    assert worst(wrong) > 100


# ------------------------------------------------------------------------------------------ D: the masses through coalescence
COAL_N = [1, 4, 16, 64]   # multiplicities in units of n_unit: equal ones are frequent, and a pair can collide up to 64 times in a step


def coal_box(real_t, dims=(3, 3), sd_conc=48, mode="strict", chem_steps=2, n_unit=1e9, r_lo=20e-6, **kw):
    """a box of drizzle: radii from r_lo to 10 r_lo and multiplicities of 1, 4, 16 or 64 x n_unit through set_particles, which sets the
    masses from rd3 again; chem_steps steps of dissolution and oxidation then leave the eight masses no longer proportional to each
    other.  (20 ... 200 um at 1e9: nearly every pair collides in a step, many of them several times; 10 ... 100 um at 1e8: a pair in
    ten, so that a box lasts for many steps.)"""
    b = Box(dims, sd_conc, real_t, mode=mode, coal_switch=True, sedi_switch=True, dbg_flags=int(lgrngn.dbg.TAG), cond_steps=1, **kw)
    check_mode(b)
    s = b.state()
    i = np.arange(s["n"].size)
    rng = np.random.default_rng(11)
    r = r_lo * 10. ** rng.random(i.size)
    n = n_unit * np.array(COAL_N, dtype=np.float64)[rng.integers(0, len(COAL_N), i.size)]
    b.p.set_particles(n, s["rd3"], r * r, b.p.state_real("kappa"), b.p.state_real("vt"), x=b.p.state_real("x"), z=b.p.state_real("z"))
    for _ in range(chem_steps):
        b.step(b.opts(chem_dsl=True, chem_rct=True))
    return b


def summator(m, sid, col, f, swap=False):
    """the reference's summator (coal.ipp:46-57, 458-480) to the letter; swap: the two sides exchanged (the negative control)"""
    m = [x.astype(f) for x in m]
    out = [x.copy() for x in m]
    touched = np.zeros(m[0].size, dtype=bool)
    for p in np.nonzero(col[:-1] > 0)[0]:
        a, b_ = sid[p], sid[p + 1]
        first_ge = col[p + 1] == -2
        if first_ge != swap:
            for sp in range(8):
                out[sp][b_] = m[sp][b_] + f(col[p]) * m[sp][a]
            touched[b_] = True
        else:
            for sp in range(8):
                out[sp][a] = m[sp][a] + f(col[p]) * m[sp][b_]
            touched[a] = True
    return out, touched


@pytest.mark.parametrize("real_t", REALS)
def test_masses_of_each_droplet_through_one_coalescence(real_t):
    """D1 and D3.  One coalescence stage on a 3 x 3 box of 48 drizzle drops per cell whose eight masses are not proportional to each
    other; the order it paired the droplets in (sorted_id), its collision record (col) and the multiplicities are read, and the
    reference's summator applied in numpy: for col[p] > 0 with a = sorted_id[p], b = sorted_id[p + 1], m[b] += col[p] m[a] if
    col[p + 1] == -2, else m[a] += col[p] m[b].  A changed value may differ by 4 eps of the working precision (one multiplication and
    one addition, fused or not); every other droplet keeps its bits.  With the two sides exchanged the same check must fail.
    At least 10 pairs collide, one of them more than once, one of them at equal multiplicities -- where the first of the pair counts
    as the greater (col[p + 1] == -2).
    D3: n m summed over a pair, and over the box, is conserved for all eight species.  Pairs of equal multiplicities are NOT left
    out: the reference's collider (coal.ipp:118-143, 243-254) takes col x n_b from n_a and halves nothing, so at equal multiplicities
    the first droplet is left with n = 0 ("flagging for recycling") and the second, which the summator adds to, carries the mass of
    both.  A split of the multiplicities happens only later and only with opts.rcyc, which copies all attributes.  The test asserts
    that the first of such a pair is used up and that the pair conserves like any other."""
    f = np.dtype(real_t).type
    b = coal_box(real_t)
    b.p.stage("hskpng_Tpr")
    b.p.stage("hskpng_vterm_all")
    s = read(b)
    assert all(np.any(x > 0) for x in s["m"][:7])                                        # (all species present; H always is)
    ratio = s["m"][c.SO2] / s["m"][c.S_VI]
    assert ratio.max() > 1.5 * ratio.min()                                               # (not proportional any more)
    b.p.stage("coal", b.opts(coal=True))
    sid = b.p.state_u64("sorted_id").astype(np.int64)
    col = b.p.state_real("col")
    t = read(b)
    pairs = np.nonzero(col[:-1] > 0)[0]
    n_a, n_b = s["n"][sid[pairs]], s["n"][sid[pairs + 1]]
    equal = n_a == n_b
    print("colliding pairs", pairs.size, "more than once", int(np.sum(col[pairs] > 1)), "at equal multiplicities", int(equal.sum()))
    assert pairs.size >= 10 and np.any(col[pairs] > 1) and equal.any()
    assert np.all(col[pairs + 1][equal] == -2)
    assert np.all((col[pairs + 1] == -2) == (n_a >= n_b))
    want, touched = summator(s["m"], sid, col, f)
    assert touched.sum() == pairs.size
    worst_err = 0.
    for sp in range(8):
        assert np.array_equal(t["m"][sp][~touched], s["m"][sp][~touched]), NAMES[sp]
        worst_err = max(worst_err, rel(t["m"][sp][touched], want[sp][touched]))
    print("largest error of a changed mass", worst_err, "bar", 4 * eps_of(real_t))
    assert worst_err <= 4 * eps_of(real_t)
    swapped, _ = summator(s["m"], sid, col, f, swap=True)
    wrong = max(rel(t["m"][sp][touched], swapped[sp][touched]) for sp in range(8))
    print("with the sides exchanged", wrong)
    assert wrong > 100 * 4 * eps_of(real_t)
    # D3: n m of a pair, all eight species.  (n < 2^37 is exact in double; in float n and each product are rounded once, and so is
    # the new mass twice: 8 eps of the pair's sum covers the six roundings)
    for sp in range(8):
        ia, ib = sid[pairs], sid[pairs + 1]
        before = s["n"][ia] * s["m"][sp][ia] + s["n"][ib] * s["m"][sp][ib]
        after = t["n"][ia] * t["m"][sp][ia] + t["n"][ib] * t["m"][sp][ib]
        assert np.all(np.abs(after - before) <= 8 * eps_of(real_t) * before), NAMES[sp]
        tot0, tot1 = np.sum(s["n"] * s["m"][sp]), np.sum(t["n"] * t["m"][sp])
        assert abs(tot1 - tot0) <= 8 * eps_of(real_t) * tot0, NAMES[sp]
    assert np.all(t["n"][sid[pairs]][equal] == 0) and np.all(t["n"][sid[pairs + 1]][equal] == n_b[equal])


INIT_SPECIES = {c.NH3: "NH3_H2O", c.S_VI: "H2SO4", c.H: "H"}


class Gains:
    """How often each super-droplet has gained by coalescence, from the raw_ getters, which compact and sort nothing (the deferred sort
    and the dead slots of the non-strict modes stay as they are): read after every step, a droplet whose rd3 differs from what its tag
    held before has gained in that step -- once per coalescence substep at most (per_step: the number of substeps, the count a change
    stands for).  A recycled slot (opts.rcyc) carries its donor's tag and rd3, and with them the donor's count."""

    def __init__(self, p, per_step=1):
        self.p, self.per_step = p, per_step
        self.cnt = {}
        for t, r in self.alive():
            self.cnt.setdefault(t, []).append((r, 0))

    def alive(self):
        tag, rd3, n = self.p.state_real("raw_tag").astype(np.int64), self.p.state_real("raw_rd3"), self.p.state_u64("raw_n")
        assert tag.size == rd3.size == n.size
        return [(int(t), float(r)) for t, r, k in zip(tag, rd3, n) if k > 0]

    def update(self):
        new = {}
        for t, r in self.alive():
            prev = self.cnt[t]
            same = [k for r0, k in prev if r0 == r]
            new.setdefault(t, []).append((r, max(same) if same else max(k for _, k in prev) + self.per_step))
        self.cnt = new

    def of(self, tag, rd3):
        return np.array([max(k for r0, k in self.cnt[int(t)] if r0 == float(r)) for t, r in zip(tag, rd3)])


def ratio_errors(m, rd3, real_t):
    """|m / rd3 - constant| / constant in units of eps, per droplet, the largest of NH3, S_VI and H"""
    worst_ = np.zeros(rd3.shape)
    for sp, key in INIT_SPECIES.items():
        const = 4. / 3 * np.pi * c.CHEM_RHO * c.M[key] / (c.M["NH4"] + c.M["HSO4"])
        worst_ = np.maximum(worst_, np.abs(m[sp] / rd3 - const) / const)
    return worst_ / eps_of(real_t)


def assert_masses_follow_rd3(b, real_t, gains):
    """D2's invariant: the initial NH3, S_VI and H masses are fixed multiples of rd3 (k_chem_init), and the summator is linear and
    applied to rd3 with the same col and the same partner, so the three ratios to rd3 stay at their constants for every surviving
    droplet; the other five masses stay 0.  The bar of a droplet is (its number of gains + 2) eps, 64 eps at the most; the gains are
    counted per tag by `gains` (class Gains)."""
    s = read(b)
    tag = b.p.state_real("tag").astype(np.int64)
    k = gains.of(tag, s["rd3"])
    err = ratio_errors(s["m"], s["rd3"], real_t)
    for kk in np.unique(k):
        print("gains", int(kk), "droplets", int(np.sum(k == kk)), "largest error", float(err[k == kk].max()), "eps; bar", min(int(kk) + 2, 64))
    assert np.all(err <= np.minimum(k + 2, 64)), (float(np.max(err / np.minimum(k + 2, 64))))
    for sp in range(8):
        if sp not in INIT_SPECIES:
            assert not s["m"][sp].any(), NAMES[sp]
    return s, k


D2_CASES = [(m, "geometric") for m in MODE_NAMES] + [("strict", "hall_pinsky_stratocumulus"), ("fast", "hall_pinsky_stratocumulus")]


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("mode,kernel", D2_CASES)
def test_masses_follow_rd3_through_coalescence_and_motion(mode, kernel, real_t):
    """D2: 20 steps of coal + adve + sedi with the Courant numbers of h.box_fields, no chemistry process and no condensation, in the three
    modes; conservation of the totals would not notice a wrong partner, a wrong side of col[p + 1] == -2 or a wrong col: this does
    (test_the_rd3_invariant_notices_a_wrong_partner).  The tabulated kernel takes the production form of the coalescence kernel, which
    writes the collision record only because chemistry (or a second kappa) asks for it."""
    b = coal_box(real_t, dims=(3, 4), sd_conc=32, mode=mode, chem_steps=0, courant=True, n_unit=1e8, r_lo=10e-6,
                 kernel=getattr(lgrngn.kernel_t, kernel))
    n0 = b.p.n_part
    gains = Gains(b.p)
    o = b.opts(adve=True, sedi=True, coal=True)
    for _ in range(20):
        b.step(o)
        gains.update()
    s, k = assert_masses_follow_rd3(b, real_t, gains)
    print("super-droplets left", k.size, "of", n0, "; grown by coalescence", int(np.sum(k > 0)), "; most gains", int(k.max()))
    assert k.size < n0 and np.sum(k > 0) >= 10 and k.max() >= 2


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("path", ["fused", "rcyc", "sstp_coal_2"])
def test_masses_follow_rd3_through_a_whole_step(path, real_t):
    """D1's box through whole step_async calls in the parity mode, where the order that coalescence paired the droplets in cannot be
    read afterwards (and col shows the last substep only): the fused move with the dead marked by the coalescence kernel, the plain
    sequence that opts.rcyc takes, and two coalescence substeps -- checked with D2's invariant at the per-droplet bar (with two
    substeps a step in which rd3 changed counts as two gains).  The exact by-tag check of what recycling copies is
    test_recycling_copies_the_masses_of_its_donor."""
    b = coal_box(real_t, chem_steps=0, **({"sstp_coal": 2} if path == "sstp_coal_2" else {}))
    gains = Gains(b.p, per_step=2 if path == "sstp_coal_2" else 1)
    o = b.opts(sedi=True, coal=True, rcyc=(path == "rcyc"))
    for _ in range(3):
        b.step(o)
        gains.update()
    s, k = assert_masses_follow_rd3(b, real_t, gains)
    print("grown by coalescence", int(np.sum(k > 0)))
    assert np.sum(k > 0) >= 10
    if path == "rcyc":
        _, cnt = np.unique(b.p.state_real("tag"), return_counts=True)
        assert np.any(cnt > 1)                                                           # (slots were recycled)


@pytest.mark.parametrize("real_t", REALS)
def test_recycling_copies_the_masses_of_its_donor(real_t):
    """the plain sequence's post_copy with opts.rcyc straight after a coalescence stage that used super-droplets up, with the eight masses
    not proportional to each other: every super-droplet afterwards holds, bit for bit, the eight masses and rd3 that its tag held after
    the coalescence (a recycled slot carries its donor's tag), and some tags are there twice"""
    b = coal_box(real_t)
    b.p.stage("hskpng_Tpr")
    b.p.stage("hskpng_vterm_all")
    b.p.stage("coal", b.opts(coal=True))
    tag0 = b.p.state_real("tag").astype(np.int64)
    s = read(b)
    assert np.sum(s["n"] == 0) >= 3 and np.unique(tag0).size == tag0.size
    b.p.stage("post_copy", b.opts(rcyc=True))
    tag1 = b.p.state_real("tag").astype(np.int64)
    t = read(b)
    _, cnt = np.unique(tag1, return_counts=True)
    print("used up", int(np.sum(s["n"] == 0)), "tags twice", int(np.sum(cnt > 1)))
    assert np.any(cnt > 1) and np.all(t["n"] > 0)
    src = np.argsort(tag0)[np.searchsorted(np.sort(tag0), tag1)]
    assert np.array_equal(tag0[src], tag1)
    assert np.all(s["n"][src] > 0)
    for sp in range(8):
        assert np.array_equal(t["m"][sp], s["m"][sp][src]), NAMES[sp]
    assert np.array_equal(t["rd3"], s["rd3"][src]) and np.array_equal(t["rw2"], s["rw2"][src])


def test_the_rd3_invariant_notices_a_wrong_partner():
    """the negative control of D2: masses proportional to rd3 go through one coalescence stage; with the library's rd3 after it, masses
    computed in numpy by the right summator keep the three ratios within (1 + 2) eps, and masses computed with the two sides
    exchanged, or with col + 1 in place of col, break them by more than 100 times that"""
    b = coal_box(np.float64, chem_steps=0)
    b.p.stage("hskpng_Tpr")
    b.p.stage("hskpng_vterm_all")
    s = read(b)
    b.p.stage("coal", b.opts(coal=True))
    sid, col = b.p.state_u64("sorted_id").astype(np.int64), b.p.state_real("col")
    rd3 = b.p.state_real("rd3")
    right, touched = summator(s["m"], sid, col, np.float64)
    assert touched.sum() >= 10
    e = ratio_errors(right, rd3, np.float64)[touched].max()
    print("right summator", e, "eps")
    assert e <= 3
    swapped, moved = summator(s["m"], sid, col, np.float64, swap=True)
    more = np.where(col > 0, col + 1, col)
    one_more, _ = summator(s["m"], sid, more, np.float64)
    for name, m, where in (("sides exchanged", swapped, touched | moved), ("col + 1", one_more, touched)):
        e = ratio_errors(m, rd3, np.float64)[where].max()
        print(name, e, "eps")
        assert e > 300


@pytest.mark.parametrize("real_t", REALS)
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_one_crowded_cell_in_the_three_modes(mode, real_t):
    """the 0-D box of 130 -- more than two waves in one cell, where the cell's sum of the dissolved amounts takes several passes of a
    wave -- in the three modes: condensation and all of the chemistry in one step_sync against the restatement fed T_of(th as passed
    in), evaluated in both precisions for a float object"""
    b = Box((0, 0), 130, real_t, mode=mode)
    check_mode(b)
    for _ in range(3):
        b.step(b.opts(cond=True, chem_dsl=True, chem_dsc=True))
    s = read(b)
    th_in, gas_in = b.th.copy(), [g.copy() for g in b.gas]
    b.step(b.opts(cond=True, chem_dsl=True, chem_dsc=True, chem_rct=True), async_=False)
    check_mode(b)
    t = read(b)
    rhod = b.rhod.ravel().astype(np.float64)
    st = dict(s, rw2=t["rw2"], T=h.T_of(th_in.ravel().astype(np.float64), rhod), amb=[g.ravel().astype(np.float64) for g in gas_in])
    if real_t is np.float32:
        st["T32"] = h.T_of(th_in.ravel(), b.rhod.ravel()).astype(np.float64)
    figs, stats = measure(st, t, real_t, True, True, True)
    both_classes(stats["flag"][stats["sel"]])
    assert stats["left_out"] <= 0.01 and stats["flag_agrees"]
    hold(figs, mode + " 0-D")


# ------------------------------------------------------------------------------------------ E: ambient_chem in three kinds of arrays
@pytest.mark.parametrize("real_t", REALS)
def test_ambient_chem_as_contiguous_strided_and_device_arrays(real_t):
    """E: the six gases passed as contiguous host arrays, as views into padded storage, with the two horizontal axes swapped in memory
    (the layouts of tests/test_api_invariants.py::test_strided_eulerian_arrays) and as lgrngn.DeviceArray over torch tensors give
    the same bits after init, after two steps of condensation and chemistry, and in the gases written back"""
    import torch
    oi = h.box_opts(4, 3, 5, 16, coal_switch=False, sedi_switch=False)
    oi.chem_switch, oi.chem_rho = True, c.CHEM_RHO
    th, rv, rhod, C = [(x.astype(real_t) if not isinstance(x, dict) else {k_: v.astype(real_t) for k_, v in x.items()}) for x in h.box_fields(oi)]
    rng = np.random.default_rng(2)
    gas0 = [(g * (1 + 0.05 * rng.random(th.shape))).astype(real_t) for g in c.ICICLE_GAS]

    def padded(a):
        big = np.full(tuple(n + 2 for n in a.shape), np.nan, dtype=real_t)
        v = big[1:-1, 1:-1, :-2]
        assert not v.flags["C_CONTIGUOUS"] and v.strides[2] == a.itemsize
        v[...] = a
        return v

    def kij(a):
        v = np.empty((a.shape[1], a.shape[0], a.shape[2]), dtype=real_t).transpose(1, 0, 2)
        assert v.strides[0] < v.strides[1]
        v[...] = a
        return v
    res = []
    for kind in ("contiguous", "padded", "kij", "device"):
        keep = None
        if kind == "device":
            keep = [torch.tensor(g, device="cuda") for g in gas0]
            torch.cuda.synchronize()
            amb = {SP(g): lgrngn.DeviceArray(keep[g].data_ptr(), keep[g].shape) for g in GASES}
        else:
            keep = [dict(contiguous=np.copy, padded=padded, kij=kij)[kind](g) for g in gas0]
            amb = {SP(g): keep[g] for g in GASES}
        a_th, a_rv = th.copy(), rv.copy()
        p = h.hip_particles(oi, real_t)
        p.init(a_th, a_rv, rhod, ambient_chem=amb, **C)
        out = [p.state_real("chem_" + nm) for nm in NAMES] + [p.state_real("ambient_" + NAMES[g]) for g in GASES]
        o = lgrngn.opts_t()
        o.adve = o.sedi = o.coal = False
        o.chem_dsl = o.chem_dsc = o.chem_rct = True
        for _ in range(2):
            p.step_sync(o, a_th, a_rv, rhod, ambient_chem=amb, **C)
            p.step_async(o)
        h.assert_mode(p, True, 0, kernel="strict")
        out += [p.state_real("chem_" + nm) for nm in NAMES] + [p.state_real("ambient_" + NAMES[g]) for g in GASES]
        if kind == "device":
            torch.cuda.synchronize()
            out += [k_.cpu().numpy() for k_ in keep]
        else:
            out += [np.array(k_) for k_ in keep]
        res.append(out + [a_th, a_rv])
    assert any(not np.array_equal(a, g) for a, g in zip(res[0][-8:-2], gas0))          # (dissolution did write the gases back)
    assert np.any(res[0][14 + c.SO2] > 0)
    for other in res[1:]:
        assert len(other) == len(res[0])
        for a, b_ in zip(res[0], other):
            assert np.array_equal(a, b_)
