"""Tracked super-droplets (include/lcx_track.h) on the device, in double and float, against tests/_track_reference.py (plain numpy over the
raw state).

1. Records are the raw state: 2-D and 3-D, condensation + coalescence + the move, a sample after each of six steps.
2. The selection rule: clauses, a box, Q below, at and above the room, a second selection, filling up, select_slots.
3. Identity through everything that moves storage: deaths, compaction, re-ordering, a source, recycling -- with LCX_DBG_TAG beside.
4. Nothing else moves: every raw array, th, rv, the puddle, the sorted order, the mode, the snapshot; a restored object is disabled.
5. The slot list is reused: `scans`, and the launch counts.
6. Automatic sampling, the buffer, reset, droplets selected between two samples.
7. Device output with padded strides, every error text, refusals, disable and enable again, a 0-D parcel.
"""
import ctypes as C

import numpy as np
import pytest

import _harness as h
import _track_reference as TR
import test_hip_move_rates as TMV
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

LD = np.longdouble
REALS = [np.float64, np.float32]
REAL_IDS = ["f64", "f32"]
F32 = lambda v: float(np.float32(v))                 # radii that float holds exactly: every way of forming the bound agrees


def rainy(real_t, dims=3, n=6, per_cell=16, seed=7, cz=None, strict=False, kappas=(.5,), **kw):
    """an n^dims box of 1 m cells in the spirit of test_hip_move_rates.rainy_box: box_fields' air and Courant numbers, radii log-uniform in
    5 ... 80 um (the large ones fall through the bottom within a few steps), multiplicities that make a few per cent of the pairs collide"""
    ny = n if dims == 3 else 0
    oi = h.box_opts(n, ny, n, per_cell, dx=1., dt=1., kernel=lgrngn.kernel_t.hall, terminal_velocity=lgrngn.vt_t.beard77fast, **kw)
    if not strict:
        h.api_default_opts(oi)
    th, rv, rhod, Cc = h.box_fields(oi)
    if cz is not None:
        Cc["Cz"] = np.full_like(Cc["Cz"], cz)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    fields = (f(th), f(rv), f(rhod), {k: f(v) for k, v in Cc.items()})
    rng = np.random.default_rng(seed)
    n_cell = n ** dims
    cells = np.repeat(np.arange(n_cell), per_cell)
    N = cells.size
    r = np.exp(rng.uniform(np.log(5e-6), np.log(80e-6), N))
    mult = rng.integers(125000, 500000, N).astype(np.uint64)
    mult[(r > 19.9e-6) & (r < 25e-6)] *= np.uint64(400)
    args = dict(n=mult, rd3=(1e-8 * (1 + np.arange(N) / 7.)) ** 3, rw2=((r.astype(LD) ** 2).astype(real_t)).astype(np.float64),
                kpa=rng.choice(np.array(kappas), N), vt=np.full(N, .1))
    if dims == 3:
        i, j, k = cells // (n * n), (cells // n) % n, cells % n
        args.update(x=i + rng.uniform(.05, .95, N), y=j + rng.uniform(.05, .95, N), z=k + rng.uniform(.05, .95, N))
    else:
        i, k = cells // n, cells % n
        args.update(x=i + rng.uniform(.05, .95, N), z=k + rng.uniform(.05, .95, N))
    prt = h.hip_particles(oi, real_t)
    prt.init(fields[0].copy(), fields[1].copy(), fields[2].copy(), **{kk: v.copy() for kk, v in fields[3].items()})
    prt.set_particles(**args)
    return prt, fields, oi


def step(prt, fields, opts):
    th, rv, rhod, Cc = fields
    prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    prt.step_async(opts)


def assert_record(rec, s, st, n_tracked, tag):
    want, alive = TR.record(st, n_tracked)
    for f in TR.FIELDS:
        assert rec[f].shape[1] == n_tracked and np.array_equal(rec[f][s], want[f], equal_nan=True), (tag, "sample", s, f, rec[f][s], want[f])
    return alive


def assert_marks(st, slots, idx, tag):
    want = np.zeros(st["n"].size)
    want[slots] = idx + 1.
    assert np.array_equal(st["track"], want), (tag, np.flatnonzero(st["track"] != want)[:8])


# ---------------------------------------------------------------------------------------------------- 1. records are the raw state
@pytest.mark.parametrize("dims", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_records_are_the_raw_state(real_t, dims):
    n = 8 if dims == 2 else 6
    prt, fields, oi = rainy(real_t, dims, n)
    h.assert_mode(prt, strict_fp=False)
    prt.track_enable(64, capacity=8)
    clauses, box = [("rng", "wet", F32(10e-6), 1.)], (1., n - 1., 1., n - 1., 0., float(n))
    st = TR.raw_state(prt)
    Q = int(TR.qualifies(st, clauses, box, real_t).sum())
    slots, idx = TR.select(st, clauses, box, 40, 64, 0, real_t)
    assert Q > 80 and slots.size <= 40 and slots[1] - slots[0] > 1, "the stride of this selection is above 1"
    assert prt.track_select(clauses, box=box, max_count=40) == slots.size
    assert_marks(TR.raw_state(prt), slots, idx, "selection")
    n_tr, opts, alive = slots.size, lgrngn.opts_t(), None                # everything on: condensation, coalescence, advection, sedimentation
    states = []
    for s in range(6):
        step(prt, fields, opts)
        prt.track_sample()
        states.append(TR.raw_state(prt))
    rec = prt.track()
    assert list(rec["steps"]) == [1, 2, 3, 4, 5, 6] and np.array_equal(rec["time"], np.arange(1, 7) * oi.dt)
    for s in range(6):
        alive = assert_record(rec, s, states[s], n_tr, (real_t.__name__, dims))
    assert 0 < alive.sum() < n_tr, "some tracked droplets have left through the bottom, others live on: %d of %d" % (alive.sum(), n_tr)
    gone = ~alive
    assert (rec["n"][-1][gone] == 0).all() and all(np.isnan(rec[f][-1][gone]).all() for f in TR.FIELDS[1:]), "the absent pattern"
    assert (rec["n"][0] > 0).sum() > alive.sum() and not np.array_equal(rec["rw2"][0], rec["rw2"][-1]) and not np.array_equal(rec["z"][0], rec["z"][1])
    if dims == 2:
        assert (rec["y"][0][rec["n"][0] > 0] == 0).all()


# ---------------------------------------------------------------------------------------------------- 2. the selection rule
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_selection_rule(real_t):
    prt, fields, oi = rainy(real_t, 3, 6, kappas=(.3, .5, .7))
    dead = np.arange(5, 3456, 97)                                         # dead slots in the middle of the storage
    st0 = TR.raw_state(prt)
    mult = st0["n"].copy()
    mult[dead] = 0
    prt.set_particles(n=mult, rd3=st0["rd3"], rw2=st0["rw2"], kpa=st0["kappa"], vt=st0["vt"], x=st0["x"], y=st0["y"], z=st0["z"])
    wet, dry, kap = ("rng", "wet", F32(20e-6), F32(40e-6)), ("rng", "dry", F32(1e-8), F32(3e-6)), ("rng", "kappa", F32(.4), F32(.6))
    box = (1.5, 4.25, 0., 3., 2., 6.)
    cases = [([wet], None), ([dry], None), ([kap], None), ([("water",)], None), ([("all",)], None), ([wet, kap], None), ([("all",), dry, ("water",), kap], box),
             ([("all",)], box), ([wet], box)]
    for clauses, bx in cases:
        prt.track_enable(4000)
        st = TR.raw_state(prt)
        assert (st["track"] == 0).all() and (st["n"][dead] == 0).all()
        Q = int(TR.qualifies(st, clauses, bx, real_t).sum())
        assert 8 < Q < (st["n"] > 0).sum() or clauses[0][0] in ("all", "water"), (clauses, Q)
        for max_count in (Q + 3, Q, Q - 1, 7, None):                      # Q < room, Q == room, Q > room (strides 2 and above), all the room
            prt.track_enable(4000 if max_count is not None else 50)
            room = max_count if max_count is not None else 50
            slots, idx = TR.select(st, clauses, bx, room, 4000 if max_count is not None else 50, 0, real_t)
            got = prt.track_select(clauses, box=bx, max_count=max_count)
            assert got == slots.size and prt.track_info()["n_tracked"] == got, (clauses, bx, max_count, got, slots.size)
            assert got == (Q if room >= Q else -(-Q // -(-Q // room)))
            assert_marks(TR.raw_state(prt), slots, idx, (clauses, bx, max_count))
    # a second selection skips marked droplets and continues the indices; the set fills up to max_tracked exactly
    prt.track_enable(100)
    st = TR.raw_state(prt)
    s1, i1 = TR.select(st, [wet], None, 30, 100, 0, real_t)
    assert prt.track_select([wet], max_count=30) == s1.size > 20
    st = TR.raw_state(prt)
    s2, i2 = TR.select(st, [("all",)], box, 1000, 100, s1.size, real_t)             # room: what is left of max_tracked
    assert prt.track_select([("all",)], box=box, max_count=1000) == s2.size and not set(s1) & set(s2) and i2[0] == s1.size
    assert_marks(TR.raw_state(prt), np.concatenate([s1, s2]), np.concatenate([i1, i2]), "second selection")
    n_now = s1.size + s2.size
    assert prt.track_info()["n_tracked"] == n_now <= 100
    if n_now == 100:                                                      # (the rule may fill the room exactly: make room for select_slots)
        prt.track_enable(100)
        assert prt.track_select([wet], max_count=30) == s1.size
        s2, i2, n_now = s2[:0], i2[:0], s1.size
    # select_slots: dead, duplicate, marked and out-of-range slots are skipped, the order is the caller's, it stops at max_tracked
    st = TR.raw_state(prt)
    free = np.flatnonzero((st["n"] > 0) & (st["track"] == 0))[::-1][:150]
    ask = np.concatenate([[dead[0], free[0], free[0], int(s1[0]), 3456, 10 ** 12, free[1]], free[2:]])
    took = TR.select_slots(st, ask, 100, n_now)
    assert took.size == 100 - n_now and took[0] == free[0] and took[1] == free[1]
    assert prt.track_select_slots(ask) == took.size
    info = prt.track_info()
    assert info["n_tracked"] == info["max_tracked"] == 100
    assert_marks(TR.raw_state(prt), np.concatenate([s1, s2, took]), np.arange(100), "select_slots")
    assert prt.track_select([("all",)]) == 0 and prt.track_select_slots(free[-5:]) == 0, "a full set takes nothing more"
    prt.track_sample()
    assert_record(prt.track(), 0, TR.raw_state(prt), 100, "after select_slots")


# ---------------------------------------------------------------------------------------------------- 3. identity
def tag_map(st, tag):
    marked = np.flatnonzero(st["track"] != 0)
    m = {int(tag[s]): int(st["track"][s]) - 1 for s in marked}
    assert len(m) == marked.size, "a tag carries one mark at most"
    return m


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_identity_through_everything_that_moves_storage(real_t):
    """(TR.raw_state reads the cell arrays "T", "RH", "rv", and a getter without "raw_" compacts the storage first: behind every step's
    reads the dead slots are gone through the test's doing, not only the step's.  The raw arrays are read ahead of that and the sample is
    taken ahead of both, so the comparisons are of one moment; the marks must survive those compactions like any other.)"""
    n = 6
    key = (.61, 0.)
    prt, fields, oi = rainy(real_t, 2, n, per_cell=32, cz=-.6, dbg_flags=int(lgrngn.dbg.TAG), reorder_every=2, src_type=lgrngn.src_t.simple,
                            src_x0=0., src_x1=float(n), src_z0=2., src_z1=4., n_sd_max=4096)
    prt.track_enable(256, capacity=16)
    n_bot = prt.track_select([("all",)], box=(0., n, 0., 0., 0., 1.), max_count=40)       # the lowest level: gone within two steps of Cz = -0.6
    n_top = prt.track_select([("all",)], box=(0., n, 0., 0., n - 1., n), max_count=40)    # the top level: lives on
    assert n_bot > 30 and n_top > 30
    st = TR.raw_state(prt)
    tag = prt.state_real("raw_tag")
    first = tag_map(st, tag)
    assert sorted(first.values()) == list(range(n_bot + n_top))
    opts = lgrngn.opts_t()
    opts.src = True
    opts.src_dry_distros = {key: (h.lognormal_fn(.05e-6, 1.5, 60e6), 8, 2)}        # fires every second step: 8 newcomers in each of 12 cells
    n_tr, n_tags, n_first = n_bot + n_top, int(tag.max()) + 1, int(tag.max()) + 1
    fired = recycled = 0
    for s in range(5):
        if s == 3:                                                            # droplets with the largest multiplicities: the donors of step 4's recycling
            big = np.argsort(-st["n"].astype(np.int64), kind="stable")[:12]
            n_tr += prt.track_select_slots(big)
            first = tag_map(TR.raw_state(prt), prt.state_real("raw_tag"))
            opts.rcyc, opts.src = True, False
        step(prt, fields, opts)
        prt.track_sample()
        st, tag = TR.raw_state(prt), prt.state_real("raw_tag")
        now = tag_map(st, tag)
        assert all(first[t] == k for t, k in now.items()), "the map tag -> track index is what it was"
        assert_record(prt.track(), s, st, n_tr, (real_t.__name__, "step", s))
        new = tag >= n_tags                                                   # newcomers of a source carry the tags behind the initial ones
        fired += int(new.sum())
        assert (st["track"][new] == 0).all(), "every newcomer has mark 0"
        uniq, cnt = np.unique(tag[st["n"] > 0], return_counts=True)
        if s == 3:
            twice = uniq[cnt == 2]
            recycled = twice.size
            assert (cnt <= 2).all()
            for t in twice:                                                   # donor and receiver carry one tag: one of them the mark, if the donor had it
                marks = st["track"][(tag == t) & (st["n"] > 0)]
                assert (marks != 0).sum() == (1 if int(t) in first else 0), (t, marks)
            assert sum(1 for t in twice if int(t) in first) >= 6, "tracked droplets were among the donors"
        n_tags = max(n_tags, int(tag.max()) + 1)
    info = prt.track_info()
    left = n_first - np.unique(tag[(st["n"] > 0) & (tag < n_first)]).size
    print(real_t.__name__, "tracked", n_tr, "initial droplets gone", left, "newcomers", fired, "recycled", recycled, "scans", info["scans"])
    assert fired >= 96 and recycled > 0, "the source fired and the recycling took place"
    assert left > 150, "droplets died (and their slots were compacted away or recycled)"
    rec = prt.track()
    assert (rec["n"][-1][:n_bot] == 0).all() and (rec["n"][0][:n_bot] > 0).any(), "the lowest level's droplets have left"
    assert (rec["n"][-1][n_bot:n_bot + n_top] > 0).sum() > 10, "the top level's droplets live on"
    assert info["scans"] >= 3, "the storage was permuted again and again: re-ordering every second step, compaction, recycling"


# ---------------------------------------------------------------------------------------------------- 4. nothing else moves
RAW = ("raw_n", "raw_ijk", "raw_x", "raw_y", "raw_z", "raw_rw2", "raw_rd3", "raw_kappa", "raw_vt", "th", "rv")


def whole_state(prt):
    out = {nm: prt.state_u64(nm) if nm in ("raw_n", "raw_ijk") else prt.state_real(nm) for nm in RAW}
    out["puddle"] = np.array(list(prt.diag_puddle().values()))
    try:
        out["raw_sorted_id"] = prt.state_u64("raw_sorted_id")
    except RuntimeError:                                                      # (a re-sort that the next step finishes: no order to compare, on
        out["raw_sorted_id"] = np.zeros(0, dtype=np.uint64)                   # either side; test_nothing_else_moves says where there is one)
    out["mode"] = np.array([int(v) for v in prt.mode()])
    out["coal_kernel"] = prt.state_u64("raw_coal_kernel")
    return out


def plain_box(real_t, strict, **kw):
    oi = h.box_opts(4, 4, 4, 32, **kw)
    if not strict:
        h.api_default_opts(oi)
    th, rv, rhod, Cc = h.box_fields(oi)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    fields = (f(th), f(rv), f(rhod), {k: f(v) for k, v in Cc.items()})
    prt = h.hip_particles(oi, real_t)
    prt.init(fields[0].copy(), fields[1].copy(), fields[2].copy(), **{kk: v.copy() for kk, v in fields[3].items()})
    return prt, fields, oi


CASES = ["fast", "strict", "colliding"]
_twins = {}


def make_case(real_t, case):
    return rainy(real_t, 3, 6, reorder_every=5) if case == "colliding" else plain_box(real_t, case == "strict", reorder_every=5)


def five_steps(real_t, case, tracking):
    """a fresh object of the case, tracking with every = 1 or not, and its whole state after each of five steps.  reorder_every = 5: the
    fifth step re-orders the storage under the tracked droplets, with a sample behind it."""
    prt, fields, oi = make_case(real_t, case)
    h.assert_mode(prt, strict_fp=(case == "strict"))
    if tracking:
        prt.track_enable(500, capacity=8, every=1)
        assert prt.track_select([("all",)], max_count=300) > 100
    opts, out = lgrngn.opts_t(), []
    for s in range(5):
        step(prt, fields, opts)
        out.append(whole_state(prt))
        if case == "colliding":
            assert int(out[-1]["coal_kernel"][0]) == 2, "the production coalescence kernel, tracking or not"
    return prt, fields, oi, out


def twin_runs(real_t, case):
    """two objects from the same options and seed, one tracking, five steps each (made once per parameter set).  Only results that no test
    changes are kept, never the objects: the states after every step, the two snapshots behind the fifth, the tracking object's
    track_info, the untracked object's state after a sixth step, and the fields and options."""
    key = (real_t.__name__, case)
    if key in _twins:
        return _twins[key]
    res, blobs = [], []
    for tracking in (True, False):
        prt, fields, oi, out = five_steps(real_t, case, tracking)
        res.append(out)
        blobs.append(bytes(prt.snapshot()))
        if tracking:
            info = prt.track_info()
    step(prt, fields, lgrngn.opts_t())                                        # the untracked object, behind its snapshot
    _twins[key] = (res, blobs, info, whole_state(prt), fields, oi)
    return _twins[key]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_nothing_else_moves(real_t, case):
    res, blobs, info, sixth, fields, oi = twin_runs(real_t, case)
    for s in range(5):
        for nm in res[0][s]:
            assert np.array_equal(res[0][s][nm], res[1][s][nm]), (case, "step", s, nm)
    # the sorted order can be read only where a step has made it (whole_state): the fast path leaves most re-sorts to the next step's
    # condensation, and there is nothing to compare then; the fifth step re-orders the storage, which needs the order made
    assert res[0][4]["raw_sorted_id"].size > 0, "behind the fifth step there was a sorted order to compare"
    if case == "colliding":
        assert res[0][0]["raw_n"].size != res[0][4]["raw_n"].size or not np.array_equal(res[0][0]["raw_n"], res[0][4]["raw_n"]), "the coalescence did collide"
    assert info["enabled"] == 1 and info["n_samples"] == 5 and info["dropped"] == 0
    assert info["scans"] == 2 if case != "colliding" else 2 <= info["scans"] <= 5, "enable's scan and the re-ordering's; where droplets die, compactions"
    twin = h.hip_particles(oi, real_t)
    twin.track_enable(16)                                                     # (enabled before the load: a restored object is disabled all the same)
    twin.restore(np.frombuffer(blobs[0], dtype=np.uint8))
    assert twin.track_info()["enabled"] == 0 and twin.state_real("raw_track").size == 0
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: track: sample while tracking is not enabled"):
        twin.track_sample()
    step(twin, fields, lgrngn.opts_t())
    b = whole_state(twin)
    for nm in sixth:
        assert np.array_equal(sixth[nm], b[nm]), (case, "restored", nm)


def sections(blob):
    """{name: the line of lcx_snapshot_describe}, and the lines that are no section"""
    lines = lgrngn.snapshot_describe(np.frombuffer(blob, dtype=np.uint8)).splitlines()
    sec = {ln.split()[1].rstrip(":"): ln for ln in lines if ln.startswith("section ")}
    return sec, [ln for ln in lines if not ln.startswith("section ")]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_two_snapshots_are_equal_byte_for_byte(real_t, case):
    """The check as the issue states it: the snapshots of the two objects of twin_runs, byte for byte.

    Two objects are two runs, so this also asks that a snapshot be reproducible from run to run.  The sections `rank` (arrival ranks that
    the last sort's atomics handed out, or the ranking's scratch) and `big_list` (the crowded cells in the order in which atomics listed
    them) were not, tracking or not; snapshot_save copies both in one form (snap_canonical_rank / _list in lcx_core.hip)."""
    res, blobs, info, sixth, fields, oi = twin_runs(real_t, case)
    assert blobs[0] == blobs[1], "the snapshot of a tracking object is that of the same run without tracking, byte for byte"


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_a_snapshot_with_the_scatter_owed_is_reproducible(real_t):
    """the default re-ordering period: after two steps the re-sort's scatter is still owed and `rank` holds LIVE arrival ranks, which the
    snapshot writes in storage order.  Two runs give the same bytes, the object that was snapshotted goes on as one that was not, and so
    does a restored one."""
    opts = lgrngn.opts_t()
    runs = [plain_box(real_t, False) for _ in range(3)]
    blobs = []
    for prt, fields, oi in runs:
        for s in range(2):
            step(prt, fields, opts)
        blobs.append(bytes(prt.snapshot()) if len(blobs) < 2 else None)
    with pytest.raises(RuntimeError, match="the re-sort of the last step has not been finished yet"):
        runs[0][0].state_u64("raw_sorted_id")                                 # the scatter is owed: the case is the one meant
    assert blobs[0] == blobs[1]
    twin = h.hip_particles(runs[0][2], real_t)
    twin.restore(np.frombuffer(blobs[0], dtype=np.uint8))
    states = []
    for p in (runs[0][0], runs[2][0], twin):                                  # snapshotted, never snapshotted, restored
        for s in range(2):
            step(p, runs[0][1], opts)
        states.append(whole_state(p))
    for nm in states[0]:
        assert np.array_equal(states[0][nm], states[1][nm]) and np.array_equal(states[1][nm], states[2][nm]), nm


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_snapshot_does_not_know_the_column(real_t, case):
    res, blobs, info, sixth, fields, oi = twin_runs(real_t, case)
    (sa, ra), (sb, rb) = sections(blobs[0]), sections(blobs[1])
    assert ra == rb and list(sa) == list(sb) and not any("track" in nm for nm in sa), "the same options, scalars and sections; none for the marks"
    for nm in sa:
        assert sa[nm] == sb[nm], nm                                            # (its checksum too; names the section where the test above fails)
    # one object of its own, the very same storage: with the column and with the column dropped, byte for byte -- and the shared run's bytes
    prt = five_steps(real_t, case, True)[0]
    with_column = bytes(prt.snapshot())
    assert with_column == blobs[0]
    assert prt.track_info()["enabled"] == 1 and (prt.state_real("raw_track") != 0).sum() > 100
    prt.track_disable()
    assert bytes(prt.snapshot()) == with_column


# ---------------------------------------------------------------------------------------------------- 5. the slot list is reused
def launches(prt):
    return int(prt.state_u64("raw_launches")[0])


def test_the_slot_list_is_reused():
    oi = h.api_default_opts(h.box_opts(4, 4, 4, 32, reorder_every=6))
    th, rv, rhod, Cc = h.box_fields(oi)
    fields = (th, rv, rhod, Cc)
    prt = h.hip_particles(oi, np.float64)
    prt.init(fields[0].copy(), fields[1].copy(), fields[2].copy(), **{kk: v.copy() for kk, v in fields[3].items()})
    opts = lgrngn.opts_t()
    opts.sedi = opts.coal = False                                             # a periodic box in which nothing dies
    prt.track_enable(200, capacity=16)
    assert prt.track_select([("all",)], max_count=150) > 100
    n_tr = prt.track_info()["n_tracked"]
    assert prt.track_info()["scans"] == 0
    for s in range(5):
        step(prt, fields, opts)
        n0 = launches(prt)
        prt.track_sample()
        assert launches(prt) - n0 == (1 if s else 2), "a sample on unpermuted storage is one launch (the first one behind enable: the scan and the sample)"
        assert prt.track_info()["scans"] == 1, "five samples, one scan: the one that enable owes"
    before = TR.slot_of(TR.raw_state(prt), n_tr)
    step(prt, fields, opts)                                                   # the sixth step re-orders the storage
    after = TR.slot_of(TR.raw_state(prt), n_tr)
    assert not np.array_equal(before, after), "the storage was permuted"
    n0 = launches(prt)
    prt.track_sample()
    assert 1 <= launches(prt) - n0 <= 3, "behind a permutation: the scan and the sample"
    assert prt.track_info()["scans"] == 2
    step(prt, fields, opts)
    prt.track_sample()
    assert prt.track_info()["scans"] == 2
    rec = prt.track()
    assert rec["n"].shape == (7, n_tr) and (rec["n"] > 0).all()
    assert_record(rec, 6, TR.raw_state(prt), n_tr, "behind the re-ordering")
    # enable on an object that has run: the list is stale once, five samples make one scan
    prt.track_enable(64, capacity=8)
    prt.track_select_slots(np.arange(0, 640, 10))
    for s in range(4):                                                        # (steps 8 .. 11: the next re-ordering is step 12's)
        step(prt, fields, opts)
        prt.track_sample()
    assert prt.track_info()["scans"] == 1 and prt.track_info()["n_samples"] == 4


def test_launch_counts():
    never, fields, _ = TMV.rainy_box(np.float64, None)
    n_never = TMV.launches_of_three_steps(never, fields)
    on, fields, _ = TMV.rainy_box(np.float64, None)
    on.track_enable(1000)
    assert on.track_select([("rng", "wet", 10e-6, 1.)]) > 100
    n_on = TMV.launches_of_three_steps(on, fields)
    gone, fields, _ = TMV.rainy_box(np.float64, None)
    gone.track_enable(1000, every=1)
    gone.track_select([("all",)])
    gone.track_disable()
    n_gone = TMV.launches_of_three_steps(gone, fields)
    print("launches per (step_sync, step_async): never enabled", n_never, "enabled, no sample", n_on, "disabled", n_gone)
    assert n_never == n_on, "enabled without a sample: what an object without tracking launches"
    assert n_never == n_gone, "a disabled object launches what a never-enabled one does"
    assert on.track_info()["scans"] == 0


# ---------------------------------------------------------------------------------------------------- 6. automatic sampling and the buffer
@pytest.mark.parametrize("variable_dt", [False, True], ids=["dt", "variable_dt"])
def test_automatic_sampling_and_the_buffer(variable_dt):
    oi = h.api_default_opts(h.box_opts(4, 0, 4, 16, variable_dt_switch=variable_dt))
    th, rv, rhod, Cc = h.box_fields(oi)
    fields = (th, rv, rhod, Cc)
    prt = h.hip_particles(oi, np.float64)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    opts = lgrngn.opts_t()
    opts.coal = opts.sedi = False
    dt = oi.dt
    if variable_dt:
        opts.dt = dt = .25
    prt.track_enable(100, capacity=3, every=2)
    n0 = prt.track_select_slots(np.arange(0, 200, 5))
    assert n0 == 40
    for s in range(10):
        step(prt, fields, opts)
    info = prt.track_info()
    assert (info["n_samples"], info["dropped"], info["every"], info["capacity"]) == (3, 2, 2, 3)
    rec = prt.track()
    assert list(rec["steps"]) == [2, 4, 6] and np.array_equal(rec["time"], np.array([2, 4, 6]) * dt) and rec["n"].shape == (3, 40)
    assert (rec["n"] > 0).all()
    again = prt.track(reset=True)
    assert all(np.array_equal(rec[k], again[k], equal_nan=True) for k in rec)
    info = prt.track_info()
    assert (info["n_samples"], info["dropped"], info["n_tracked"]) == (0, 0, 40), "reset empties the buffer; the tracked set stays"
    assert prt.track()["n"].shape == (0, 40)
    prt.track_sample()                                                        # later samples start at slot 0
    n1 = prt.track_select_slots(np.arange(1, 200, 5))                         # selected between two samples: absent in the earlier one
    assert n1 == 40
    step(prt, fields, opts)                                                   # step 11: no automatic sample
    step(prt, fields, opts)                                                   # step 12: one
    rec = prt.track()
    assert list(rec["steps"]) == [10, 12] and np.array_equal(rec["time"], np.array([10, 12]) * dt) and rec["n"].shape == (2, 80)
    assert (rec["n"][0, :40] > 0).all() and (rec["n"][0, 40:] == 0).all() and all(np.isnan(rec[f][0, 40:]).all() for f in TR.FIELDS[1:])
    assert (rec["n"][1] > 0).all()
    assert_record(rec, 1, TR.raw_state(prt), 80, "the automatic sample is the state at the end of its step")


# ---------------------------------------------------------------------------------------------------- 7. device output, errors, the surface
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_device_output_with_padded_strides(real_t):
    import torch
    prt, fields, oi = rainy(real_t, 2, 6)
    prt.track_enable(64, capacity=4)
    nt = prt.track_select([("rng", "wet", F32(15e-6), 1.)], max_count=50)
    assert nt > 20
    opts = lgrngn.opts_t()
    for s in range(3):
        step(prt, fields, opts)
        prt.track_sample()
    host = prt.track()
    fs, ss = nt + 3, 12 * (nt + 3) + 5
    buf = torch.full((3 * ss,), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    got = prt.track(out=lgrngn.DeviceArray(buf.data_ptr(), (3, 12, nt), (ss, fs, 1)))
    assert set(got) == {"steps", "time"} and list(got["steps"]) == [1, 2, 3]
    flat = buf.cpu().numpy()
    seen = np.zeros(flat.size, dtype=bool)
    for s in range(3):
        for f, nm in enumerate(TR.FIELDS):
            lo = s * ss + f * fs
            assert np.array_equal(flat[lo:lo + nt], host[nm][s], equal_nan=True), (s, nm)
            seen[lo:lo + nt] = True
    assert (flat[~seen] == -1).all(), "the padding is untouched"
    with pytest.raises(ValueError, match="out must be a DeviceArray of shape"):
        prt.track(out=lgrngn.DeviceArray(buf.data_ptr(), (3, 12, nt + 1)))


def test_every_error_text():
    oi = h.api_default_opts(h.box_opts(4, 0, 4, 16))
    th, rv, rhod, Cc = h.box_fields(oi)
    prt = h.hip_particles(oi, np.float64)
    f = lambda name: getattr(prt._lib, "lcx_track_" + name)
    last = prt._f("last_error")
    last.restype = C.c_char_p
    sz, i32 = C.c_size_t, C.c_int
    refused = lambda rc, text: (rc == 1 and last().decode() == text) or pytest.fail("%r, not %r" % (last().decode(), text))
    cl = (lgrngn._diag_clause_c * 5)()
    got, out = sz(), np.zeros((4, 12, 8))
    outp = C.c_void_p(out.ctypes.data)
    slots = (C.c_ulonglong * 2)(0, 1)
    # while not enabled: info answers, everything else but enable and check refuses
    assert prt.track_info() == dict(enabled=0, max_tracked=0, n_tracked=0, capacity=0, n_samples=0, dropped=0, every=0, scans=0)
    for what, call in (("disable", lambda: f("disable")(prt._h)), ("sample", lambda: f("sample")(prt._h)),
                       ("select", lambda: f("select")(prt._h, cl, i32(1), None, sz(1), C.byref(got))),
                       ("select_slots", lambda: f("select_slots")(prt._h, slots, sz(2), C.byref(got))),
                       ("read", lambda: f("read")(prt._h, outp, sz(96), sz(8), None, None, sz(4), C.byref(got), i32(0), i32(0)))):
        refused(call(), "libcloudph++: track: %s while tracking is not enabled (lcx_track_enable)" % what)
    # the ranges of enable
    for mx in (0, (1 << 20) + 1):
        refused(f("enable")(prt._h, sz(mx), sz(4), i32(0)), "libcloudph++: track: max_tracked = %d is outside 1 .. 1048576" % mx)
    refused(f("enable")(prt._h, sz(8), sz(0), i32(0)), "libcloudph++: track: capacity == 0")
    refused(f("enable")(prt._h, sz(8), sz(4), i32(-1)), "libcloudph++: track: every = -1 < 0")
    assert prt.track_info()["enabled"] == 0, "a failed call leaves the object as it was"
    # before init()
    prt.track_enable(8, capacity=4)
    assert prt.track_info() == dict(enabled=1, max_tracked=8, n_tracked=0, capacity=4, n_samples=0, dropped=0, every=0, scans=0)
    refused(f("sample")(prt._h), "libcloudph++: track: sample before init()")
    refused(f("select")(prt._h, cl, i32(1), None, sz(1), C.byref(got)), "libcloudph++: track: select before init()")
    refused(f("select_slots")(prt._h, slots, sz(2), C.byref(got)), "libcloudph++: track: select_slots before init()")
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    assert prt.state_real("raw_track").size == prt.state_u64("raw_n").size and (prt.state_real("raw_track") == 0).all()
    # select
    box = lambda *v: (C.c_double * 6)(*v)
    for k in (0, 5):
        refused(f("select")(prt._h, cl, i32(k), None, sz(1), C.byref(got)), "libcloudph++: track: n_clauses = %d is outside 1 .. 4" % k)
    refused(f("select")(prt._h, None, i32(1), None, sz(1), C.byref(got)), "libcloudph++: track: clause == NULL")
    cl[1].sel = 7
    refused(f("select")(prt._h, cl, i32(2), None, sz(1), C.byref(got)), "libcloudph++: track: clause 1: unknown sel 7")
    refused(f("select")(prt._h, cl, i32(1), box(0, 4, 0, 1, 3, 1), sz(1), C.byref(got)), "libcloudph++: track: box: lo > hi in pair 2")
    refused(f("select")(prt._h, cl, i32(1), box(0, float("inf"), 0, 1, 0, 1), sz(1), C.byref(got)), "libcloudph++: track: box: bound 1 is not finite")
    refused(f("select")(prt._h, cl, i32(1), None, sz(0), C.byref(got)), "libcloudph++: track: max_count == 0")
    assert f("select")(prt._h, cl, i32(1), box(0, 160, 9, 1, float("nan"), 160), sz(1), C.byref(got)) == 1      # (z's pair is read ...
    assert f("select")(prt._h, cl, i32(1), box(0, 160, 9, 1, 0, 160), sz(3), C.byref(got)) == 0 and got.value == 3, "... the pair of the missing y is not"
    refused(f("select_slots")(prt._h, None, sz(2), C.byref(got)), "libcloudph++: track: slot == NULL with n > 0")
    assert prt.track_info()["n_tracked"] == 3
    # read
    assert f("sample")(prt._h) == 0 and f("sample")(prt._h) == 0
    refused(f("read")(prt._h, outp, sz(96), sz(2), None, None, sz(4), C.byref(got), i32(0), i32(0)), "libcloudph++: track: field_stride (2) < n_tracked (3)")
    refused(f("read")(prt._h, outp, sz(95), sz(8), None, None, sz(4), C.byref(got), i32(0), i32(0)), "libcloudph++: track: sample_stride (95) < 12 * field_stride (8)")
    refused(f("read")(prt._h, outp, sz(96), sz(8), None, None, sz(1), C.byref(got), i32(0), i32(0)), "libcloudph++: track: cap_samples (1) < the samples held (2)")
    refused(f("read")(prt._h, None, sz(96), sz(8), None, None, sz(4), C.byref(got), i32(0), i32(0)), "libcloudph++: track: out == NULL with samples to write")
    assert prt.track_info()["n_samples"] == 2
    assert f("read")(prt._h, outp, sz(96), sz(8), None, None, sz(4), C.byref(got), i32(0), i32(1)) == 0 and got.value == 2
    assert (out[:2, 0, :3] > 0).all() and (out[:2, :, 3:] == 0).all() and (out[2:] == 0).all(), "elements in between are not written"
    assert f("read")(prt._h, None, sz(36), sz(3), None, None, sz(0), C.byref(got), i32(0), i32(0)) == 0 and got.value == 0, "nothing held: out may be NULL"
    # the one text that no object of today's options reaches: they use 22 attribute columns at most, MAX_EXT is 24
    import os
    core = open(os.path.join(h.ROOT, "libcloudphxx_amd", "csrc", "lcx_core.hip")).read()
    assert "libcloudph++: track: no free attribute column (all " in core


def test_a_multi_device_object_is_refused(monkeypatch):
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = h.box_opts(4, 4, 4, 16)
    oi.dev_count = 2
    prt = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert prt.dev_count == 2
    for call in (lambda: prt.track_enable(8), prt.track_disable, prt.track_info, prt.track_sample, prt.track, lambda: prt.track_select(),
                 lambda: prt.track_select_slots([0])):
        with pytest.raises(RuntimeError, match=r"libcloudph\+\+: track on a multi-device object is not built"):
            call()


def test_a_slab_with_neighbours_is_refused():
    oi = h.box_opts(4, 4, 4, 16)
    oi.bcond_lft = oi.bcond_rgt = 1                                     # (distmem: the slab's side walls hand droplets to neighbours)
    prt = h.hip_particles(oi)
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: track on a decomposed domain is not built"):
        prt.track_enable(8)
    assert prt.track_info()["enabled"] == 0


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_disable_then_enable_with_another_size(real_t):
    prt, fields, oi = rainy(real_t, 2, 6)
    opts = lgrngn.opts_t()
    prt.track_enable(32, capacity=2, every=1)
    assert prt.track_select([("all",)]) == 32
    step(prt, fields, opts)
    assert prt.track()["n"].shape == (1, 32)
    prt.track_disable()
    assert prt.track_info()["enabled"] == 0 and prt.state_real("raw_track").size == 0
    with pytest.raises(RuntimeError, match="not enabled"):
        prt.track()
    step(prt, fields, opts)
    prt.track_enable(300, capacity=5)
    assert prt.track_info() == dict(enabled=1, max_tracked=300, n_tracked=0, capacity=5, n_samples=0, dropped=0, every=0, scans=0)
    assert (prt.state_real("raw_track") == 0).all()
    st = TR.raw_state(prt)
    slots, idx = TR.select(st, [("water",)], None, 300, 300, 0, real_t)
    assert prt.track_select([("water",)]) == slots.size > 200
    assert_marks(TR.raw_state(prt), slots, idx, "enabled again")
    for s in range(2):
        step(prt, fields, opts)
        prt.track_sample()
        assert_record(prt.track(), s, TR.raw_state(prt), slots.size, "enabled again")
    assert list(prt.track()["steps"]) == [1, 2], "the steps count from the last enable"


def test_a_parcel_tracks():
    oi = lgrngn.opts_init_t()
    oi.dt, oi.sd_conc, oi.n_sd_max = 1., 64, 64
    oi.dry_distros = {(.61, 0.): h.lgrngn_bimodal()}
    oi.coal_switch = oi.sedi_switch = False
    prt = h.hip_particles(oi)
    prt.init(np.array([300.]), np.array([.010]), np.array([1.1]))
    prt.track_enable(16, capacity=4, every=1)
    assert prt.track_select([("all",)], box=(0., 0., 0., 0., 0., 0.), max_count=10) == 10, "no pair of a 0-D object's box is read"
    opts = lgrngn.opts_t()
    opts.coal = opts.sedi = opts.adve = False
    for s in range(2):
        prt.step_sync(opts, np.array([300.]), np.array([.012]), np.array([1.1]))
        prt.step_async(opts)
    rec = prt.track()
    assert rec["n"].shape == (2, 10) and (rec["n"] > 0).all()
    assert all((rec[f] == 0).all() for f in ("x", "y", "z", "cell"))
    assert (rec["rw2"][1] != rec["rw2"][0]).any() and (rec["T"] > 250).all() and (rec["RH"] > .5).all()
    assert_record(rec, 1, TR.raw_state(prt), 10, "parcel")
