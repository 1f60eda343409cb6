"""The particle dump (include/lcx_dump.h) on the device, in double and float, against tests/_dump_reference.py (plain numpy over the raw
state).  Every field is a stored value converted to double: every comparison is np.array_equal(..., equal_nan=True).

1. Records are the raw state: 2-D and 3-D, condensation + coalescence + the move, every field after each of four steps.
2. Tile, wave and workgroup edges of the compaction: ten storage extents, dead slots, five patterns of qualifiers.
3. The selection: the clause cases of the track test, marked droplets, max_count around Q, the count-only call.
4. Nothing moves: two objects from one set-up, one of them dumping all the time.
5. Optional columns: the chemical masses and the in-cloud time, and their refusal.
6. Output forms and errors: padded device output, every error text, a multi-device object, a slab with neighbours, a parcel.
"""
import ctypes as C

import numpy as np
import pytest

import _harness as h
import _dump_reference as DR
import test_hip_track as TT
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

REALS = [np.float64, np.float32]
REAL_IDS = ["f64", "f32"]
F32 = TT.F32
ALL = [("all",)]


def assert_dump(got, st, slots, fields, tag):
    want = DR.record(st, slots, fields)
    for f in fields:
        assert got[f].dtype == np.float64 and got[f].shape == (slots.size,), (tag, f, got[f].shape, slots.size)
        assert np.array_equal(got[f], want[f], equal_nan=True), (tag, f, np.flatnonzero(~((got[f] == want[f]) | (np.isnan(got[f]) & np.isnan(want[f]))))[:8])


# ---------------------------------------------------------------------------------------------------- 1. records are the raw state
@pytest.mark.parametrize("dims", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_records_are_the_raw_state(real_t, dims):
    n = 8 if dims == 2 else 6
    prt, fields, oi = TT.rainy(real_t, dims, n)
    h.assert_mode(prt, strict_fp=False)
    opts = lgrngn.opts_t()                                                    # everything on: condensation, coalescence, advection, sedimentation
    n0 = int((prt.state_u64("raw_n") > 0).sum())
    left = 0
    for s in range(4):
        TT.step(prt, fields, opts)
        st = DR.raw(prt)                                                      # the raw arrays, then the dump, then the compacting reads
        got = prt.dump(ALL, fields=DR.BASE)
        assert prt.state_u64("raw_n").size == st["n"].size, "the dump has not compacted"
        DR.cells(prt, st)
        Q, stride, slots = DR.written(st, ALL, None, None, real_t)
        assert (got["n_qualifying"], got["stride"]) == (Q, 1) and Q == int((st["n"] > 0).sum())
        assert np.array_equal(got["slot"], slots.astype(np.float64)) and (np.diff(got["slot"]) > 0).all(), "slots come out ascending"
        assert_dump(got, st, slots, DR.BASE, (real_t.__name__, dims, s))
        assert (got["n"] > 0).all() and (got["track"] == 0).all()
        assert not np.isnan(got["T"]).any()
        if dims == 2:
            assert (got["y"] == 0).all()
        left = n0 - Q
    assert left > 0, "droplets have left through the bottom (or were collected) and are absent: %d" % left
    assert (st["n"] == 0).any() or st["n"].size < n0


# ---------------------------------------------------------------------------------------------------- 2. tile, wave and workgroup edges
EXTENTS = (1, 63, 64, 65, 255, 257, 2047, 2048, 2049, 3 * 2048 + 65)
R_IN, R_OUT = 30e-6, 5e-6
EDGE_FIELDS = ("slot", "n", "rw2", "rd3", "x", "z", "cell", "kappa", "vt", "T")


def edge_patterns(N):
    """name -> the slots whose radius is R_IN (the clause's range), before the dead ones are taken out"""
    idx = np.arange(N)
    pats = {"nothing": idx[:0], "everything": idx, "last_slot": idx[N - 1:], "last_partial_wave": idx[(N - 1) // 64 * 64:]}
    for m in (1, 32):                                                         # wave m has no qualifier, waves m - 1 and m + 1 have (m = 32: the
        if N > (m + 1) * 64:                                                  # first wave of the second tile)
            pats["hole_at_wave_%d" % m] = idx[((idx // 64 == m - 1) | (idx // 64 == m + 1))]
    return pats


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_tile_wave_and_workgroup_edges(real_t):
    oi = h.api_default_opts(h.box_opts(4, 0, 4, 16, dx=1., n_sd_max=3 * 2048 + 65 + 64))
    th, rv, rhod, Cc = h.box_fields(oi)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    prt = h.hip_particles(oi, real_t)
    prt.init(f(th), f(rv), f(rhod), **{k: f(v) for k, v in Cc.items()})
    wet = [("rng", "wet", F32(20e-6), F32(40e-6))]
    seen = set()
    for N in EXTENTS:
        rng = np.random.default_rng(N)
        dead = np.arange(5, N, 97)
        for name, inside in edge_patterns(N).items():
            seen.add(name)
            mult = rng.integers(1, 1000, N).astype(np.uint64)
            mult[dead] = 0
            r = np.full(N, R_OUT)
            r[inside] = R_IN
            rw2 = (r.astype(np.longdouble) ** 2).astype(real_t).astype(np.float64)
            prt.set_particles(n=mult, rd3=(1e-8 * (1 + np.arange(N) / 7.)) ** 3, rw2=rw2, kpa=np.full(N, .5), vt=np.full(N, .1),
                              x=rng.uniform(.05, 3.95, N), z=rng.uniform(.05, 3.95, N))
            st = DR.raw(prt)
            assert st["n"].size == N, "the storage extent is what set_particles gave"
            clauses = ALL if name == "everything" else wet
            got = prt.dump(clauses, fields=EDGE_FIELDS)
            count = prt.dump_count(clauses)
            g2 = prt.dump(clauses, fields=("slot", "n"), max_count=3)         # the stride rule across the same edges
            assert prt.state_u64("raw_n").size == N
            DR.cells(prt, st)
            Q, stride, slots = DR.written(st, clauses, None, None, real_t)
            want = np.setdiff1d(inside, dead)
            assert np.array_equal(slots, want), (N, name)
            assert (got["n_qualifying"], count, got["slot"].size) == (Q, Q, Q) and got["stride"] == (1 if Q else 0), (N, name, got["n_qualifying"], Q)
            assert_dump(got, st, slots, EDGE_FIELDS, (real_t.__name__, N, name))
            Q2, stride2, slots2 = DR.written(st, clauses, None, 3, real_t)
            assert (g2["n_qualifying"], g2["stride"]) == (Q, stride2) and np.array_equal(g2["slot"], slots2.astype(np.float64)), (N, name)
            assert np.array_equal(g2["n"], st["n"][slots2].astype(np.float64)), (N, name)
    assert seen == {"nothing", "everything", "last_slot", "last_partial_wave", "hole_at_wave_1", "hole_at_wave_32"}


# ---------------------------------------------------------------------------------------------------- 3. the selection
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_selection(real_t):
    prt, fields, oi = TT.rainy(real_t, 3, 6, kappas=(.3, .5, .7))
    dead = np.arange(5, 3456, 97)                                             # dead slots in the middle of the storage
    st0 = DR.raw(prt)
    mult = st0["n"].copy()
    mult[dead] = 0
    prt.set_particles(n=mult, rd3=st0["rd3"], rw2=st0["rw2"], kpa=st0["kappa"], vt=st0["vt"], x=st0["x"], y=st0["y"], z=st0["z"])
    prt.track_enable(4000)
    assert prt.track_select([("rng", "wet", F32(20e-6), F32(40e-6))], max_count=300) > 100      # marked droplets qualify like any other
    wet, dry, kap = ("rng", "wet", F32(20e-6), F32(40e-6)), ("rng", "dry", F32(1e-8), F32(3e-6)), ("rng", "kappa", F32(.4), F32(.6))
    box = (1.5, 4.25, 0., 3., 2., 6.)
    cases = [([wet], None), ([dry], None), ([kap], None), ([("water",)], None), ([("all",)], None), ([wet, kap], None), ([("all",), dry, ("water",), kap], box),
             ([("all",)], box), ([wet], box)]
    st = DR.cells(prt, DR.raw(prt))                                           # (nothing steps below: one state serves every case; no slot is dead AND compacted --
    assert st["n"].size == 3456 and (st["n"][dead] == 0).all()                # set_particles' extent stays while nothing compacts)
    assert (st["track"] > 0).sum() > 100
    fl = ("slot", "n", "track", "rw2", "rd3", "kappa", "x", "y", "z", "cell", "rv")
    for clauses, bx in cases:
        Q, _, _ = DR.written(st, clauses, bx, None, real_t)
        assert 8 < Q < (st["n"] > 0).sum() or clauses[0][0] in ("all", "water"), (clauses, Q)
        assert prt.dump_count(clauses, box=bx) == Q, (clauses, bx)
        for max_count in (Q + 3, Q, Q - 1, 7, None):                          # Q < room, Q == room, Q > room (strides 2 and above), everything
            Qw, stride, slots = DR.written(st, clauses, bx, max_count, real_t)
            got = prt.dump(clauses, box=bx, fields=fl, max_count=max_count)
            assert (got["n_qualifying"], got["stride"]) == (Q, stride), (clauses, bx, max_count, got["stride"], stride)
            assert got["slot"].size == (Q if max_count is None or max_count >= Q else -(-Q // -(-Q // max_count)))
            assert_dump(got, st, slots, fl, (clauses, bx, max_count))
        marks = prt.dump(clauses, box=bx, fields=("track", "slot"))
        assert np.array_equal(marks["track"], st["track"][marks["slot"].astype(np.int64)])
        if bx is None and clauses == [wet]:
            assert (marks["track"] > 0).sum() > 100, "the marks come out with their droplets"
    assert prt.state_u64("raw_n").size == 3456 and prt.track_info()["scans"] <= 1, "no dump compacted or made the slot list stale"


# ---------------------------------------------------------------------------------------------------- 4. nothing moves
def whole_state(prt):
    out = {nm: prt.state_u64(nm) if nm in ("raw_n", "raw_ijk") else prt.state_real(nm) for nm in TT.RAW + ("raw_track",)}
    out["puddle"] = np.array(list(prt.diag_puddle().values()))
    out["mode"] = prt.state_u64("raw_mode")
    out["scans"] = np.array([prt.track_info()["scans"]])
    return out


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_nothing_moves(real_t):
    runs = []
    for dumping in (True, False):
        prt, fields, oi = TT.rainy(real_t, 3, 6, reorder_every=5)
        prt.track_enable(500, capacity=8, every=1)
        assert prt.track_select(ALL, max_count=300) > 100
        th, rv, rhod, Cc = fields
        opts, states, per_step, uncompacted = lgrngn.opts_t(), [], [], 0
        for s in range(6):
            n0 = TT.launches(prt)
            prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
            if dumping and s < 5:
                a = prt.dump([("rng", "wet", F32(10e-6), 1.)], fields=lgrngn.DUMP_FIELDS[:14])          # between step_sync and step_async
                assert a["n_qualifying"] > 0
            prt.step_async(opts)
            per_step.append(TT.launches(prt) - n0)
            if dumping and s < 5:
                raw_n = prt.state_u64("raw_n")
                b = prt.dump(ALL, fields=("n", "slot"), max_count=50)
                c = prt.dump_count([("water",)], box=(0., 6., 0., 6., 0., 3.))
                d = prt.dump(ALL)
                assert b["stride"] > 1 and 0 < c < d["n_qualifying"] == int((raw_n > 0).sum())
                after = prt.state_u64("raw_n")
                assert after.size == raw_n.size and np.array_equal(after, raw_n), "a dump right after a step returns without compacting"
                uncompacted += int((raw_n == 0).any())
            states.append(whole_state(prt))
        if dumping:
            assert uncompacted > 0, "at least one step left dead slots behind, and the dumps left them there"
        runs.append((states, per_step, bytes(prt.snapshot())))
    (sa, la, ba), (sb, lb, bb) = runs
    for s in range(6):
        for nm in sa[s]:
            assert np.array_equal(sa[s][nm], sb[s][nm], equal_nan=True), ("step", s, nm)
    assert ba == bb, "the snapshot of the dumping object is that of the other, byte for byte"
    assert la[5] == lb[5], "a step with no dump in it launches what it launches without any dump before it: %r, %r" % (la, lb)
    assert all(x > y for x, y in zip(la[:5], lb[:5])), "(the steps with a dump between step_sync and step_async count its launches)"
    assert sa[0]["raw_n"].size != sa[5]["raw_n"].size or not np.array_equal(sa[0]["raw_n"], sa[5]["raw_n"]), "the coalescence did collide"


# ---------------------------------------------------------------------------------------------------- 5. optional columns
CHEM = ("chem_hno3", "chem_nh3", "chem_co2", "chem_so2", "chem_h2o2", "chem_o3", "chem_s_vi", "chem_h")


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_chemical_masses(real_t):
    import test_hip_chemistry as TCH
    b = TCH.Box((3, 4), 24, real_t=real_t, mode="fast", cond_steps=3)
    o = b.opts(chem_dsl=True, chem_dsc=True, chem_rct=True)
    for _ in range(2):
        b.step(o)
    prt = b.p
    got = prt.dump([("rng", "wet", F32(1e-6), 1.)], fields=("slot", "n") + CHEM)
    every = prt.dump(ALL, fields=CHEM + ("slot",))
    # nothing dies in this box (no sedimentation, no coalescence): the storage holds no dead slot, the read below does not permute it and
    # a raw_-free name shows the column in storage order
    assert prt.state_u64("raw_n").size == prt.n_part == every["n_qualifying"] == 3 * 4 * 24
    slots = got["slot"].astype(np.int64)
    assert 10 < slots.size < prt.n_part, "a true subset: %d of %d" % (slots.size, prt.n_part)
    for f, nm in zip(CHEM, TCH.NAMES):
        col = prt.state_real("chem_" + nm)
        assert np.array_equal(got[f], col[slots]) and np.array_equal(every[f], col), f
    assert (got["chem_s_vi"] > 0).all() and (every["chem_so2"] > 0).any()
    assert np.array_equal(got["n"], prt.state_u64("n").astype(np.float64)[slots])


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_incloud_time(real_t):
    prt, fields, oi = TT.plain_box(real_t, False, diag_incloud_time=True, coal_switch=False, sedi_switch=False)
    opts = lgrngn.opts_t()
    opts.coal = opts.sedi = False
    for s in range(3):
        TT.step(prt, fields, opts)
    got = prt.dump([("rng", "wet", F32(.5e-6), 1.)], fields=("incloud_time", "slot", "rw2"))
    assert prt.state_u64("raw_n").size == prt.n_part, "nothing died: the read below shows the column in storage order"
    slots = got["slot"].astype(np.int64)
    col = prt.state_real("incloud_time")
    assert slots.size > 10 and np.array_equal(got["incloud_time"], col[slots]) and np.array_equal(got["rw2"], prt.state_real("raw_rw2")[slots])
    assert (col > 0).any() and (got["incloud_time"] > 0).any(), "activated droplets have spent time in cloud"


def test_optional_fields_are_refused_without_their_option():
    prt, fields, oi = TT.plain_box(np.float64, False)
    for f in CHEM:
        with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: dump: field 1: a chemistry field, but opts_init.chem_switch is off$"):
            prt.dump(ALL, fields=("n", f))
    with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: dump: field 0: incloud_time, but opts_init.diag_incloud_time is off$"):
        prt.dump(ALL, fields=("incloud_time",))


# ---------------------------------------------------------------------------------------------------- 6. output forms and errors
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_device_output_with_padded_strides(real_t):
    import torch
    prt, fields, oi = TT.rainy(real_t, 2, 6)
    TT.step(prt, fields, lgrngn.opts_t())
    clauses, fl = [("rng", "wet", F32(15e-6), 1.)], ("n", "z", "rw2", "slot", "RH")
    host = prt.dump(clauses, fields=fl)
    Q = host["n_qualifying"]
    assert Q > 40
    for max_count in (Q + 5, 17):                                             # everything fits and elements stay free; the stride rule
        fs = max_count + 3
        buf = torch.full((len(fl) * fs + 2,), -1., dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        got = prt.dump(clauses, fields=fl, max_count=max_count, out=lgrngn.DeviceArray(buf.data_ptr(), (len(fl), max_count), (fs, 1)))
        stride = -(-Q // max_count)
        nw = -(-Q // stride)
        assert got == {"n_qualifying": Q, "stride": stride, "n_written": nw}
        flat = buf.cpu().numpy()
        seen = np.zeros(flat.size, dtype=bool)
        for f, nm in enumerate(fl):
            assert np.array_equal(flat[f * fs:f * fs + nw], host[nm][::stride], equal_nan=True), (max_count, nm)
            seen[f * fs:f * fs + nw] = True
        assert (flat[~seen] == -1).all(), "the padding and the elements beyond n_written are untouched"
        again = prt.dump(clauses, fields=fl, max_count=max_count)             # host output: the same bits
        assert all(np.array_equal(again[nm], host[nm][::stride], equal_nan=True) for nm in fl) and again["stride"] == stride


def test_every_error_text():
    oi = h.api_default_opts(h.box_opts(4, 0, 4, 16))
    th, rv, rhod, Cc = h.box_fields(oi)
    prt = h.hip_particles(oi, np.float64)
    dump = prt._lib.lcx_dump
    last = prt._f("last_error")
    last.restype = C.c_char_p
    sz, i32 = C.c_size_t, C.c_int
    refused = lambda rc, text: (rc == 1 and last().decode() == text) or pytest.fail("%r, not %r" % (last().decode(), text))
    cl = (lgrngn._diag_clause_c * 5)()
    ints = lambda *v: (C.c_int * len(v))(*v)
    q, w, st = sz(), sz(), C.c_ulonglong()
    out = np.full((3, 64), -1.)
    outp = C.c_void_p(out.ctypes.data)
    call = lambda clause=cl, nc=1, box=None, field=ints(0, 4), nf=2, o=outp, fs=64, mc=64: dump(
        prt._h, clause, i32(nc), box, field, i32(nf), o, sz(fs), sz(mc), i32(0), C.byref(q), C.byref(w), C.byref(st))
    refused(call(), "libcloudph++: dump: called before init()")
    with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: dump: called before init\(\)$"):
        prt.dump_count()
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    before = DR.raw(prt)
    box = lambda *v: (C.c_double * 6)(*v)
    for k in (0, 5):
        refused(call(nc=k), "libcloudph++: dump: n_clauses = %d is outside 1 .. 4" % k)
    refused(call(clause=None), "libcloudph++: dump: clause == NULL")
    cl[1].sel = 7
    refused(call(nc=2), "libcloudph++: dump: clause 1: unknown sel 7")
    refused(call(box=box(0, 4, 0, 1, 3, 1)), "libcloudph++: dump: box: lo > hi in pair 2")
    refused(call(box=box(0, float("inf"), 0, 1, 0, 1)), "libcloudph++: dump: box: bound 1 is not finite")
    for k in (0, 24):
        refused(call(nf=k), "libcloudph++: dump: n_fields = %d is outside 1 .. 23" % k)
    refused(call(field=None), "libcloudph++: dump: field == NULL")
    refused(call(field=ints(0, 23)), "libcloudph++: dump: field 1: unknown field 23")
    refused(call(field=ints(4, 4)), "libcloudph++: dump: field 1: field 4 is given twice")
    refused(call(field=ints(0, 15)), "libcloudph++: dump: field 1: a chemistry field, but opts_init.chem_switch is off")
    refused(call(field=ints(14, 0)), "libcloudph++: dump: field 0: incloud_time, but opts_init.diag_incloud_time is off")
    refused(call(mc=0), "libcloudph++: dump: max_count == 0")
    refused(call(fs=63), "libcloudph++: dump: field_stride (63) < max_count (64)")
    assert (out == -1).all(), "a refused call writes nothing"
    assert call(box=box(0, 160, 9, 1, float("nan"), 160)) == 1                                # (z's pair is read ...
    assert call(box=box(0, 160, 9, 1, 0, 160), mc=3, fs=64) == 0 and (q.value, w.value) == (256, 3), "... the pair of the missing y is not"
    assert st.value == 86 and (out[:2, :3] >= 0).all() and (out[:2, 3:] == -1).all() and (out[2] == -1).all(), "elements beyond n_written are not written"
    assert call(o=None, mc=0, fs=0) == 0 and (q.value, w.value, st.value) == (256, 0, 0), "out == NULL: the call only counts, neither number is read"
    assert dump(prt._h, cl, i32(1), None, ints(0), i32(1), outp, sz(64), sz(64), i32(0), None, None, None) == 0, "any of the three results may be NULL"
    after = DR.raw(prt)
    assert all(np.array_equal(before[k], after[k]) for k in before if k != "has")


def test_a_multi_device_object_is_refused(monkeypatch):
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = h.box_opts(4, 4, 4, 16)
    oi.dev_count = 2
    prt = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert prt.dev_count == 2
    for call in (prt.dump, prt.dump_count, lambda: prt.dump(max_count=4)):
        with pytest.raises(RuntimeError, match=r"^libcloudph\+\+: dump on a multi-device object is not built$"):
            call()


def test_a_slab_with_neighbours_dumps_its_raw_state():
    oi = h.box_opts(6, 0, 5, 24, dx=20., coal_switch=False)
    oi.n_sd_max = 24 * 6 * 5 * 3
    th, rv, rhod, Cc = h.box_fields(oi)
    ring = h.LocalRing(oi, 2, h.hip_particles, h.dev_alloc)
    ring.init(th.copy(), rv.copy(), rhod.copy(), **Cc)
    opts = lgrngn.opts_t()
    opts.coal = False
    fl = ("slot", "n", "x", "z", "rw2", "rd3", "cell", "vt")
    for it in range(3):
        ring.step(opts, th.copy(), rv.copy(), rhod.copy(), **Cc)
        for r, prt in enumerate(ring.prts):
            assert prt.opts_init.bcond_lft == 1 and prt.opts_init.bcond_rgt == 1, "a slab with neighbours on both sides"
            st = DR.raw(prt)
            x0, x1 = prt.opts_init.x0, prt.opts_init.x1
            bx = (x0, (x0 + x1) / 2, 0., 0., 0., 60.)
            for clauses, b in ((ALL, None), ([("water",)], bx)):
                got = prt.dump(clauses, box=b, fields=fl)
                Q, stride, slots = DR.written(st, clauses, b, None, np.float64)
                assert Q > 20 and got["n_qualifying"] == Q
                assert_dump(got, st, slots, fl, ("slab", r, it))
            assert prt.state_u64("raw_n").size == st["n"].size


def test_a_parcel_dumps():
    oi = lgrngn.opts_init_t()
    oi.dt, oi.sd_conc, oi.n_sd_max = 1., 64, 64
    oi.dry_distros = {(.61, 0.): h.lgrngn_bimodal()}
    oi.coal_switch = oi.sedi_switch = False
    prt = h.hip_particles(oi)
    prt.init(np.array([300.]), np.array([.010]), np.array([1.1]))
    opts = lgrngn.opts_t()
    opts.coal = opts.sedi = opts.adve = False
    for s in range(2):
        prt.step_sync(opts, np.array([300.]), np.array([.012]), np.array([1.1]))
        prt.step_async(opts)
    st = DR.raw(prt)
    got = prt.dump(ALL, box=(0., 0., 0., 0., 0., 0.), fields=DR.BASE, max_count=10)
    DR.cells(prt, st)
    Q, stride, slots = DR.written(st, ALL, None, 10, np.float64)
    assert (got["n_qualifying"], got["stride"], got["n"].size) == (64, 7, 10), "no pair of a 0-D object's box is read"
    assert all((got[f] == 0).all() for f in ("x", "y", "z", "cell", "track"))
    assert (got["T"] > 250).all() and (got["RH"] > .5).all()
    assert_dump(got, st, slots, DR.BASE, "parcel")
