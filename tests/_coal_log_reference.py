"""What the tests of the collision log (include/lcx_coal_log.h) need beyond the helpers of the collision rates, with no project code in it:
the boxes of crafted cell occupancies, the bookkeeping of an event list (sorting, bitwise comparison), the replay of a launch's events
against the raw state before and after it, and the reduction of a list to the seven sums of include/lcx_coal_rates.h by its table."""
import numpy as np

import _coal_rates_reference as CR
import _vterm_coal_reference as R

LD = np.longdouble
FIELDS = ("launch", "cell", "slot_d", "slot_r", "col_no", "n_d", "n_r", "rw2_d", "rw2_r", "rw2_new", "rd3_d", "rd3_r", "vt_d", "vt_r")
# super-droplets per cell of a 4 x 4 cell 2-D box: around the wave (64), the window of a ranked cell (256) and the ranked tile (512)
OCC = [0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 257, 511, 513, 1030]
# ... and a box of the same kind without a cell above 256: the kernels that rank for themselves take no order with a larger cell in it
OCC_RANKABLE = [0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 2, 256, 191]
EQUAL_CELLS = (4, 7, 10)                                              # cells whose droplets all carry one multiplicity: every pair is capped at q = 1


def bits(a):
    """the bits of an array of doubles (NaN compares equal to itself)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def occupancy_case(occ, real_t, seed=1, boost=100):
    """the particles of a 4 x 4 box (dx = dz = 1) holding occ[c] droplets in cell c = 4 i + k, in a storage order that is no cell order.
    Positions are unique per droplet, and so is kappa (0.5 + 1e-5 k, which this coalescence neither reads nor writes): a step's periodic
    wrap may round a position in its last bit, so droplets are matched across a re-ordering by kappa.  Radii log-uniform 5 ... 80 um; multiplicities as the production case of the collision rates draws
    them, times `boost` and 63 / (m - 1) for a cell of m droplets (the scale factor of its pairs), so that a third of the pairs or more
    collide wherever the kernel gives the pair an efficiency; in EQUAL_CELLS one large multiplicity for all: prob >> 1, the count is
    capped at n_big / n_small = 1 and the donor is used up."""
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.arange(16), occ)
    j = np.concatenate([np.arange(m) for m in occ]) if sum(occ) else np.zeros(0)
    m_of = np.asarray(occ)[cells]
    N = cells.size
    r = np.exp(rng.uniform(np.log(5e-6), np.log(80e-6), N))
    n = (rng.integers(125000, 500000, N) * boost * 63 // np.maximum(m_of - 1, 1)).astype(np.uint64)
    for c in EQUAL_CELLS:
        n[cells == c] = np.uint64(10 ** 13 // max(occ[c] - 1, 1))
    assert int(n.max()) < 2 ** 50
    x = cells // 4 + (j + 1.) / (m_of + 2.)
    z = cells % 4 + .5
    rd3 = (1e-8 * (1 + np.arange(N) / 7.)) ** 3
    perm = rng.permutation(N)
    args = dict(n=n[perm], rd3=rd3[perm].astype(real_t).astype(np.float64), rw2=((r.astype(LD) ** 2).astype(real_t)).astype(np.float64)[perm],
                kpa=.5 + 1e-5 * np.arange(N), vt=np.full(N, .1), x=x[perm], z=z[perm])
    assert len(set(zip(args["x"].astype(real_t), args["z"].astype(real_t)))) == N, "positions must be unique in the object's type"
    return dict(cells=cells[perm], args=args, pairs=int(sum(m // 2 for m in occ)))


def sort_events(ev):
    """the events ordered by their key (LAUNCH, SLOT_R)"""
    order = np.lexsort((ev["slot_r"], ev["launch"]))
    return {f: np.asarray(ev[f])[order] for f in FIELDS}


def assert_key_unique(ev):
    key = set(zip(ev["launch"], ev["slot_r"]))
    assert len(key) == len(ev["launch"]), "(LAUNCH, SLOT_R) must be a key"


def assert_same_events(a, b, tag=""):
    a, b = sort_events(a), sort_events(b)
    for f in FIELDS:
        assert a[f].shape == b[f].shape and np.array_equal(bits(a[f]), bits(b[f])), (tag, f)


def subset_rows(a, b):
    """for every event of a (by its key) the index of the same event in b; asserts that it is there, bit for bit"""
    where = {k: i for i, k in enumerate(zip(b["launch"], b["slot_r"]))}
    idx = np.array([where[k] for k in zip(a["launch"], a["slot_r"])], dtype=np.int64)
    for f in FIELDS:
        assert np.array_equal(bits(a[f]), bits(np.asarray(b[f])[idx])), f
    return idx


def replay_one_launch(ev, before, after, real_t, strict, collide_bar_eps, tag="", vt="before"):
    """One launch's events against the raw state around it.  before / after: dicts of n (uint64), rw2, rd3, vt (doubles holding the
    object's type) indexed by the storage slot AT THE LAUNCH; after["gone"], optional: slots that the storage no longer holds (used up and
    compacted away: their multiplicity counts as 0 and nothing else of them is compared).  vt: "before" where the launch read the
    velocities that `before` holds; "after" where a velocity pass ran between `before` and the launch (step_async): VT_D is then compared
    with the donor's velocity afterwards, which nothing has touched since, and VT_R with nothing (the receiver's is invalidated).  Checks
    every item of the replay identity and returns the number of events."""
    E = len(ev["launch"])
    D, Rr = ev["slot_d"].astype(np.int64), ev["slot_r"].astype(np.int64)
    nslot = len(before["n"])
    assert ((D >= 0) & (D < nslot) & (Rr >= 0) & (Rr < nslot)).all(), tag
    named = np.concatenate([D, Rr])
    assert len(set(named.tolist())) == 2 * E, (tag, "a slot is named twice")
    gone = after.get("gone", np.zeros(nslot, dtype=bool))
    col_no, nD, nR = (ev[f].astype(np.uint64) for f in ("col_no", "n_d", "n_r"))
    assert (ev["col_no"] >= 1).all() and (ev["n_r"] >= 1).all() and (ev["n_d"] >= ev["n_r"]).all(), tag
    # what the kernel read is what the state held, bit for bit
    assert np.array_equal(nD, before["n"][D]) and np.array_equal(nR, before["n"][Rr]), (tag, "N_D, N_R")
    if vt == "after":
        assert np.array_equal(bits(ev["vt_d"][~gone[D]]), bits(after["vt"][D][~gone[D]])), (tag, "vt_d")
        assert (ev["vt_r"] > 0).all(), (tag, "vt_r")
    for f, col in (("rw2", "rw2"), ("rd3", "rd3")) + ((("vt", "vt"),) if vt == "before" else ()):
        assert np.array_equal(bits(ev[f + "_d"]), bits(before[col][D])), (tag, f + "_d")
        assert np.array_equal(bits(ev[f + "_r"]), bits(before[col][Rr])), (tag, f + "_r")
    # what the kernel stored is what the state holds
    want_nD = nD - col_no * nR
    assert (col_no * nR <= nD).all(), (tag, "the cap")
    n_after_D = np.where(gone[D], np.uint64(0), after["n"][D])
    assert np.array_equal(n_after_D, want_nD), (tag, "n[SLOT_D] after")
    assert not gone[Rr].any() and np.array_equal(after["n"][Rr], nR), (tag, "the receiver keeps its multiplicity")
    assert np.array_equal(bits(after["rw2"][Rr]), bits(ev["rw2_new"])), (tag, "rw2[SLOT_R] after")
    rd3D, rd3R = ev["rd3_d"].astype(real_t), ev["rd3_r"].astype(real_t)
    want_rd3 = (col_no.astype(real_t) * rd3D).astype(real_t) + rd3R                   # (a product and a sum, each rounded to the real type)
    got_rd3 = after["rd3"][Rr].astype(real_t)
    if strict:
        assert np.array_equal(got_rd3, want_rd3), (tag, "rd3[SLOT_R] after, strict_fp")
    else:
        err = np.abs(got_rd3.astype(LD) - want_rd3.astype(LD)) / want_rd3.astype(LD)
        assert (err <= 2 * LD(np.finfo(real_t).eps)).all(), (tag, "rd3[SLOT_R] after", float(err.max()))
    # RW2_NEW against the long-double collide()
    eps_t = LD(np.finfo(real_t).eps)
    worst = LD(0)
    for i in range(E):
        out = R.collide(int(nD[i]), int(nR[i]), ev["rw2_d"][i], ev["rw2_r"][i], ev["rd3_d"][i], ev["rd3_r"][i], int(col_no[i]))
        assert out["a_is_big"] and out["count"] == int(col_no[i]), (tag, i)
        worst = max(worst, abs(LD(ev["rw2_new"][i]) - out["rw2b"]) / out["rw2b"] / eps_t)
    print("%-40s events %5d  RW2_NEW against collide(): worst %.2f eps (bar %.0f)" % (tag, E, float(worst), collide_bar_eps))
    assert worst <= collide_bar_eps, (tag, float(worst))
    # nothing else moved
    live = before["n"] > 0
    untouched = live.copy()
    untouched[named] = False
    assert not gone[untouched].any(), (tag, "a live slot that no event names is still there")
    for col in ("rw2", "rd3"):
        assert np.array_equal(bits(after[col][untouched]), bits(before[col][untouched])), (tag, col, "of a slot that no event names")
        assert np.array_equal(bits(after[col][D][~gone[D]]), bits(before[col][D][~gone[D]])), (tag, col, "of a donor")
    assert np.array_equal(after["n"][untouched], before["n"][untouched]), (tag, "n of a slot that no event names")
    changed = live & ~gone & (bits(after["rw2"]) != bits(before["rw2"]))
    assert int(changed.sum()) == E, (tag, "live slots whose rw2 changed", int(changed.sum()), E)
    return E


def expected_after(before, ev):
    """n and rw2 by slot as one launch's events leave them, from the state before it"""
    n, rw2 = before["n"].copy(), before["rw2"].copy()
    D, Rr = ev["slot_d"].astype(np.int64), ev["slot_r"].astype(np.int64)
    n[D] -= ev["col_no"].astype(np.uint64) * ev["n_r"].astype(np.uint64)
    rw2[Rr] = ev["rw2_new"]
    return n, rw2


def live_multiset(n, rw2):
    """the living droplets as a sorted list of (n, bits of rw2): what a re-ordering and a compaction leave alone"""
    keep = n > 0
    return sorted(zip(n[keep].tolist(), bits(rw2[keep]).tolist()))


def reduce_to_rates(ev, lo, n_cell):
    """the seven sums of include/lcx_coal_rates.h from an event list, by the header's table: a _coal_rates_reference.Sums (numbers as
    Python integers, M3 in long double with the sum of |term| and the events per cell).  lo: the threshold's bound in the object's type."""
    s = CR.Sums(n_cell)
    lo = LD(lo)
    for i in range(len(ev["launch"])):
        c, cnt, m = int(ev["cell"][i]), int(ev["col_no"][i]), int(ev["n_r"][i])
        rw2D, rw2R, new = LD(ev["rw2_d"][i]), LD(ev["rw2_r"][i]), LD(ev["rw2_new"][i])
        rainD, rainR = rw2D >= lo, rw2R >= lo
        rainP = rainD or rainR or new >= lo
        rD3, rR3 = rw2D * np.sqrt(rw2D), rw2R * np.sqrt(rw2R)

        def add_m3(w, term):
            s.m3[w, c] += term
            s.abs_m3[w, c] += abs(term)
        if not rainD and not rainR and not rainP:
            s.num[5][c] += cnt * m; s.rows["cc->c"] += 1
        elif not rainD and not rainR:
            add_m3(0, m * (cnt * rD3 + rR3)); s.num[1][c] += (cnt + 1) * m; s.num[2][c] += m; s.rows["cc->r"] += 1
        elif not rainD:
            add_m3(3, cnt * m * rD3); s.num[4][c] += cnt * m; s.rows["cr"] += 1
        elif not rainR:
            add_m3(3, m * rR3); s.num[4][c] += m; s.num[6][c] += (cnt - 1) * m; s.rows["rc"] += 1
        else:
            s.num[6][c] += cnt * m; s.rows["rr"] += 1
        s.events[c] += 1
    return s
