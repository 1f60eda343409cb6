"""Collision rates per cell (include/lcx_coal_rates.h) in numpy long double and Python integers: a walk over one coalescence launch, pair
by pair, from the state before it, the cell-sorted order it paired up and the random numbers it drew.  No project code: the kernel, the
pair probability, the scale factor and collide() come from tests/_vterm_coal_reference.py (written from the reference's sources).

A pair is an event only where its count is beyond the reach of rounding, and the walk asserts that itself.  With `rel` the relative
uncertainty of the device's probability against the long-double one (the caller's: what its velocities and its kernel can differ by), a
pair must be in one of two regimes:
  free     prob (1 + rel) < 0.5 and the random number clear of it: u < prob (1 - rel) -- one collision -- or u > prob (1 + rel) -- none;
  capped   prob (1 - rel) > 2 q with q = n_big / n_small: the count is q whatever u is (q = 1 with equal multiplicities uses the donor up).
The class of both members and of the product (rw2 < lo: cloud) must be clear of lo by `class_margin` (relative).

The seven sums follow the header's table: D the member with the larger or equal multiplicity (the pair's first on a tie), R the other,
m = R's multiplicity; a receiver without droplets (m = 0) moves nothing."""
import numpy as np

from _vterm_coal_reference import LD, collide, kernel, prob, scale_factor   # noqa: F401  (scale_factor: through prob)

NAMES = ("acnv_m3", "acnv_nc", "acnv_nr", "accr_m3", "accr_nc", "self_cloud_n", "self_rain_n")
M3_ROWS = (0, 3)
ROWS = ("cc->c", "cc->r", "cr", "rc", "rr")            # donor class, receiver class (and the product's, of two cloud droplets)


def cell_sorted_order(ijk, keys):
    """the order a launch pairs up: by cell, inside a cell by the shuffle key, the lower id first on a tie"""
    ids = np.arange(len(ijk))
    return ids[np.lexsort((ids, np.asarray(keys), np.asarray(ijk)))]


class Sums:
    """what a walk adds up: exact integers, long-double M3 sums with the sum of |term| and the events of each cell"""

    def __init__(self, n_cell):
        self.n_cell = n_cell
        self.num = [[0] * n_cell for _ in NAMES]                      # Python integers (the M3 rows stay 0)
        self.m3 = np.zeros((len(NAMES), n_cell), dtype=LD)
        self.abs_m3 = np.zeros((len(NAMES), n_cell), dtype=LD)        # sum |term|
        self.loose_m3 = np.zeros((len(NAMES), n_cell), dtype=LD)      # ... of the terms with a member that grew earlier in the same walk chain
        self.events = np.zeros(n_cell, dtype=np.int64)                # events that added an M3 term or a number
        self.rows = {r: 0 for r in ROWS}

    def value(self, w, c):
        return self.m3[w, c] if w in M3_ROWS else self.num[w][c]


def walk(sums, real_t, name, state, ijk, order, u01, dt, dv, lo, rel=1e-6, class_margin=None, grown=None, kernel_kw=None, pick=None):
    """One launch.  state: dict of n (uint64), rw2, rd3, vt (real_t) by id -- changed in place to the state after it (the product's rw2 and
    rd3 rounded to real_t from long double, vt of a grown droplet set to -1).  order: ids in cell-sorted order; u01: by position (the
    pair's first), or None with pick(position, prob_lo, prob_hi, q) -> u, which then fills and returns the array that was drawn.
    grown: boolean array by id, droplets whose rw2 the device holds with its own rounding (they grew earlier in the chain); updated.
    rel: a scalar or a function(a, b) -> the pair's relative uncertainty."""
    eps_t = LD(np.finfo(real_t).eps)
    class_margin = 64 * eps_t if class_margin is None else class_margin
    kernel_kw = kernel_kw or {}
    n, rw2, rd3, vt = state["n"], state["rw2"], state["rd3"], state["vt"]
    grown = np.zeros(len(n), dtype=bool) if grown is None else grown
    lo_ld = LD(real_t(lo))
    drawn = np.full(len(order), .5) if u01 is None else None
    cells = np.asarray(ijk)[order]
    assert (np.diff(cells.astype(np.int64)) >= 0).all(), "the order must be sorted by cell"
    start = np.searchsorted(cells, np.arange(sums.n_cell), side="left")
    end = np.searchsorted(cells, np.arange(sums.n_cell), side="right")

    def cls(x, what):
        x = LD(x)
        assert abs(x - lo_ld) > class_margin * lo_ld, ("a radius too close to the threshold", what, float(x), float(lo_ld))
        return x >= lo_ld                                             # True: rain

    for c in range(sums.n_cell):
        N = int(end[c] - start[c])
        for p in range(int(start[c]), int(start[c]) + N - 1, 2):
            a, b = int(order[p]), int(order[p + 1])
            g = lambda arr, i: arr[i:i + 1]
            K = kernel(name, real_t, g(n, a), g(n, b), g(rw2, a), g(rw2, b), g(vt, a), g(vt, b), **kernel_kw)[0]
            pr = prob(LD(real_t(dt)), LD(dv[c]), N, K)
            r = rel(a, b) if callable(rel) else rel
            p_lo, p_hi = pr * (1 - LD(r)), pr * (1 + LD(r))
            na, nb = int(n[a]), int(n[b])
            nB, nS = max(na, nb), min(na, nb)
            q = nB // nS if nS > 0 else None
            if u01 is None:
                drawn[p] = pick(p, p_lo, p_hi, q)
            u = LD(real_t(drawn[p] if u01 is None else u01[p]))
            if q is not None and p_lo > 2 * q:
                cnt_drawn = q                                         # (anything >= q: collide() caps it)
            else:
                assert p_hi < .5, ("a pair in neither regime", c, p, float(pr), q)
                assert u < p_lo or u > p_hi, ("a random number within reach of the probability", c, p, float(u), float(pr))
                cnt_drawn = 1 if u < p_lo else 0
            if cnt_drawn == 0:
                continue
            out = collide(na, nb, rw2[a], rw2[b], rd3[a], rd3[b], cnt_drawn)
            cnt = out["count"]
            D, R = (a, b) if out["a_is_big"] else (b, a)
            m = int(n[R])
            rw2_new = real_t(out["rw2b"] if out["a_is_big"] else out["rw2a"])
            rd3_new = real_t(out["rd3b"] if out["a_is_big"] else out["rd3a"])
            if m > 0:
                rainD, rainR = cls(rw2[D], "donor"), cls(rw2[R], "receiver")
                rainP = rainD or rainR or cls(rw2_new, "product")
                rD3 = LD(rw2[D]) * np.sqrt(LD(rw2[D]))
                rR3 = LD(rw2[R]) * np.sqrt(LD(rw2[R]))
                loose = bool(grown[D] or grown[R])

                def add_m3(w, term):
                    sums.m3[w, c] += term
                    sums.abs_m3[w, c] += abs(term)
                    if loose:
                        sums.loose_m3[w, c] += abs(term)

                def add(w, v):
                    sums.num[w][c] += int(v)
                if not rainD and not rainR and not rainP:
                    add(5, cnt * m); sums.rows["cc->c"] += 1
                elif not rainD and not rainR:
                    add_m3(0, m * (cnt * rD3 + rR3)); add(1, (cnt + 1) * m); add(2, m); sums.rows["cc->r"] += 1
                elif not rainD:
                    add_m3(3, cnt * m * rD3); add(4, cnt * m); sums.rows["cr"] += 1
                elif not rainR:
                    add_m3(3, m * rR3); add(4, m); add(6, (cnt - 1) * m); sums.rows["rc"] += 1
                else:
                    add(6, cnt * m); sums.rows["rr"] += 1
                sums.events[c] += 1
            n[D] = np.uint64(int(n[D]) - cnt * m)
            rw2[R], rd3[R], vt[R] = rw2_new, rd3_new, real_t(-1)
            grown[R] = True
    return drawn


def m3_bar(sums, w, c, real_t, collide_bar_eps):
    """the bar of an M3 sum of cell c against the walk's: K - 1 additions in any order and the terms' own rounding, (K + 8) eps_double
    sum |term|; a term with a member that grew earlier in the chain carries the rounding of the radius the device stored for it,
    1.5 (the power from rw2 to r^3) times collide()'s bar in eps of the real type"""
    eps_d = LD(np.finfo(np.float64).eps)
    return (int(sums.events[c]) + 8) * eps_d * sums.abs_m3[w, c] + LD(1.5 * collide_bar_eps) * LD(np.finfo(real_t).eps) * sums.loose_m3[w, c]
