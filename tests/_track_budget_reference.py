"""The budget of tracked super-droplets (include/lcx_track_budget.h) restated in numpy long double from raw states of an object, read
with the raw_ getters only (raw_n, raw_rw2, raw_rd3, raw_track: reading "T", "RH" or "rv" compacts the storage and must not happen
between the two reads of a pass).  No project code; droplets are matched by their mark (_track_reference.slot_of).

A pass is given by the raw state ahead of it and the raw state behind it.  Index k takes part if a slot carries mark k + 1 with n > 0
ahead of the pass; n1 = 0 where no such slot is left behind it.  Besides the seven accumulators the module keeps, per index and real
field, K (the number of terms added) and S (the sum of c(w1) + c(w0), or of d1 + d0): the bar of a sum of K terms is (K + 8) 2^-52 S
(each cube carries at most 1.5 ulp, each difference and each addition half an ulp: the error stays below (2 + K / 2) eps S; the stored
float of a float object converts to double exactly, so the bar is in double eps there too)."""
import numpy as np

import _track_reference as TR

LD = np.longdouble
FIELDS = ("cond_dr3", "coal_dr3", "coal_drd3", "chem_drd3", "coal_dn", "coal_gains", "coal_gives")      # enum LCX_TRB_*, in its order
REAL_FIELDS, INT_FIELDS = FIELDS[:4], FIELDS[4:]
EPS = LD(2) ** -52


def raw(prt):
    return {"n": prt.state_u64("raw_n"), "rw2": prt.state_real("raw_rw2"), "rd3": prt.state_real("raw_rd3"), "track": prt.state_real("raw_track")}


def cube(v):
    x = np.asarray(v, dtype=LD)
    return x * np.sqrt(x)


def values(st, n_tracked):
    """(n, rw2, rd3) per track index: the stored values of the slot that carries mark k + 1, n = 0 where there is none"""
    so = TR.slot_of(st, n_tracked)
    n, w, d = np.zeros(n_tracked, dtype=np.uint64), np.zeros(n_tracked), np.zeros(n_tracked)
    has = so >= 0
    n[has], w[has], d[has] = st["n"][so[has]], st["rw2"][so[has]], st["rd3"][so[has]]
    return n, w, d


def bar(K, S):
    return (np.asarray(K, dtype=LD) + 8) * EPS * S


class Budget:
    def __init__(self):
        self.n = 0
        self.acc = {f: np.zeros(0, dtype=LD) for f in FIELDS}
        self.S = {f: np.zeros(0, dtype=LD) for f in REAL_FIELDS}
        self.K = {f: np.zeros(0, dtype=np.int64) for f in REAL_FIELDS}
        self.passes = {"cond": 0, "chem": 0, "coal": 0}
        self.used_up = 0

    def grow(self, n_tracked):
        """indices selected since: zero from now on"""
        for tab in (self.acc, self.S, self.K):
            for f in tab:
                tab[f] = np.concatenate([tab[f], np.zeros(n_tracked - self.n, dtype=tab[f].dtype)])
        self.n = n_tracked

    def _add(self, f, part, new, old):
        self.acc[f][part] += new - old
        self.S[f][part] += new + old
        self.K[f][part] += 1

    def add(self, family, before, after, n_tracked):
        """one pass of `family` ("cond", "chem", "coal") between the raw states before and after"""
        self.grow(n_tracked)
        self.passes[family] += 1
        n0, w0, d0 = values(before, n_tracked)
        n1, w1, d1 = values(after, n_tracked)
        part = n0 > 0
        dw, dd = part & (n1 > 0) & (w1 != w0), part & (n1 > 0) & (d1 != d0)
        if family == "cond":
            self._add("cond_dr3", dw, cube(w1[dw]), cube(w0[dw]))
        elif family == "chem":
            self._add("chem_drd3", dd, d1[dd].astype(LD), d0[dd].astype(LD))
        else:
            self._add("coal_dr3", dw, cube(w1[dw]), cube(w0[dw]))
            self._add("coal_drd3", dd, d1[dd].astype(LD), d0[dd].astype(LD))
            gives = part & (n1 < n0)
            assert not (part & (n1 > n0)).any(), "no pass raises a multiplicity"
            self.acc["coal_dn"][gives] += (n0[gives] - n1[gives]).astype(LD)
            self.acc["coal_gives"][gives] += 1
            self.acc["coal_gains"][part & (n1 == n0) & (dw | dd)] += 1
            self.used_up += int((gives & (n1 == 0)).sum())
        return part

    def snapshot(self):
        return {"acc": {f: v.copy() for f, v in self.acc.items()}, "S": {f: v.copy() for f, v in self.S.items()},
                "K": {f: v.copy() for f, v in self.K.items()}}


def assert_matches(got, snap, tag):
    """got: {field: n_tracked doubles} (a row, or "now"); snap: Budget.snapshot().  The integer fields exactly, the sums to their bar.
    Returns the worst error in units of the bar."""
    worst = 0.
    for f in INT_FIELDS:
        want = snap["acc"][f]
        assert got[f].shape == want.shape and np.array_equal(got[f].astype(LD), want), (tag, f, np.flatnonzero(got[f].astype(LD) != want)[:8])
    for f in REAL_FIELDS:
        want, S, K = snap["acc"][f], snap["S"][f], snap["K"][f]
        err, lim = np.abs(got[f].astype(LD) - want), bar(K, S)
        none = K == 0
        assert (got[f][none] == 0).all(), (tag, f, "no term, yet not zero")
        bad = err > lim
        assert not bad.any(), (tag, f, np.flatnonzero(bad)[:8], err[bad][:4], lim[bad][:4])
        if (~none).any():
            worst = max(worst, float((err[~none] / lim[~none]).max()))
    return worst
