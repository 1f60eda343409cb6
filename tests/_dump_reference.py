"""The particle dump (include/lcx_dump.h) restated in plain numpy from the raw state of an object: which storage slots qualify, which of them
the stride rule writes, and what every field must hold.  No project code.

The raw state is what lcx_get_state_u64 / lcx_get_state_real show under the "raw_" names (the storage as it is, dead slots included), every
real converted to double.  The cell arrays "T", "RH" and "rv" are no raw_ names: reading them compacts the storage, so `cells` is called
AFTER the dump that is compared (it leaves the cell arrays as they are)."""
import numpy as np

from _track_reference import RAW_REAL, bound, _ATTR

FIELDS = ("n", "x", "y", "z", "rw2", "rd3", "kappa", "vt", "cell", "T", "RH", "rv", "slot", "track", "incloud_time",
          "chem_hno3", "chem_nh3", "chem_co2", "chem_so2", "chem_h2o2", "chem_o3", "chem_s_vi", "chem_h")
BASE = FIELDS[:14]                                    # what every object has


def raw(prt):
    """the raw arrays alone: nothing here compacts, sorts or waits for more than the stream"""
    st = {"n": prt.state_u64("raw_n"), "cell": prt.state_u64("raw_ijk")}
    N = st["n"].size
    for nm, name in RAW_REAL.items():
        v = prt.state_real(name)
        st[nm] = v if v.size else np.zeros(N)          # (a dimension the object lacks: no column, the record holds 0)
    st["has"] = {d: prt.state_real("raw_" + d).size > 0 for d in "xyz"}
    tr = prt.state_real("raw_track")
    st["track"] = tr if tr.size else np.zeros(N)       # (not tracking: the field is 0)
    return st


def cells(prt, st):
    """adds the cell arrays (a compacting read: behind the dump)"""
    for nm in ("T", "RH", "rv"):
        st["cell_" + nm] = prt.state_real(nm)
    return st


def qualifies(st, clauses, box, real_t):
    """the predicate per storage slot: alive, every clause, the box; the mark plays no part"""
    q = st["n"] > 0
    for c in clauses:
        if c[0] == "all":
            continue
        if c[0] == "water":
            q = q & (st["rw2"] > 0)
            continue
        assert c[0] == "rng"
        lo, hi = bound(c[1], c[2], real_t), bound(c[1], c[3], real_t)
        v = st[_ATTR[c[1]]]
        q = q & (v >= lo) & (v < hi)
    if box is not None:
        for d, nm in enumerate("xyz"):
            if st["has"][nm]:
                q = q & (st[nm] >= box[2 * d]) & (st[nm] < box[2 * d + 1])
    return q


def written(st, clauses, box, max_count, real_t):
    """(Q, stride, the slots written in their order): stride = ceil(Q / max_count), the ranks that are multiples of it.  max_count None: all"""
    slots = np.flatnonzero(qualifies(st, clauses, box, real_t))
    Q = int(slots.size)
    if Q == 0:
        return 0, 0, slots
    stride = 1 if max_count is None else -(-Q // int(max_count))
    took = slots[::stride]
    assert max_count is None or took.size == -(-Q // stride) <= max_count
    return Q, stride, took


def record(st, slots, fields):
    """{field: doubles}: the stored values at the given slots"""
    out = {}
    c = st["cell"][slots].astype(np.int64)
    for f in fields:
        if f == "n":
            out[f] = st["n"][slots].astype(np.float64)
        elif f == "cell":
            out[f] = c.astype(np.float64)
        elif f == "slot":
            out[f] = slots.astype(np.float64)
        elif f in ("T", "RH", "rv"):
            arr = st["cell_" + f]
            v = np.full(slots.size, np.nan)
            ok = c < arr.size
            v[ok] = arr[c[ok]]
            out[f] = v
        else:
            out[f] = np.asarray(st[f], dtype=np.float64)[slots]
    return out
