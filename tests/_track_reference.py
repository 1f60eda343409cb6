"""Tracked super-droplets (include/lcx_track.h) restated in plain numpy from the raw state of an object: which droplets a selection takes
and which indices they get, and what a sample must hold.  No project code.

The raw state is what lcx_get_state_u64 / lcx_get_state_real show under the "raw_" names (the storage as it is, dead slots included), every
real converted to double, plus the cell arrays "T", "RH" and "rv"."""
import numpy as np

FIELDS = ("n", "x", "y", "z", "rw2", "rd3", "kappa", "vt", "cell", "T", "RH", "rv")
RAW_REAL = {"x": "raw_x", "y": "raw_y", "z": "raw_z", "rw2": "raw_rw2", "rd3": "raw_rd3", "kappa": "raw_kappa", "vt": "raw_vt"}
_POWER = {"dry": 3, "wet": 2, "kappa": 1}
_ATTR = {"dry": "rd3", "wet": "rw2", "kappa": "kappa"}


def raw_state(prt):
    """everything the two rules read, from the object's getters.  The raw arrays come first: "T", "RH" and "rv" are no raw_ names, so reading
    them compacts the storage (dead slots leave, the slot list of a tracking object goes stale) AFTER the raw arrays were taken."""
    st = {"n": prt.state_u64("raw_n"), "cell": prt.state_u64("raw_ijk"), "track": prt.state_real("raw_track")}
    for nm, raw in RAW_REAL.items():
        v = prt.state_real(raw)
        st[nm] = v if v.size else np.zeros(st["n"].size)          # (a dimension the object lacks: no column, the record holds 0)
    for nm in ("T", "RH", "rv"):
        st["cell_" + nm] = prt.state_real(nm)
    st["has"] = {d: prt.state_real("raw_" + d).size > 0 for d in "xyz"}
    return st


def bound(attr, r, real_t):
    """a radius as lcx_diag_*_rng takes it: the square (wet) or cube (dry) in double, rounded to the object's real type (as in
    tests/_diag_reference.py for radii that the real type holds exactly)"""
    return np.float64(real_t(np.float64(r) ** _POWER[attr]))


def qualifies(st, clauses, box, real_t):
    """the qualifying predicate per storage slot"""
    q = (st["n"] > 0) & (st["track"] == 0)
    for c in clauses:
        if c[0] == "all":
            continue
        if c[0] == "water":
            q &= st["rw2"] > 0
            continue
        assert c[0] == "rng"
        lo, hi = bound(c[1], c[2], real_t), bound(c[1], c[3], real_t)
        v = st[_ATTR[c[1]]]
        q &= (v >= lo) & (v < hi)
    if box is not None:
        for d, nm in enumerate("xyz"):
            if st["has"][nm]:
                q &= (st[nm] >= box[2 * d]) & (st[nm] < box[2 * d + 1])
    return q


def select(st, clauses, box, max_count, max_tracked, n_tracked, real_t):
    """(slots taken in storage order, their track indices): Q qualifying droplets ranked in storage order, room = min(max_count,
    max_tracked - n_tracked), stride = ceil(Q / room), the ranks that are multiples of the stride"""
    slots = np.flatnonzero(qualifies(st, clauses, box, real_t))
    Q, room = int(slots.size), min(int(max_count), int(max_tracked) - int(n_tracked))
    if Q == 0 or room <= 0:
        return slots[:0], np.zeros(0, dtype=np.int64)
    stride = -(-Q // room)
    took = slots[::stride]
    assert took.size == -(-Q // stride) <= room
    return took, n_tracked + np.arange(took.size)


def select_slots(st, slots, max_tracked, n_tracked):
    """the slots that lcx_track_select_slots takes, in the order given"""
    took = []
    for s in slots:
        s = int(s)
        if n_tracked + len(took) >= max_tracked:
            break
        if s < 0 or s >= st["n"].size or st["n"][s] == 0 or st["track"][s] != 0 or s in took:
            continue
        took.append(s)
    return np.array(took, dtype=np.int64)


def slot_of(st, n_tracked):
    """the storage slot that carries mark k + 1, or -1; no mark twice"""
    out = np.full(n_tracked, -1, dtype=np.int64)
    marked = np.flatnonzero(st["track"] != 0)
    k = st["track"][marked].astype(np.int64) - 1
    assert np.array_equal(st["track"][marked], k + 1.) and (k >= 0).all() and (k < n_tracked).all(), "marks are whole numbers in 1 .. n_tracked"
    assert np.unique(k).size == k.size, "no index on two slots"
    out[k] = marked
    return out


def record(st, n_tracked):
    """{field: n_tracked doubles}: the values at the slot whose mark is k + 1; N = 0 and NaN elsewhere where that slot is missing or dead"""
    so = slot_of(st, n_tracked)
    alive = so >= 0
    alive[alive] = st["n"][so[alive]] > 0
    rec = {f: np.full(n_tracked, np.nan) for f in FIELDS}
    rec["n"] = np.zeros(n_tracked)
    s = so[alive]
    rec["n"][alive] = st["n"][s].astype(np.float64)
    for f in ("x", "y", "z", "rw2", "rd3", "kappa", "vt"):
        rec[f][alive] = st[f][s]
    c = st["cell"][s].astype(np.int64)
    rec["cell"][alive] = c.astype(np.float64)
    for f in ("T", "RH", "rv"):
        rec[f][alive] = st["cell_" + f][c]
    return rec, alive
