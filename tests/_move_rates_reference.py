"""The rows of include/lcx_move_rates.h from the raw state, without any project code: numpy long double and Python integers.

tally(n0, ijk0, rw2, pos0, n1, ijk1, lo, box, pos1=None): per storage slot ahead of the move n0 the multiplicities, ijk0 the cells, rw2 the
stored rw2 (in the object's real type), pos0 = (x, y, z) the positions (None for a dimension the box lacks); behind it n1 (0: removed) and
ijk1 the cell that the step stored, both aligned with the slots of n0; lo the bounds lo_t in the real type; box a Box.  pos1: the stored
positions behind the move where the caller still has them (the storage was not compacted).  A removed droplet's exit is named from pos1 in
the order of the move -- side walls, then top, then bottom; without pos1 (closed side walls only) from pos0: a droplet that moves by less
than half the domain's height leaves through the bottom from the lower half and through the top from the upper half.

Returns a Rows: value(row, cell) is a Python int for the _N rows and a long double for the _M3 rows; count(row, cell) is K_c, the droplets
that contribute to an _M3 row, and weight(row, cell) is S = sum m r^3 over them."""
import numpy as np

LD = np.longdouble
NAMES = ("in_n", "in_m3", "out_n", "out_m3", "down_n", "down_m3", "up_n", "up_m3", "precip_n", "precip_m3")
IN_N, IN_M3, OUT_N, OUT_M3, DOWN_N, DOWN_M3, UP_N, UP_M3, PRECIP_N, PRECIP_M3, PER_THR = range(11)


class Box:
    """the cells (z fastest) and the walls; nz = 0: no vertical dimension"""
    def __init__(self, nx, ny, nz, x0=0., x1=None, y0=0., y1=None, z0=0., z1=None, open_side_walls=False, periodic_topbot=False):
        self.nx, self.ny, self.nz = nx, ny, nz
        self.n_cell = max(nx, 1) * max(ny, 1) * max(nz, 1)
        self.x0, self.x1, self.y0, self.y1, self.z0, self.z1 = x0, x1, y0, y1, z0, z1
        self.open_side_walls, self.periodic_topbot = open_side_walls, periodic_topbot

    def k_of(self, c):
        return c % self.nz if self.nz else None


def bounds(r_thr, real_t):
    """lo_t: the square in double, rounded to the real type"""
    return [real_t(np.float64(r) ** 2) for r in r_thr]


def cube(rw2):
    x = np.asarray(rw2).astype(LD)
    return x * np.sqrt(x)


class Rows:
    def __init__(self, n_thr, n_cell):
        self.n_thr, self.n_cell, self.n_rows = n_thr, n_cell, PER_THR * n_thr
        self.val = [[0 if self.is_number(w) else LD(0) for _ in range(n_cell)] for w in range(self.n_rows)]
        self.cnt = np.zeros((self.n_rows, n_cell), dtype=np.int64)
        self.wgt = np.zeros((self.n_rows, n_cell), dtype=LD)
        self.removed = [0] * n_thr                                     # multiplicities removed above each threshold
        self.events = dict(stay=0, moved=0, bottom=0, top=0, side=0)   # droplets (not multiplicities), whatever their radius

    @staticmethod
    def is_number(w):
        return w % 2 == 0

    def value(self, w, c):
        return self.val[w][c]

    def count(self, w, c):
        return int(self.cnt[w, c])

    def weight(self, w, c):
        return self.wgt[w, c]

    def both(self, t, which_n, c, m, mr3):
        self.val[PER_THR * t + which_n][c] += m
        w = PER_THR * t + which_n + 1
        self.val[w][c] += mr3
        self.cnt[w, c] += 1
        self.wgt[w, c] += mr3

    def block(self):
        """the rows as a (10 K, n_cell) array of long doubles"""
        return np.array([[LD(v) for v in row] for row in self.val], dtype=LD)


def exit_of(box, i, pos0, pos1):
    """'side', 'top', 'bottom' or None (removed without leaving the domain: not by the move's walls)"""
    if pos1 is not None:
        x, y, z = (None if p is None else p[i] for p in pos1)
        if box.open_side_walls:
            if x is not None and (x >= box.x1 or x < box.x0):
                return "side"
            if box.ny and box.nz and y is not None and (y >= box.y1 or y < box.y0):
                return "side"
        if box.nz and (box.nx or box.ny) and not box.periodic_topbot:
            if z >= box.z1:
                return "top"
            if z < box.z0:
                return "bottom"
        return None
    assert not box.open_side_walls and box.nz and not box.periodic_topbot
    return "bottom" if pos0[2][i] < (box.z0 + box.z1) / 2 else "top"


def tally(n0, ijk0, rw2, pos0, n1, ijk1, lo, box, pos1=None, rows=None):
    rows = rows if rows is not None else Rows(len(lo), box.n_cell)
    r3 = cube(rw2)
    vertical = bool(box.nz) and bool(box.nx or box.ny)
    for i in range(len(n0)):
        m, c0 = int(n0[i]), int(ijk0[i])
        if m == 0 or not 0 <= c0 < box.n_cell:
            continue
        removed = int(n1[i]) == 0
        c1 = None if removed else int(ijk1[i])
        if not removed and c1 == c0:
            rows.events["stay"] += 1
            continue
        down = up = precip = False
        if removed:
            ex = exit_of(box, i, pos0, pos1)
            rows.events[{"bottom": "bottom", "top": "top", "side": "side", None: "side"}[ex]] += 1
            down = precip = ex == "bottom"
            up = ex == "top"
        else:
            rows.events["moved"] += 1
            if vertical:
                down, up = box.k_of(c1) < box.k_of(c0), box.k_of(c1) > box.k_of(c0)
        mr3 = m * r3[i]
        for t, l in enumerate(lo):
            if not rw2[i] >= l:
                continue
            rows.both(t, OUT_N, c0, m, mr3)
            if removed:
                rows.removed[t] += m
            else:
                rows.both(t, IN_N, c1, m, mr3)
            if down:
                rows.both(t, DOWN_N, c0, m, mr3)
            if up:
                rows.both(t, UP_N, c0, m, mr3)
            if precip:
                rows.both(t, PRECIP_N, c0 - box.k_of(c0), m, mr3)
    return rows


def m3_bar(rows, w, c):
    """(K_c + 8) eps_double S: each term is a few roundings in double of exactly converted inputs, and K_c - 1 additions in any order"""
    return (rows.count(w, c) + 8) * LD(np.finfo(np.float64).eps) * rows.weight(w, c)
