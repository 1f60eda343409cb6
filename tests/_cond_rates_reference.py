"""The rows of include/lcx_cond_rates.h from the raw state, without any project code: numpy long double and Python integers.

tally(n, ijk, rw2_0, rw2_1, lo, n_cell): n the multiplicities, ijk the cells, rw2_0 / rw2_1 the stored rw2 before and after (in the object's
real type), lo the bounds lo_t in that type.  Returns a Rows: value(row, cell) is a Python int for the number rows and a long double for the
M3 rows; count(row, cell) is K_c, the droplets that contribute to an M3 row, and weight(row, cell) is S = sum n (r0^3 + r1^3) over them."""
import numpy as np

LD = np.longdouble
NAMES = ("above_dm3", "up_n", "up_m3", "down_n", "down_m3")
ABOVE_DM3, UP_N, UP_M3, DOWN_N, DOWN_M3, PER_THR = range(6)
NUMBER = (UP_N, DOWN_N)


def bounds(r_thr, real_t):
    """lo_t: the square in double, rounded to the real type"""
    return [real_t(np.float64(r) ** 2) for r in r_thr]


def cube(rw2):
    x = np.asarray(rw2).astype(LD)
    return x * np.sqrt(x)


class Rows:
    def __init__(self, n_thr, n_cell):
        self.n_thr, self.n_cell, self.n_rows = n_thr, n_cell, PER_THR * n_thr + 1
        self.val = [[0 if self.is_number(w) else LD(0) for _ in range(n_cell)] for w in range(self.n_rows)]
        self.cnt = np.zeros((self.n_rows, n_cell), dtype=np.int64)
        self.wgt = np.zeros((self.n_rows, n_cell), dtype=LD)
        self.up = np.zeros((n_thr, n_cell), dtype=np.int64)            # droplets (not multiplicities) that crossed, per threshold and cell
        self.down = np.zeros((n_thr, n_cell), dtype=np.int64)

    def is_number(self, w):
        return w < PER_THR * self.n_thr and w % PER_THR in NUMBER

    def value(self, w, c):
        return self.val[w][c]

    def count(self, w, c):
        return int(self.cnt[w, c])

    def weight(self, w, c):
        return self.wgt[w, c]

    def add(self, w, c, v, s=None):
        self.val[w][c] += v
        if s is not None:
            self.cnt[w, c] += 1
            self.wgt[w, c] += s


def tally(n, ijk, rw2_0, rw2_1, lo, n_cell, rows=None):
    rows = rows if rows is not None else Rows(len(lo), n_cell)
    c0, c1 = cube(rw2_0), cube(rw2_1)
    total = PER_THR * len(lo)
    for i in range(len(n)):
        m, c = int(n[i]), int(ijk[i])
        if m == 0 or not 0 <= c < n_cell:
            continue
        s = m * (c0[i] + c1[i])
        rows.add(total, c, m * (c1[i] - c0[i]), s)
        for t, l in enumerate(lo):
            a0, a1 = bool(rw2_0[i] >= l), bool(rw2_1[i] >= l)
            if a0 and a1:
                rows.add(PER_THR * t + ABOVE_DM3, c, m * (c1[i] - c0[i]), s)
            elif a1:
                rows.add(PER_THR * t + UP_N, c, m)
                rows.add(PER_THR * t + UP_M3, c, m * c1[i], s)
                rows.up[t, c] += 1
            elif a0:
                rows.add(PER_THR * t + DOWN_N, c, m)
                rows.add(PER_THR * t + DOWN_M3, c, m * c0[i], s)
                rows.down[t, c] += 1
    return rows


def m3_bar(rows, w, c):
    """(K_c + 8) eps_double S: each term is a few roundings in double of exactly converted inputs, and K_c - 1 additions in any order"""
    return (rows.count(w, c) + 8) * LD(np.finfo(np.float64).eps) * rows.weight(w, c)
