"""src_type = matching (k_src_match) super-droplet by super-droplet.

tests/test_hip_sources.py holds a matching firing to counts per cell and to two moment ratios.  Here every (source cell, size bin) of a
firing is held to a plain restatement in numpy float64, written in this file (match_reference; the CPU oracle has no source): which old
super-droplets the bin holds, whether its candidate stays, who may gain and how much.  Everything is keyed by the persistent debug tag
(opts_init.dbg_flags = TAG), and read through the "raw_*" state so that reading compacts nothing.

What a candidate's multiplicity was cannot be read once it has been handed on.  On the first firing of an object it comes from a TWIN:
the same options and seed with src_type = simple, which keeps every candidate.  The twin is a yardstick only because the candidates that
survive the matching run are bit-identical to the twin's newcomers of the same tag (asserted first).  On later firings the gain is held
to the range that int(multiplier * n(ln rd) * rhod / rho_stp + .5) takes over the bin (gain_bounds).

An old super-droplet whose bin coordinate lies within eps of an integer is ambiguous between the device's real_t and the restatement's
double (coord_eps): for it and the two bins it lies between only the weaker statement is asserted, and at most 1 % of a case's (cell,
bin) pairs may be weakened that way (AMBIGUOUS_CAP; the one test without the gpu mark holds the cases' inputs to it on the CPU)."""
import math

import numpy as np
import pytest

import _harness as h
from libcloudphxx_amd import lgrngn
from test_hip_sources import dist_analysis, src_cells, only_src, spectrum, steps, KEY, INIT, SRC, RHO_STP

REALS = [np.float64, np.float32]
REAL_IDS = ["double", "float"]
AMBIGUOUS_CAP = 0.01

# case: (grid, initial sd_conc, source sd_conc = bins, supstp, dt, cell volume, source cells)
CASES = {
    "sparse_3d": dict(init_sd=16, bins=64, supstp=3, dt=.5, vol=2. * 1.5 * 1., n_src=4, n_cell=60),
    "crowded": dict(init_sd=600, bins=8, supstp=50, dt=1., vol=1., n_src=2, n_cell=4),
    "bins_above_a_workgroup": dict(init_sd=64, bins=300, supstp=50, dt=1., vol=1., n_src=2, n_cell=4),
    "the_cap": dict(init_sd=16, bins=4096, supstp=1, dt=1., vol=1., n_src=2, n_cell=4),
    "moving": dict(init_sd=32, bins=16, supstp=1, dt=1., vol=1., n_src=6, n_cell=30),
}
# The seeds are inputs, chosen by what the RESTATEMENT says of the state before the match, never by what the kernel under test answers:
# 44 is the suite's usual seed.  The moving case has 96 pairs only, so one old super-droplet near a bin edge is 2 % of them: with seeds
# 44 and 4 a float object has one (the cap then fails the test before the kernel is looked at), with seed 1 the restatement leaves 23
# candidates (under the quarter that makes the twin a yardstick), with 2 it has none near an edge, leaves 27 and sees winners that move.
SEEDS = {"sparse_3d": 44, "crowded": 44, "bins_above_a_workgroup": 44, "the_cap": 44, "moving": 2}


# ------------------------------------------------------------------ the plain reference
def coord_eps(real_t, lo, hi, n_bins):
    """how close to an integer a bin coordinate may lie before the device's real_t and the restatement's double may disagree on its floor"""
    if real_t is np.float64:
        return 1e-9
    # float: the device forms ln rd = log(rd3) / 3 with |log(rd3)| in [32, 64) (ulp 2 ulp_float(20)) and |ln rd| in [16, 32): the
    # logarithm's rounding (one ulp of its result, i.e. 2/3 ulp_float(20) in ln rd), the division's (1/2), the subtraction of log_rd_min
    # (itself rounded to float: 1/2 + 1/2) and slack for the library logarithm being good to 1-2 ulp only: about 4 ulp_float(20) in ln rd,
    # i.e. n_bins * 4 * ulp_float(20) / (hi - lo) in the coordinate; the division by (hi - lo) and the product with n_bins add relative
    # 2^-23 of a coordinate < n_bins, which is less than 1/50 of that.  Eight times that.
    return 8 * n_bins * 4 * float(np.spacing(np.float32(20.))) / (hi - lo)


def classify(rd3, lo, hi, n_bins, eps):
    """(bin, near) per super-droplet in double: bin = floor of the coordinate, -1 outside [lo, hi); near = the integer k in 0 .. n_bins
    that the coordinate lies within eps of (the droplet is then between bins k - 1 and k, or across an end of the range), else -1"""
    x = (np.log(np.asarray(rd3, dtype=np.float64)) / 3. - lo) / (hi - lo) * n_bins
    b = np.floor(x).astype(np.int64)
    b[(x < 0) | (x >= n_bins)] = -1
    k = np.rint(x).astype(np.int64)
    near = np.where((np.abs(x - k) <= eps) & (k >= 0) & (k <= n_bins), k, -1)
    return b, near


def ambiguous_bins(near, n_bins):
    amb = np.zeros(n_bins, dtype=bool)
    for k in near[near >= 0]:
        amb[max(k - 1, 0):min(k, n_bins - 1) + 1] = True
    return amb


def match_reference(before, after, twin_new, cells, lo, hi, n_bins, tag_base, eps=1e-9):
    """before / after: dicts of tag, n, rd3, ijk (snapshot); twin_new: {tag: (rd3, n, ijk)} of the simple twin's newcomers, or None.
    Returns (bins, gains): bins[(ci, b)] = dict(old = the old tags surely in bin b of source cell number ci -- by the AFTER-step ijk,
    matching runs behind the move --, maybe = old tags that are within eps of one of its edges, ambiguous, survives = whether the
    candidate must still be there (None where ambiguous), n_cand = the twin's multiplicity of the candidate); gains = {old tag: n_after -
    n_before} where that is not 0."""
    pos = {int(t): i for i, t in enumerate(after["tag"])}
    missing = [int(t) for t in before["tag"] if int(t) not in pos]
    assert not missing, ("old super-droplets gone", missing[:8])
    idx = np.array([pos[int(t)] for t in before["tag"]], dtype=np.int64)
    ijk = after["ijk"][idx]
    diff = after["n"][idx] - before["n"]
    b, near = classify(before["rd3"], lo, hi, n_bins, eps)
    bins = {}
    for ci, c in enumerate(cells):
        here = ijk == c
        amb = ambiguous_bins(near[here], n_bins)
        old = [[] for _ in range(n_bins)]
        maybe = [[] for _ in range(n_bins)]
        for t, bb, k in zip(before["tag"][here], b[here], near[here]):
            if k >= 0:
                for m in (k - 1, k):
                    if 0 <= m < n_bins:
                        maybe[m].append(int(t))
            elif bb >= 0:
                old[bb].append(int(t))
        for bb in range(n_bins):
            cand = tag_base + ci * n_bins + bb
            bins[(ci, bb)] = dict(old=old[bb], maybe=maybe[bb], ambiguous=bool(amb[bb]), survives=None if amb[bb] else not old[bb],
                                  n_cand=None if twin_new is None else int(twin_new[cand][1]))
    gains = {int(t): int(d) for t, d in zip(before["tag"], diff) if d != 0}
    return bins, gains


def gain_bounds(par, builtin, real_t, lo, hi, mult, n_bins, rhod):
    """per bin, the least and the largest int(mult * n(ln rd) * rhod / rho_stp + .5) over the bin: a lognormal has one mode, so the
    extremes are at the bin's ends and at the mode if it is inside.  Exact for a callable spectrum in double; the built-in one is
    evaluated by the device's own exp / log: +- 1, as tests/test_hip_sources.py allows it.  A float object rounds the multiplier, the
    function's value, two products and a quotient, and rho_stp itself: < 8 * 2^-24 relative, held to 16 * 2^-24 of the bound, rounded up."""
    fn, mode = h.lognormal_fn(*par), math.log(par[0])
    edges = lo + (hi - lo) * np.arange(n_bins + 1) / n_bins
    out = []
    for b in range(n_bins):
        pts = [edges[b], edges[b + 1]] + ([mode] if edges[b] < mode < edges[b + 1] else [])
        v = [int(mult * fn(x) * rhod / RHO_STP + .5) for x in pts]
        w = (1 if builtin else 0) + (0 if real_t is np.float64 else int(math.ceil(max(v) * 16 * 2. ** -24)))
        out.append((max(min(v) - w, 0), max(v) + w))
    return out


def snapshot(p):
    """tag, n, rd3, ijk of the living, from the storage as it is: the "raw_*" state compacts and sorts nothing on the way"""
    n = p.state_u64("raw_n").astype(np.int64)
    live = n > 0
    s = dict(tag=p.state_real("raw_tag")[live].astype(np.int64), n=n[live], rd3=p.state_real("raw_rd3")[live],
             ijk=p.state_u64("raw_ijk")[live].astype(np.int64))
    assert live.sum() == p.n_part and np.unique(s["tag"]).size == s["tag"].size
    return s


def newcomers(snap, tag_base):
    return {int(t): (r, int(n), int(c)) for t, r, n, c in zip(snap["tag"], snap["rd3"], snap["n"], snap["ijk"]) if t >= tag_base}


def check_firing(before, after, twin_new, cells, lo, hi, n_bins, tag_base, eps, bounds=None, what=""):
    """the assertions of one matching firing; returns the figures the callers print or build on"""
    bins, gains = match_reference(before, after, twin_new, cells, lo, hi, n_bins, tag_base, eps)    # (every old tag is present)
    old_tags = set(int(t) for t in before["tag"])
    pos = {int(t): i for i, t in enumerate(after["tag"])}
    idx = np.array([pos[int(t)] for t in before["tag"]], dtype=np.int64)
    assert np.array_equal(after["rd3"][idx], before["rd3"])                  # bit for bit
    assert all(g > 0 for g in gains.values()), [g for g in gains.values() if g <= 0][:8]
    new_after = newcomers(after, tag_base)
    assert set(pos) == old_tags | set(new_after)
    assert all(tag_base <= t < tag_base + len(cells) * n_bins for t in new_after), sorted(new_after)[-4:]
    n_amb = sum(r["ambiguous"] for r in bins.values())
    assert n_amb <= AMBIGUOUS_CAP * len(bins), (n_amb, len(bins))

    # the twin is a yardstick only if the survivors ARE the twin's newcomers
    if twin_new is not None:
        assert len(twin_new) == len(bins) and all(v[1] > 0 for v in twin_new.values())
        assert 4 * len(new_after) >= len(bins), (len(new_after), len(bins))
        for t, v in new_after.items():
            assert v == twin_new[t], (t, v, twin_new[t])

    winners, accounted = {}, set()
    for (ci, b), r in bins.items():
        cand = tag_base + ci * n_bins + b
        if r["ambiguous"]:
            if cand not in new_after:       # handed on: to an old super-droplet of this bin or of one of the ambiguous bins next to it
                pool = set()
                for m in (b - 1, b, b + 1):
                    if (ci, m) in bins and bins[(ci, m)]["ambiguous"]:
                        pool |= set(bins[(ci, m)]["old"]) | set(bins[(ci, m)]["maybe"])
                got = [t for t in pool if t in gains]
                assert got, (what, ci, b)
                accounted |= set(got)
            continue
        if r["survives"]:
            assert cand in new_after, (what, "the candidate of an empty bin is gone", ci, b)
            rd3, n, c = new_after[cand]
            assert c == cells[ci], (ci, b, c)
            x = (math.log(rd3) / 3. - lo) / (hi - lo) * n_bins
            assert b - eps <= x < b + 1 + eps, (ci, b, x)
            if twin_new is not None:
                assert n == r["n_cand"]
            elif bounds is not None:
                assert bounds[ci][b][0] <= n <= bounds[ci][b][1], (ci, b, n, bounds[ci][b])
            continue
        assert cand not in new_after, (what, "the candidate of an occupied bin stayed", ci, b)
        got = [t for t in r["old"] if t in gains]
        assert len(got) == 1, (what, "winners of one bin", ci, b, got, len(r["old"]))
        g = gains[got[0]]
        if twin_new is not None:
            assert g == r["n_cand"], (what, ci, b, g, r["n_cand"])
        else:
            assert bounds[ci][b][0] <= g <= bounds[ci][b][1], (what, ci, b, g, bounds[ci][b])
        winners[(ci, b)] = got[0]
        accounted.add(got[0])
    # nothing else gained: no droplet outside the source box, outside [lo, hi), or a bin's second one
    assert set(gains) == accounted, (what, sorted(set(gains) - accounted)[:8])
    gone = len(bins) - len(new_after)
    assert len(gains) == gone, (what, len(gains), gone)
    if twin_new is not None:
        assert int(after["n"].sum()) == int(before["n"].sum()) + sum(v[1] for v in twin_new.values())
    return dict(pairs=len(bins), ambiguous=n_amb, survivors=len(new_after), winners=winners, bins=bins, gains=gains)


# ------------------------------------------------------------------ the cases
def make_case(case, real_t, builtin, src_type):
    k = CASES[case]
    oi = lgrngn.opts_init_t()
    if case == "sparse_3d":                                         # the box of test_structure_of_one_simple_firing_3d
        oi.nx, oi.ny, oi.nz = 4, 3, 5
        oi.dx, oi.dy, oi.dz = 2., 1.5, 1.
        oi.x1, oi.y1, oi.z1 = 8., 4.5, 5.
        oi.src_x0, oi.src_x1, oi.src_y0, oi.src_y1, oi.src_z0, oi.src_z1 = 1.7, 6.3, .8, 2.9, .6, 3.4
        shp = (4, 3, 5)
    elif case == "moving":
        oi.nx, oi.nz = 6, 5
        oi.x1, oi.z1 = 6., 5.
        oi.src_x0, oi.src_x1, oi.src_z0, oi.src_z1 = 1., 4., 0., 2.
        shp = (6, 5)
    else:
        oi.nx = oi.nz = 2
        oi.x1 = oi.z1 = 2.
        oi.src_x0, oi.src_x1, oi.src_z0, oi.src_z1 = 0., 2., 0., 1.     # the lower row
        shp = (2, 2)
    oi.dt = k["dt"]
    oi.coal_switch = oi.sedi_switch = False
    oi.dbg_flags = int(lgrngn.dbg.TAG)
    oi.rng_seed = SEEDS[case]
    oi.src_type = src_type
    oi.dry_distros = {KEY: spectrum(INIT, builtin)}
    oi.sd_conc = k["init_sd"]
    oi.n_sd_max = k["init_sd"] * k["n_cell"] + k["bins"] * k["n_src"]
    cells = src_cells(oi)
    assert len(cells) == k["n_src"] and oi.dx * oi.dy * oi.dz == k["vol"]
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, builtin), k["bins"], k["supstp"])}
    n_cell = int(np.prod(shp))
    rhod = (1. + .01 * np.arange(float(n_cell)).reshape(shp)) if case == "sparse_3d" else np.full(shp, 1.)
    f = [np.full(shp, 300., real_t), np.full(shp, .01, real_t), rhod.astype(real_t)]
    C = {}
    if case == "moving":
        opts.adve = True
        C = dict(Cx=np.full((7, 5), .4, real_t), Cz=np.zeros((6, 6), real_t))
        f += [C["Cx"], None, C["Cz"]]
    p = h.hip_particles(oi, real_t)
    p.init(*f[:3], **C)
    return p, opts, tuple(f), oi, cells


@pytest.mark.gpu
@pytest.mark.parametrize("builtin", [False, True], ids=["callable", "lognormal"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("case", list(CASES))
def test_one_matching_firing_per_droplet(case, real_t, builtin):
    k = CASES[case]
    p, opts, f, oi, cells = make_case(case, real_t, builtin, lgrngn.src_t.matching)
    twin, t_opts, t_f, _, _ = make_case(case, real_t, builtin, lgrngn.src_t.simple)
    tag_base = p.n_part
    assert tag_base == k["init_sd"] * k["n_cell"]
    before = snapshot(p)
    t_before = snapshot(twin)
    assert all(np.array_equal(before[q], t_before[q]) for q in before)
    steps(p, opts, f, 1)
    steps(twin, t_opts, t_f, 1)
    after, t_after = snapshot(p), snapshot(twin)
    twin_new = newcomers(t_after, tag_base)
    assert twin.n_part == tag_base + k["bins"] * len(cells)
    lo, hi, _ = dist_analysis(h.lognormal_fn(*SRC), k["bins"], k["supstp"] * oi.dt, oi.dx * oi.dy * oi.dz, real_t)
    eps = coord_eps(real_t, lo, hi, k["bins"])
    res = check_firing(before, after, twin_new, cells, lo, hi, k["bins"], tag_base, eps, what=case)
    cell_before, cell_after = dict(zip(before["tag"].tolist(), before["ijk"].tolist())), dict(zip(after["tag"].tolist(), after["ijk"].tolist()))
    moved = [t for t in res["winners"].values() if cell_before[t] != cell_after[t]]
    print("%s %s %s: pairs %d ambiguous %d (%.3f %%) survivors %d (%.1f %%) winners %d of which moved %d; most old in a cell %d; eps %.3g"
          % (case, real_t.__name__, "lognormal" if builtin else "callable", res["pairs"], res["ambiguous"],
             100. * res["ambiguous"] / res["pairs"], res["survivors"], 100. * res["survivors"] / res["pairs"], len(res["winners"]),
             len(moved), max(np.bincount(after["ijk"][after["tag"] < tag_base])), eps))
    if case == "moving":
        assert moved                                                # or the case proves nothing
    if case == "crowded":
        assert min((after["ijk"][after["tag"] < tag_base] == c).sum() for c in cells) > 256        # beyond one trip of the workgroup
    # the compacted, public view shows the same super-droplets
    pub = dict(zip(p.state_real("tag").astype(np.int64).tolist(), p.state_u64("n").astype(np.int64).tolist()))
    assert pub == dict(zip(after["tag"].tolist(), after["n"].tolist()))


# ------------------------------------------------------------------ the ambiguity cap on the CPU
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("case", list(CASES))
def test_ambiguity_cap_of_the_cases_inputs(case, real_t):
    """The restatement's own binning on synthetic stratified samples of the initial spectrum, as init() draws them (one per stratum of
    the analysed range, per cell): the share of (cell, bin) pairs that an old super-droplet near a bin edge would weaken stays in the cap."""
    k = CASES[case]
    i_lo, i_hi, _ = dist_analysis(h.lognormal_fn(*INIT), k["init_sd"], 1., k["vol"], real_t)
    lo, hi, _ = dist_analysis(h.lognormal_fn(*SRC), k["bins"], k["supstp"] * k["dt"], k["vol"], real_t)
    eps = coord_eps(real_t, lo, hi, k["bins"])
    rng = np.random.default_rng(SEEDS[case])
    n_amb = n_in = 0
    for _ in range(k["n_src"]):
        lnrd = i_lo + (np.arange(k["init_sd"]) + rng.random(k["init_sd"])) * (i_hi - i_lo) / k["init_sd"]
        rd3 = np.exp(3 * lnrd).astype(real_t)
        b, near = classify(rd3, lo, hi, k["bins"], eps)
        n_in += int((b >= 0).sum())
        n_amb += int(ambiguous_bins(near, k["bins"]).sum())
    pairs = k["n_src"] * k["bins"]
    print(case, real_t.__name__, "in range", n_in, "ambiguous pairs", n_amb, "of", pairs, "eps", eps)
    assert n_in > 0
    assert n_amb <= AMBIGUOUS_CAP * pairs, (n_amb, pairs)


# ------------------------------------------------------------------ a firing over holes, and later firings
@pytest.mark.gpu
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_second_firing_over_uncompacted_dead(real_t):
    n_bins, init_sd = 2, 64
    oi = lgrngn.opts_init_t()
    oi.nx = oi.nz = 2
    oi.x1 = oi.z1 = 2.
    oi.dt = 1.
    oi.coal_switch = oi.sedi_switch = False
    oi.dbg_flags = int(lgrngn.dbg.TAG)
    oi.rng_seed = 44
    oi.src_type = lgrngn.src_t.matching
    oi.src_x0, oi.src_x1, oi.src_z0, oi.src_z1 = 0., 2., 0., 1.
    oi.dry_distros = {KEY: spectrum(INIT, False)}
    oi.sd_conc = init_sd
    oi.n_sd_max = 4 * init_sd + 32
    cells = src_cells(oi)
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, False), n_bins, 1)}
    rhod = np.array([[1.1, 1.], [.9, .8]])
    f = (np.full((2, 2), 300., real_t), np.full((2, 2), .01, real_t), rhod.astype(real_t))
    p = h.hip_particles(oi, real_t)
    p.init(*f)
    lo, hi, mult = dist_analysis(h.lognormal_fn(*SRC), n_bins, 1., 1., real_t)
    eps = coord_eps(real_t, lo, hi, n_bins)
    bounds = [gain_bounds(SRC, False, real_t, lo, hi, mult, n_bins, float(real_t(rhod.flat[c]))) for c in cells]
    first = snapshot(p)
    n_init = p.n_part
    old = lambda s: int(s["n"][s["tag"] < n_init].sum())
    steps(p, opts, f, 1)                                            # the first firing matches every candidate ...
    assert p.n_part == n_init
    raw = p.state_u64("raw_n")
    assert raw.size == n_init + n_bins * len(cells) and (raw == 0).sum() == n_bins * len(cells)    # ... and their slots are still there
    tag_base = n_init + n_bins * len(cells)
    check_firing(first, snapshot(p), None, cells, lo, hi, n_bins, n_init, eps, bounds, "firing 1")
    for firing in (2, 3):
        before = snapshot(p)
        holes = p.state_u64("raw_n").size - p.n_part
        steps(p, opts, f, 1)
        res = check_firing(before, snapshot(p), None, cells, lo, hi, n_bins, tag_base, eps, bounds, "firing %d" % firing)
        print("firing", firing, real_t.__name__, "dead slots in storage before it", holes, "ambiguous", res["ambiguous"], "survivors", res["survivors"])
        if firing == 2:
            assert holes > 0
        assert res["survivors"] == 0
        tag_base += n_bins * len(cells)
    grown = old(snapshot(p)) - old(first)
    low, high = (3 * sum(b[i] for per_cell in bounds for b in per_cell) for i in (0, 1))
    print("sum n of the old grew by", grown, "bounds", low, high)
    assert low <= grown <= high


# ------------------------------------------------------------------ the pick
def test_the_winner_is_uniform_in_its_bin_setup():
    """the geometry that test_the_winner_is_uniform_in_its_bin builds on, from the distribution analysis alone (no GPU)"""
    uniform_geometry()


K_OLD, UNI_BINS, UNI_LNRD = 8, 16, -15.48


def uniform_geometry():
    i_lo, i_hi, _ = dist_analysis(h.lognormal_fn(*INIT), 4, 1., 1.)
    lo, hi, _ = dist_analysis(h.lognormal_fn(*SRC), UNI_BINS, 1., 1.)
    b = int(math.floor((UNI_LNRD - lo) / (hi - lo) * UNI_BINS))
    e0, e1 = lo + b * (hi - lo) / UNI_BINS, lo + (b + 1) * (hi - lo) / UNI_BINS
    assert lo <= e0 and e1 <= hi and 0 <= b < UNI_BINS              # inside the source's range,
    assert i_hi < e0                                                # the whole bin above what init() can draw from the initial spectrum,
    assert e0 + .05 < UNI_LNRD < e1 - .05                           # and well inside its bin
    return lo, hi, b


@pytest.mark.gpu
def test_the_winner_is_uniform_in_its_bin():
    try:
        from scipy.stats import chi2
        bar = float(chi2.isf(1e-6, K_OLD - 1))
    except ImportError:
        bar = 40.52                                                 # scipy.stats.chi2.isf(1e-6, 7) = 40.5218
    assert abs(bar - 40.52) < .01
    lo, hi, b_k = uniform_geometry()
    nx = 16
    oi = lgrngn.opts_init_t()
    oi.nx = oi.nz = nx
    oi.x1 = oi.z1 = float(nx)
    oi.dt = 1.
    oi.coal_switch = oi.sedi_switch = False
    oi.dbg_flags = int(lgrngn.dbg.TAG)
    oi.rng_seed = 44
    oi.src_type = lgrngn.src_t.matching
    oi.src_x0, oi.src_x1, oi.src_z0, oi.src_z1 = 0., float(nx), 0., float(nx)
    oi.dry_distros = {KEY: spectrum(INIT, False)}
    oi.sd_conc = 4
    oi.dry_sizes = {KEY: {math.exp(UNI_LNRD): [1e6, K_OLD]}}
    n_cell, firings = nx * nx, 4
    oi.n_sd_max = n_cell * (4 + K_OLD + (firings + 1) * UNI_BINS)
    cells = src_cells(oi)
    assert cells == list(range(n_cell))
    opts = only_src()
    opts.src_dry_distros = {KEY: (spectrum(SRC, False), UNI_BINS, 1)}
    f = (np.full((nx, nx), 300.), np.full((nx, nx), .01), np.full((nx, nx), 1.))
    p = h.hip_particles(oi)
    p.init(*f)
    assert p.n_part == n_cell * (4 + K_OLD)
    tag_base = p.n_part
    ranks = np.empty((firings, n_cell), dtype=np.int64)
    for firing in range(firings):
        before = snapshot(p)
        steps(p, opts, f, 1)
        after = snapshot(p)
        bins, gains = match_reference(before, after, None, cells, lo, hi, UNI_BINS, tag_base)
        for ci in range(n_cell):
            r = bins[(ci, b_k)]
            assert len(r["old"]) == K_OLD and not r["ambiguous"], (ci, r)     # the K of dry_sizes and nobody else
            assert all(t >= n_cell * 4 for t in r["old"]) and (firing == 0 or sorted(r["old"]) == group[ci])
            got = [t for t in r["old"] if t in gains]
            assert len(got) == 1, (firing, ci, got)
            ranks[firing, ci] = sorted(r["old"]).index(got[0])
        if firing == 0:
            group = [sorted(bins[(ci, b_k)]["old"]) for ci in range(n_cell)]
        tag_base += UNI_BINS * n_cell
    counts = np.bincount(ranks.ravel(), minlength=K_OLD)
    expect = ranks.size / K_OLD
    stat = float(((counts - expect) ** 2 / expect).sum())
    same = float((ranks[1:] == ranks[:-1]).mean())
    pairs = ranks[1:].size
    sd = math.sqrt(1. / K_OLD * (1 - 1. / K_OLD) / pairs)
    print("ranks of %d picks" % ranks.size, counts, "chi-square", stat, "bar", bar, "same winner in consecutive firings", same, "1/K", 1. / K_OLD, "sd", sd)
    assert stat < bar
    assert abs(same - 1. / K_OLD) <= 5 * sd
