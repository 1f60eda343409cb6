"""Move rates per cell (include/lcx_move_rates.h) on the device, in double and float.

1. Droplet by droplet: the boxes of tests/test_move_rates_design.py (which shows on the CPU oracle that every row of the table occurs in
   them at every threshold), the raw storage read before and after one step_async, the rows of tests/_move_rates_reference.py against
   move_rates().  _N rows exact, _M3 rows to (K_c + 8) eps_double S.  euler, implicit and pred_corr, 2-D and 3-D.
2. The same droplets in interleaved storage (runs of one lane) and with dead slots in the middle.
3. The ground: PRECIP against diag_puddle over three steps, and sum IN = sum OUT - removed.
4. The plain sequence: opts.rcyc and a firing matching source; newcomers are not arrivals.
5. open_side_walls, periodic_topbot_walls, subsidence and turb_adve.
6. Three steps read once and with a reset in between.
7. The full closure of a cell's rain-drop number with the condensation and collision rates, everything on.
8. Nothing else moves; 9. launch counts; 10. diag_move_rate and device output; 11. the surface.
"""
import ctypes as C

import numpy as np
import pytest

import _harness as h
import _move_rates_reference as MV
import test_move_rates_design as D
import test_hip_coal_rates as TCR
from libcloudphxx_amd import lgrngn

pytestmark = pytest.mark.gpu

LD = np.longdouble
REALS = [np.float64, np.float32]
REAL_IDS = ["f64", "f32"]
THR = D.THR
SCHEMES = {"euler": lgrngn.as_t.euler, "implicit": lgrngn.as_t.implicit, "pred_corr": lgrngn.as_t.pred_corr}


def start(case, real_t, thr=THR, when="after"):
    prt = h.hip_particles(case["oi"], real_t)
    if thr is not None and when == "before":
        prt.move_rates_enable(thr)
    D.start(prt, case, (lambda p: p.move_rates_enable(thr)) if thr is not None and when == "after" else None)
    return prt


def as_block(prt):
    got = prt.move_rates()
    k = len(prt.move_rates_info()[1])
    out = np.zeros((10 * k, prt.n_cell))
    for w, nm in enumerate(lgrngn.MOVE_RATES):
        assert got[nm].shape == (k, out.shape[1])
        out[w::10] = got[nm]
    return out


def assert_rows(got, rows, tag):
    """got: (10 K, n_cell) doubles of the device"""
    assert got.shape == (rows.n_rows, rows.n_cell), (got.shape, rows.n_rows, rows.n_cell)
    worst = 0.
    for w in range(rows.n_rows):
        for c in range(rows.n_cell):
            want = rows.value(w, c)
            if rows.is_number(w):
                assert want < 2 ** 53 and got[w, c] == float(want), (tag, "row", w, MV.NAMES[w % 10], "cell", c, got[w, c], want)
            else:
                bar = MV.m3_bar(rows, w, c)
                err = abs(LD(got[w, c]) - want)
                if bar > 0:
                    worst = max(worst, float(err / bar))
                assert err <= bar, (tag, "row", w, MV.NAMES[w % 10], "cell", c, got[w, c], float(want), "bar", float(bar))
    print("%-44s worst |M3 - reference| / bar: %.3f" % (tag, worst))


def occurred(rows):
    """the case is not an empty one: every row at every threshold"""
    blk = rows.block()
    return all(blk[w].sum() > 0 for w in range(rows.n_rows))


def tallied_step(prt, case, real_t, lo, opts=None, rows=None):
    b, a = D.one_step(prt, case, real_t, opts, "raw_")
    return D.reference(case, b, a, lo, rows), b, a


# ---------------------------------------------------------------------------------------------------- 1. droplet by droplet
@pytest.mark.parametrize("dims", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_every_droplet_of_one_step(real_t, scheme, dims):
    case = D.design(real_t, dims, adve_scheme=SCHEMES[scheme])
    prt = start(case, real_t, when="before" if dims == 2 else "after")
    assert np.array_equal(prt.state_u64("raw_ijk"), case["cells"])
    rows, b, a = tallied_step(prt, case, real_t, MV.bounds(THR, real_t))
    print(real_t.__name__, scheme, "%d-D" % dims, rows.events, "slots kept" if a["n"].size == b["n"].size else "compacted")
    if scheme == "euler":
        assert occurred(rows) and a["n"].size == b["n"].size, "the design's step, slot for slot (tests/test_move_rates_design.py)"
    assert rows.events["stay"] and rows.events["moved"] and rows.events["bottom"] and rows.events["top"]
    assert prt.move_rates_info() == (True, tuple(THR), 1)
    got = as_block(prt)
    assert_rows(got, rows, "%s %s %d-D" % (real_t.__name__, scheme, dims))
    if dims == 2 and scheme == "euler":
        assert (got[:, 10] == 0).all(), "the still cell"


# ---------------------------------------------------------------------------------------------------- 2. storage order, dead slots
def interleaved(case, occ):
    cells = case["cells"]
    rank = np.arange(cells.size) - np.concatenate(([0], np.cumsum(occ)))[cells]
    return D.permuted(case, np.lexsort((cells, rank)))


@pytest.mark.parametrize("dims", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_cells_interleaved_in_storage(real_t, dims):
    """the same droplets, stored by their rank in the cell first: adjacent slots lie in different cells, so runs have length 1"""
    case = interleaved(D.design(real_t, dims), D.OCC if dims == 2 else D.OCC3)
    assert (np.diff(case["cells"][:14]) != 0).all()
    prt = start(case, real_t)
    assert np.array_equal(prt.state_u64("raw_ijk"), case["cells"])
    rows, _, _ = tallied_step(prt, case, real_t, MV.bounds(THR, real_t))
    assert occurred(rows)
    assert_rows(as_block(prt), rows, "%s %d-D interleaved" % (real_t.__name__, dims))


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_dead_slots_in_the_middle_of_the_storage(real_t):
    case = D.design(real_t)
    dead = np.zeros(case["cells"].size, dtype=bool)
    dead[5::37] = True
    dead[200:203] = True
    case["args"]["n"] = np.where(dead, 0, case["args"]["n"]).astype(np.uint64)
    prt = start(case, real_t)
    assert np.array_equal(prt.state_u64("raw_n") == 0, dead), "set_particles keeps the n = 0 entries where they are"
    rows, b, a = tallied_step(prt, case, real_t, MV.bounds(THR, real_t))
    assert rows.events["moved"] and rows.events["bottom"] and rows.events["top"]
    assert_rows(as_block(prt), rows, "%s dead slots" % real_t.__name__)


# ---------------------------------------------------------------------------------------------------- the default box
def rainy_box(real_t, thr=None, seed=7, nxyz=8, per_cell=16, **kw):
    """an 8 x 8 x 8 x 16 box of 1 m cells with the API's default arithmetic: box_fields' air and Courant numbers (|C| <= 0.35), radii
    log-uniform in 5 ... 80 um with a tenth of them within 0.5 % of 25 um (condensation carries some across), multiplicities as in
    test_hip_coal_rates.production_case (a few per cent of the pairs collide in a step)"""
    oi = h.api_default_opts(h.box_opts(nxyz, nxyz, nxyz, per_cell, dx=1., dt=1., kernel=lgrngn.kernel_t.hall, terminal_velocity=lgrngn.vt_t.beard77fast, **kw))
    th, rv, rhod, Cc = h.box_fields(oi)
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    fields = (f(th), f(rv), f(rhod), {k: f(v) for k, v in Cc.items()})
    rng = np.random.default_rng(seed)
    n_cell = nxyz ** 3
    cells = np.repeat(np.arange(n_cell), per_cell)
    N = cells.size
    r = np.exp(rng.uniform(np.log(5e-6), np.log(80e-6), N))
    near = rng.random(N) < .1
    r[near] = 25e-6 * (1 + rng.uniform(-5e-3, 5e-3, near.sum()))
    n = rng.integers(125000, 500000, N).astype(np.uint64)
    n[(r > 19.9e-6) & (r < 25e-6)] *= np.uint64(400)
    i, j, k = cells // (nxyz * nxyz), (cells // nxyz) % nxyz, cells % nxyz
    args = dict(n=n, rd3=(1e-8 * (1 + np.arange(N) / 7.)) ** 3, rw2=((r.astype(LD) ** 2).astype(real_t)).astype(np.float64), kpa=np.full(N, .5),
                vt=np.full(N, .1), x=i + rng.uniform(.05, .95, N), y=j + rng.uniform(.05, .95, N), z=k + rng.uniform(.05, .95, N))
    prt = h.hip_particles(oi, real_t)
    prt.init(fields[0].copy(), fields[1].copy(), fields[2].copy(), **{kk: v.copy() for kk, v in fields[3].items()})
    if thr is not None:
        prt.move_rates_enable(thr)
    prt.set_particles(**args)
    box = MV.Box(nxyz, nxyz, nxyz, x1=float(nxyz), y1=float(nxyz), z1=float(nxyz), open_side_walls=bool(oi.open_side_walls),
                 periodic_topbot=bool(oi.periodic_topbot_walls))
    return prt, fields, dict(oi=oi, fields=fields, box=box, args=args, cells=cells)


def full_step(prt, fields, opts):
    th, rv, rhod, Cc = fields
    prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    prt.step_async(opts)


# ---------------------------------------------------------------------------------------------------- 3. the ground
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_precip_is_what_the_puddle_receives_and_the_domain_closes(real_t):
    thr = [0., 25e-6, 60e-6]
    prt, fields, case = rainy_box(real_t, thr, reorder_every=-1)
    lo = MV.bounds(thr, real_t)
    opts = D.move_only()
    pud0 = prt.diag_puddle()
    removed = [0, 0, 0]
    k_precip = 0
    for s in range(3):
        b, a = D.one_step(prt, case, real_t, opts, "raw_")
        n1, _, _ = D.aligned(b, a)
        for t in range(3):
            removed[t] += int(b["n"][(n1 == 0) & (b["n"] != 0) & (b["rw2"] >= lo[t])].astype(object).sum())
        k_precip += int(((n1 == 0) & (b["n"] != 0)).sum())
    pud1 = prt.diag_puddle()
    got = prt.move_rates()
    assert prt.move_rates_info()[2] == 3
    d_num = pud1["particle_number"] - pud0["particle_number"]
    assert d_num > 0 and int(got["precip_n"][0].sum()) == int(d_num), (got["precip_n"][0].sum(), d_num)
    nz = 8
    assert (got["precip_n"][:, np.arange(512) % nz != 0] == 0).all(), "precipitation is booked at the foot of the column"
    assert (got["precip_n"][0].reshape(64, nz)[:, 0] > 0).sum() > 1, "a map, not a total"
    vol = LD(4) / 3 * LD(np.pi) * got["precip_m3"][0].astype(LD).sum()
    d_vol = LD(pud1["liquid_volume"]) - LD(pud0["liquid_volume"])
    # the tally's bar, (K_c + 8) eps S over the droplets that left (no more than all that were removed), and the puddle's own rounding:
    # it computes every term 4/3 pi n pow(rw2, 3/2) in the object's real type (a few eps_T each) and sums them in double
    bar = (k_precip + 8) * LD(np.finfo(np.float64).eps) * vol + 8 * LD(np.finfo(real_t).eps) * vol
    print(real_t.__name__, "puddle: particles +%d, liquid volume +%.6e, tally %.6e, |difference| / bar %.3f" % (d_num, float(d_vol), float(vol), float(abs(vol - d_vol) / bar)))
    assert abs(vol - d_vol) <= bar
    for t in range(3):
        assert int(got["in_n"][t].sum()) == int(got["out_n"][t].sum()) - removed[t] and removed[t] > 0, t
        assert (got["down_n"][t] <= got["out_n"][t]).all() and (got["up_n"][t] <= got["out_n"][t]).all()


# ---------------------------------------------------------------------------------------------------- 4. the plain sequence
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_a_step_with_rcyc_takes_the_plain_sequence(real_t):
    case = D.design(real_t)
    prt = start(case, real_t)
    rows, b, a = tallied_step(prt, case, real_t, MV.bounds(THR, real_t), D.move_only(rcyc=True))
    print(real_t.__name__, "rcyc", rows.events, "slots", b["n"].size, "->", a["n"].size)
    assert rows.events["moved"] and rows.events["bottom"] and rows.events["top"]
    assert_rows(as_block(prt), rows, "%s rcyc" % real_t.__name__)


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_a_firing_matching_source_takes_the_plain_sequence_and_newcomers_are_not_arrivals(real_t):
    case = D.design(real_t, src_type=lgrngn.src_t.matching, src_x0=0., src_x1=4., src_z0=0., src_z1=4., n_sd_max=sum(D.OCC) + 16 * 8 + 64)
    prt = start(case, real_t)
    opts = D.move_only(src=True, src_dry_distros={(.61, 0.): (h.lognormal_fn(.05e-6, 1.4, 60e4), 8, 1)})
    rows, b, a = tallied_step(prt, case, real_t, MV.bounds(THR, real_t), opts)
    assert a["n"].size > b["n"].size - 16 and (~np.isin(a["rd3"], b["rd3"])).any(), "the source fired"
    new = ~np.isin(a["rd3"], b["rd3"])
    print(real_t.__name__, "matching source", rows.events, "slots", b["n"].size, "->", a["n"].size, "newcomers", int(new.sum()))
    assert rows.events["moved"] and rows.events["bottom"] and rows.events["top"]
    assert_rows(as_block(prt), rows, "%s matching source" % real_t.__name__)


# ---------------------------------------------------------------------------------------------------- 5. the other moves
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_open_side_walls(real_t):
    case = D.design(real_t, open_side_walls=True)
    prt = start(case, real_t)
    rows, b, a = tallied_step(prt, case, real_t, MV.bounds(THR, real_t))
    print(real_t.__name__, "open side walls", rows.events)
    assert a["n"].size == b["n"].size, "slots kept: the removed droplets' last positions name their exits"
    assert rows.events["side"] >= 1 and rows.events["bottom"] >= 1 and rows.events["top"] >= 1 and rows.events["moved"] >= 1
    assert_rows(as_block(prt), rows, "%s open side walls" % real_t.__name__)


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_periodic_topbot_walls(real_t):
    case = D.design(real_t, periodic_topbot_walls=True)
    prt = start(case, real_t)
    rows, b, a = tallied_step(prt, case, real_t, MV.bounds(THR, real_t))
    n1, ijk1, _ = D.aligned(b, a)
    wrapped = (n1 != 0) & (np.abs(b["ijk"] % 4 - ijk1 % 4) == 3)
    print(real_t.__name__, "periodic top and bottom", rows.events, "wrapped", int(wrapped.sum()))
    assert rows.events["bottom"] == 0 and rows.events["top"] == 0 and wrapped.sum() >= 2, "nothing is removed; wraps read as the opposite direction"
    got = as_block(prt)
    assert (got[MV.PRECIP_N::10] == 0).all()
    assert_rows(got, rows, "%s periodic top and bottom" % real_t.__name__)


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_subsidence(real_t):
    case = D.design(real_t, subs_switch=True, w_LS=np.full(4, .3))
    plain = D.design(real_t)
    res = []
    for cs, opts in ((case, D.move_only(subs=True)), (plain, D.move_only())):
        prt = start(cs, real_t)
        rows, b, a = tallied_step(prt, cs, real_t, MV.bounds(THR, real_t), opts)
        assert_rows(as_block(prt), rows, "%s subsidence %s" % (real_t.__name__, opts.subs))
        res.append(rows.block()[MV.DOWN_N].sum())
    assert res[0] > res[1], "subsidence carried more droplets down"


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_turb_adve_against_the_devices_own_cells(real_t):
    case = D.design(real_t, dims=3, turb_adve_switch=True, SGS_mix_len=np.full(4, 1.))
    prt = start(case, real_t)
    th, rv, rhod, Cc = case["fields"]
    opts = D.move_only(turb_adve=True)
    diss = np.ascontiguousarray(np.full(rhod.shape, 1e-2), dtype=real_t)
    prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), diss_rate=diss)
    b = D.raw(prt, real_t, "raw_")
    prt.step_async(opts)
    a = D.raw(prt, real_t, "raw_")
    rows = D.reference(case, b, a, MV.bounds(THR, real_t))
    print(real_t.__name__, "turb_adve", rows.events)
    assert rows.events["moved"] and rows.events["stay"]
    assert_rows(as_block(prt), rows, "%s turb_adve" % real_t.__name__)


# ---------------------------------------------------------------------------------------------------- 6. several steps, reset
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_three_steps_read_once_and_with_a_reset_in_between(real_t):
    lo = MV.bounds(THR, real_t)
    blocks = []
    for reset_after_first in (False, True):
        case = D.design(real_t)
        prt = start(case, real_t)
        refs = [MV.Rows(3, 16), MV.Rows(3, 16)]
        whole = MV.Rows(3, 16)
        reads = []
        for s in range(3):
            b, a = D.one_step(prt, case, real_t, None, "raw_")
            for r in (whole, refs[0 if s == 0 else 1]):
                D.reference(case, b, a, lo, r)
            if reset_after_first and s == 0:
                assert prt.move_rates_info()[2] == 1
                reads.append(prt.move_rates(reset=True, out=np.zeros((30, 16))))
                assert prt.move_rates_info()[2] == 0
        if reset_after_first:
            assert prt.move_rates_info()[2] == 2
            reads.append(as_block(prt))
            assert_rows(reads[0], refs[0], "%s first step" % real_t.__name__)
            assert_rows(reads[1], refs[1], "%s steps two and three" % real_t.__name__)
            blocks.append(reads[0] + reads[1])
        else:
            assert prt.move_rates_info()[2] == 3
            blocks.append(as_block(prt))
            assert_rows(blocks[0], whole, "%s three steps" % real_t.__name__)
    once, summed = blocks
    for w in range(30):
        if whole.is_number(w):
            assert np.array_equal(once[w], summed[w]), w
        else:
            for c in range(16):
                assert abs(LD(once[w, c]) - LD(summed[w, c])) <= 2 * MV.m3_bar(whole, w, c), (w, c)


# ---------------------------------------------------------------------------------------------------- 7. the full closure
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_number_of_rain_drops_closes_in_integers_with_everything_on(real_t):
    prt, fields, case = rainy_box(real_t, [TCR.R_THR])
    prt.cond_rates_enable(TCR.R_THR)
    prt.coal_rates_enable(TCR.R_THR)
    opts = lgrngn.opts_t()
    assert opts.adve and opts.sedi and opts.cond and opts.coal
    before = TCR.class_sums(prt, real_t, 512)
    for s in range(3):
        full_step(prt, fields, opts)
    after = TCR.class_sums(prt, real_t, 512)
    cd, cl, mv = prt.cond_rates(), prt.coal_rates(), prt.move_rates()
    assert prt.cond_rates_info()[2] == 3 and prt.coal_rates_info()[2] == 3 and prt.move_rates_info()[2] == 3
    for c in range(512):
        want = (int(cd["up_n"][0][c]) - int(cd["down_n"][0][c]) + int(cl["acnv_nr"][c]) - int(cl["self_rain_n"][c]) +
                int(mv["in_n"][0][c]) - int(mv["out_n"][0][c]))
        assert after["Nr"][c] - before["Nr"][c] == want, (c, after["Nr"][c] - before["Nr"][c], want)
    print(real_t.__name__, "crossed up", int(cd["up_n"][0].sum()), "down", int(cd["down_n"][0].sum()), "autoconverted", int(cl["acnv_nr"].sum()),
          "self-collected", int(cl["self_rain_n"].sum()), "arrived", int(mv["in_n"][0].sum()), "left", int(mv["out_n"][0].sum()),
          "onto the ground", int(mv["precip_n"][0].sum()))
    assert cd["up_n"][0].sum() + cd["down_n"][0].sum() > 0, "condensation carried droplets across the threshold"
    assert cl["acnv_nr"].sum() + cl["self_rain_n"].sum() > 0, "collisions changed the number of rain drops"
    assert mv["in_n"][0].sum() > 0 and mv["out_n"][0].sum() > mv["in_n"][0].sum() and mv["precip_n"][0].sum() > 0, "and rain moved and fell out"


# ---------------------------------------------------------------------------------------------------- 8. nothing else moves
def whole_state(prt):
    names = ("raw_n", "raw_rw2", "raw_rd3", "raw_ijk", "raw_x", "raw_y", "raw_z", "th", "rv")
    out = {nm: prt.state_u64(nm) if nm in ("raw_n", "raw_ijk") else prt.state_real(nm) for nm in names}
    out["puddle"] = np.array(list(prt.diag_puddle().values()))
    return out


@pytest.mark.parametrize("dims", [2, 3], ids=["2d", "3d"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_design_steps_move_nothing_else(real_t, dims):
    res = []
    for thr in (THR, None):
        case = D.design(real_t, dims)
        prt = start(case, real_t, thr)
        out = {}
        for s in range(2):
            D.one_step(prt, case, real_t, None, "raw_")
            out[s] = whole_state(prt)
        res.append(out)
    for s in res[0]:
        for nm in res[0][s]:
            assert np.array_equal(res[0][s][nm], res[1][s][nm]), (s, nm)


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_the_default_box_moves_nothing_else_and_the_next_coalescence_is_the_same(real_t):
    res = []
    for thr in ([0., 25e-6], None):
        prt, fields, _ = rainy_box(real_t, thr)
        opts = lgrngn.opts_t()
        out = {}
        for s in range(3):
            full_step(prt, fields, opts)                                # condensation, coalescence, advection and sedimentation of the API's defaults
            out[s] = whole_state(prt)
        res.append(out)
        if thr is not None:
            assert prt.move_rates_info()[2] == 3
    for s in res[0]:
        for nm in res[0][s]:
            assert np.array_equal(res[0][s][nm], res[1][s][nm]), (s, nm)
    a, b = res[0][0]["raw_n"], res[0][2]["raw_n"]
    assert a.size != b.size or not np.array_equal(a, b), "the coalescence did collide"


# ---------------------------------------------------------------------------------------------------- 9. launch counts
def launches_of_three_steps(prt, fields):
    th, rv, rhod, Cc = fields
    opts = lgrngn.opts_t()
    per_step = []
    for s in range(3):
        n0 = int(prt.state_u64("raw_launches")[0])
        prt.step_sync(opts, th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
        n1 = int(prt.state_u64("raw_launches")[0])
        prt.step_async(opts)
        per_step.append((n1 - n0, int(prt.state_u64("raw_launches")[0]) - n1))
    return per_step


def test_launch_counts():
    never, fields, _ = rainy_box(np.float64, None)
    n_never = launches_of_three_steps(never, fields)
    gone, fields, _ = rainy_box(np.float64, THR)
    gone.move_rates_disable()
    assert gone.move_rates_info() == (False, (), 0)
    n_gone = launches_of_three_steps(gone, fields)
    on, fields, _ = rainy_box(np.float64, [25e-6])
    n_on = launches_of_three_steps(on, fields)
    print("launches per (step_sync, step_async): never enabled", n_never, "disabled", n_gone, "enabled", n_on)
    assert n_never == n_gone, "a disabled object launches what a never-enabled one does"
    for (s_on, a_on), (s_off, a_off) in zip(n_on, n_never):
        assert s_on == s_off and a_on == a_off + 1, "one more launch per tallied move (k_move_rates; the two copies are none), none in step_sync"


# ---------------------------------------------------------------------------------------------------- 10. outbuf, device output
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_diag_move_rate_and_device_output(real_t):
    import torch
    case = D.design(real_t)
    prt = start(case, real_t)
    D.one_step(prt, case, real_t, None, "raw_")
    got = as_block(prt)
    assert (got.sum(1) > 0).all()
    dv, rhod = prt.state_real("dv").astype(real_t), prt.state_real("rhod").astype(real_t)
    for row in range(30):
        if row % 3:
            prt.diag_move_rate(lgrngn.MOVE_RATES[row % 10], row // 10)
        else:
            prt.diag_move_rate(row)
        out = np.frombuffer(prt.outbuf(), dtype=real_t).copy()
        want = (got[row].astype(real_t) / dv) / rhod                   # (the division in the object's type, by dv and then by rhod)
        assert np.array_equal(out, want), row
    buf = torch.full((30, 24), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    prt.move_rates(out=lgrngn.DeviceArray(buf.data_ptr(), (30, 16), (24, 1)))
    host = buf.cpu().numpy()
    assert np.array_equal(host[:, :16], got)
    assert (host[:, 16:] == -1).all(), "the elements between n_cell and the stride are not written"
    wide = np.full((30, 20), -2.)
    prt.move_rates(out=wide[:, :16])
    assert np.array_equal(wide[:, :16], got) and (wide[:, 16:] == -2).all()


# ---------------------------------------------------------------------------------------------------- 11. the surface
def test_every_error_text():
    case = D.design(np.float64)
    prt = h.hip_particles(case["oi"], np.float64)
    f = lambda name: getattr(prt._lib, "lcx_" + name)
    last = prt._f("last_error")
    last.restype = C.c_char_p
    arr = lambda *v: (C.c_double * len(v))(*v)
    for call in (prt.move_rates, lambda: prt.diag_move_rate("in_n"), lambda: prt.diag_move_rate(0)):
        with pytest.raises(RuntimeError, match=r"libcloudph\+\+: move_rates: .* while the tally is not enabled"):
            call()
    for k in (0, 5, -1):
        assert f("move_rates_enable")(prt._h, arr(1e-6, 2e-6, 3e-6, 4e-6, 5e-6), C.c_int(k)) == 1
        assert "libcloudph++: move_rates: n_thr = %d is outside 1 .. 4" % k in last().decode()
    for bad in (-1e-6, float("nan"), float("inf")):
        assert f("move_rates_enable")(prt._h, arr(1e-6, bad), C.c_int(2)) == 1
        assert "libcloudph++: move_rates: every threshold must be non-negative and finite" in last().decode()
    for bad in ((2e-6, 1e-6), (1e-6, 1e-6), (0., 0.)):
        assert f("move_rates_enable")(prt._h, arr(*bad), C.c_int(2)) == 1
        assert "libcloudph++: move_rates: the thresholds must be strictly increasing" in last().decode()
    assert prt.move_rates_info() == (False, (), 0)
    prt.move_rates_enable(THR)                                          # before init()
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: move_rates: diag_move_rate before init\(\)"):
        prt.diag_move_rate("in_n")
    th, rv, rhod, Cc = case["fields"]
    prt.init(th.copy(), rv.copy(), rhod.copy(), **{k: v.copy() for k, v in Cc.items()})
    out = np.zeros((30, 16))
    for row in (-1, 30):
        assert f("diag_move_rate")(prt._h, C.c_int(row)) == 1 and "libcloudph++: move_rates: row = %d is outside 0 .. 29" % row in last().decode()
    assert f("move_rates_read")(prt._h, C.c_void_p(out.ctypes.data), C.c_size_t(15), C.c_int(0), C.c_int(0)) == 1
    assert "libcloudph++: move_rates: stride (15) < n_cell (16)" in last().decode()
    assert f("move_rates_read")(prt._h, None, C.c_size_t(16), C.c_int(0), C.c_int(0)) == 1 and "libcloudph++: move_rates: out == NULL" in last().decode()
    assert f("move_rates_read")(prt._h, C.c_void_p(out.ctypes.data), C.c_size_t(16), C.c_int(0), C.c_int(0)) == 0
    # two radii that differ in double and whose squares are one float
    close = (1e-6, 1e-6 * (1 + 1e-9))
    prt.move_rates_enable(close)
    assert prt.move_rates_info()[1] == close
    p32 = h.hip_particles(D.design(np.float32)["oi"], np.float32)
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: move_rates: the bounds r_thr\^2 of thresholds 0 and 1 are not strictly increasing in the object's real type"):
        p32.move_rates_enable(close)
    assert p32.move_rates_info()[0] is False


def test_a_multi_device_object_is_refused(monkeypatch):
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    oi = h.box_opts(4, 4, 4, 16)
    oi.dev_count = 2
    prt = lgrngn.factory(lgrngn.backend_t.multi_HIP, oi)
    assert prt.dev_count == 2
    for call in (lambda: prt.move_rates_enable(THR), prt.move_rates_disable, prt.move_rates_info, prt.move_rates, lambda: prt.diag_move_rate(0)):
        with pytest.raises(RuntimeError, match=r"libcloudph\+\+: move_rates on a multi-device object is not built"):
            call()


def test_a_slab_with_neighbours_is_refused():
    oi = h.box_opts(4, 4, 4, 16)
    oi.bcond_lft = oi.bcond_rgt = 1                                     # (distmem: the slab's side walls hand droplets to neighbours)
    prt = h.hip_particles(oi)
    with pytest.raises(RuntimeError, match=r"libcloudph\+\+: move_rates on a decomposed domain is not built"):
        prt.move_rates_enable(THR)
    assert prt.move_rates_info() == (False, (), 0)


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_enable_again_with_other_thresholds_and_disable(real_t):
    case = D.design(real_t)
    prt = start(case, real_t, when="before")
    tallied_step(prt, case, real_t, MV.bounds(THR, real_t))
    assert (as_block(prt) != 0).any()
    prt.move_rates_enable(25e-6)                                        # other thresholds on an enabled object: zeroed, K = 1
    assert prt.move_rates_info() == (True, (25e-6,), 0)
    assert as_block(prt).shape == (10, 16) and (as_block(prt) == 0).all()
    rows, _, _ = tallied_step(prt, case, real_t, MV.bounds([25e-6], real_t))
    assert_rows(as_block(prt), rows, "%s K = 1" % real_t.__name__)
    four = [0., 10e-6, 25e-6, 60e-6]
    prt.move_rates_enable(four)                                         # K = 4
    rows, _, _ = tallied_step(prt, case, real_t, MV.bounds(four, real_t))
    assert as_block(prt).shape == (40, 16)
    assert_rows(as_block(prt), rows, "%s K = 4" % real_t.__name__)
    # rows 32 .. 39 exist only at K = 4 (a mask of the count rows needs 64 bits for them): single rows, and the 40 rows into device memory
    import torch
    block = as_block(prt)
    assert any((block[row] != 0).any() for row in (32, 38, 39)), "droplets above 60 um moved in this step: not zeros against zeros"
    dv, rhod = prt.state_real("dv").astype(real_t), prt.state_real("rhod").astype(real_t)
    for row in (31, 32, 38, 39):                                        # (even rows are counts, odd rows sums of m r^3)
        prt.diag_move_rate(row)
        out = np.frombuffer(prt.outbuf(), dtype=real_t).copy()
        assert np.array_equal(out, (block[row].astype(real_t) / dv) / rhod), row
    buf = torch.full((40, 24), -1., dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    prt.move_rates(out=lgrngn.DeviceArray(buf.data_ptr(), (40, 16), (24, 1)))
    host = buf.cpu().numpy()
    assert np.array_equal(host[:, :16], block)
    assert (host[:, 16:] == -1).all(), "the elements between n_cell and the stride are not written"
    prt.move_rates_disable()
    assert prt.move_rates_info() == (False, (), 0)
    with pytest.raises(RuntimeError, match="not enabled"):
        prt.move_rates()


@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_a_snapshot_drops_the_tally_and_the_run_goes_on(real_t):
    prt, fields, case = rainy_box(real_t, THR)
    opts = lgrngn.opts_t()
    full_step(prt, fields, opts)
    blob = prt.snapshot()
    assert prt.move_rates_info() == (True, tuple(THR), 1), "taking a snapshot leaves the tally as it is"
    twin = h.hip_particles(case["oi"], real_t)
    twin.move_rates_enable([25e-6])                                     # (enabled before the load: a restored object starts disabled all the same)
    twin.restore(blob)
    assert twin.move_rates_info() == (False, (), 0)
    with pytest.raises(RuntimeError, match="not enabled"):
        twin.move_rates()
    for p in (prt, twin):
        full_step(p, fields, opts)
    a, b = whole_state(prt), whole_state(twin)
    for nm in a:
        assert np.array_equal(a[nm], b[nm]), nm
    assert prt.move_rates_info()[2] == 2 and (prt.move_rates()["out_n"] != 0).any()


def test_a_parcel_enables_and_stays_zero():
    oi = lgrngn.opts_init_t()
    oi.dt, oi.sd_conc, oi.n_sd_max = 1., 64, 64
    oi.dry_distros = {(.61, 0.): h.lgrngn_bimodal()}
    oi.coal_switch = oi.sedi_switch = False
    prt = h.hip_particles(oi)
    prt.init(np.array([300.]), np.array([.010]), np.array([1.1]))
    prt.move_rates_enable([0.])
    opts = lgrngn.opts_t()
    opts.coal = opts.sedi = opts.adve = False
    for s in range(2):
        prt.step_sync(opts, np.array([300.]), np.array([.012]), np.array([1.1]))
        prt.step_async(opts)
    assert prt.move_rates_info() == (True, (0.,), 2)
    assert as_block(prt).shape == (10, 1) and (as_block(prt) == 0).all()
    prt.diag_move_rate("out_n")
    assert np.frombuffer(prt.outbuf(), dtype=np.float64)[0] == 0
