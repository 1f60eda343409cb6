"""The diagnostics of the CPU oracle (double and float) against tests/_diag_reference.py, a plain long-double statement of each
diag_* call written from the reference's sources, on crafted states with very uneven cells.  tests/test_hip_diagnostics.py runs the
same cases (CASES, run_case below) through the HIP object; here they prove the reference module and the crafted inputs without a GPU
and give the oracle a check that is not its own author's reading.

Shapes (each the smallest that reaches its branch of k_cell_seqsum / cf_cells, lcx_kernels.hpp, lcx_core.hip):
  A   2-D 9 x 30 = 270 cells, cf_cells() == 64: a workgroup's 64 cells hold exactly CF_CAP = 2048 values, 2049, one cell of 2100
      between empty neighbours, sparse cells with empty cells at the group's edges, and the partial last group with the domain's last
      cell empty (A1) or holding the whole group (A2)
  B   3-D 1 x 2 x 3 at ~300 per cell (five cells per group), two cells of 2100 (one per group, never staged), 0-D (not specific)
  C   knife edges of [min, max) at powers of two, 0-D so that the counts are exact
  D   SGS velocities of both signs after two turb_adve steps: odd moments
  E   dead slots in the storage and an object nobody has read
Tolerances: see check().
"""
import numpy as np
import pytest

import _diag_reference as R
import _harness as h
from libcloudphxx_amd import lgrngn

LD = np.longdouble
ORACLES = {np.float64: h.oracle_particles, np.float32: h.oracle_f32_particles}

# wet_mass_dens, T, p, RH are chains of transcendental functions without a simple bound: measured worst |oracle - reference| of the
# CPU oracle of the same type over all cases below, in units of eps * scale (scale: |reference| of T, p, RH; the scaled sum of |term|
# of wet_mass_dens), and the bar given to every object: 8 x that, never below 16.
MEASURED = {np.float64: {"temperature": 2.5, "pressure": 3.4, "RH": 49.1, "wet_mass_dens": 273.3},
            np.float32: {"temperature": 4.3, "pressure": 5.3, "RH": 80.2, "wet_mass_dens": 86.5}}
BARS = {t: {k: max(16., 8. * v) for k, v in m.items()} for t, m in MEASURED.items()}


# ---------------------------------------------------------------------------------------------------- crafted states
def cast_fields(fields, real_t):
    th, rv, rhod, C = fields
    f = lambda a: np.ascontiguousarray(a, dtype=real_t)
    return f(th), f(rv), f(rhod), {k: f(v) for k, v in C.items()}


def crafted(oi, fields, counts, real_t, seed, zero_rw=False):
    """set_particles arguments for counts[c] super-droplets in cell c, storage order shuffled, each strictly inside its cell (1 %
    margin); multiplicities 1 .. 1e9 with every 17th at 0; three kappas; dry radii 1e-9 .. 1e-6 m, wet up to 1e3 times the dry;
    no super-droplet near the thresholds of diag_RH_ge_Sc / diag_rw_ge_rc (moved away where the draw put one there)"""
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.arange(len(counts)), counts)
    cells = cells[rng.permutation(cells.size)]
    N = cells.size
    n = np.floor(10 ** (9 * rng.random(N))).astype(np.uint64)
    n[1], n[2] = 1, 10 ** 9
    n[::17] = 0
    rd = 10 ** rng.uniform(-9, -6, N)
    rw = rd * 10 ** rng.uniform(0, 3, N)
    kappa = rng.choice([.3, .5, 1.28], N).astype(real_t)
    rd3, rw2 = (rd ** 3).astype(real_t), (rw ** 2).astype(real_t)
    th, rv, rhod, _ = cast_fields(fields, real_t)
    T = R.T_of(th.ravel().astype(LD), rhod.ravel().astype(LD))
    RH = R.RH_of(R.p_of(rhod.ravel().astype(LD), rv.ravel().astype(LD), T), rv.ravel().astype(LD), T)
    S = R.S_cr(rd3.astype(LD), kappa.astype(LD), T[cells])
    near = np.abs(RH[cells] - S) / S < 1e-4
    rd3[near] = (rd3[near] * 1.01).astype(real_t)
    rc2 = R.rw3_cr(rd3.astype(LD), kappa.astype(LD), T[cells]) ** (LD(2) / 3)
    near = np.abs(rw2.astype(LD) - rc2) / rc2 < 1e-3
    rw2[near] = (rw2[near] * 1.01).astype(real_t)
    if zero_rw:
        rw2[5::23] = 0
    nx, ny, nz = oi.nx, oi.ny, oi.nz
    pos = {}
    if nx:
        i = cells // (max(ny, 1) * max(nz, 1))
        pos["x"] = (i + .01 + .98 * rng.random(N)) * oi.dx
    if ny:
        pos["y"] = ((cells // nz) % ny + .01 + .98 * rng.random(N)) * oi.dy
    if nz:
        pos["z"] = (cells % nz + .01 + .98 * rng.random(N)) * oi.dz
    return dict(n=n, rd3=rd3, rw2=rw2, kpa=kappa, vt=np.full(N, -1.), **pos), cells


def counts_A(last_group_in_last_cell):
    c = np.zeros(270, dtype=int)
    c[0:64] = 32                                          # a group total of exactly 2048: staged
    c[64:128] = 32                                        # 2049, unevenly: not staged
    c[64], c[127], c[100] = 12, 52, 33
    c[128:192] = np.arange(128, 192) % 3 + 1              # sparse around one cell above the cap with empty neighbours
    c[159], c[160], c[161] = 0, 2100, 0
    c[192:256] = np.arange(192, 256) % 4                  # sparse, empty cells at both edges of the group
    c[192] = c[255] = 0
    if last_group_in_last_cell:
        c[269] = 40
    else:
        c[256:270] = np.arange(256, 270) % 5 + 1
        c[269] = 0                                        # the domain's last cell empty
    assert c[0:64].sum() == 2048 and c[64:128].sum() == 2049
    return c


def standard_calls(real_t, zero_rw=False, extra=()):
    """(selection steps, counting call): every diagnostic on a state with rd3, rw2, kappa"""
    ALL = [("all",)]
    wet_k = [-1, 0, 1, 2, 3] + ([6] if real_t is np.float64 else [])      # (float: rw^6 leaves the normal range, not requested)
    if zero_rw:
        wet_k.remove(-1)                                                  # (0^(-1/2) is infinite in any arithmetic)
    calls = [(ALL, ("sd_conc",))]
    calls += [(ALL, ("mom", "wet", k)) for k in wet_k]
    calls += [(ALL, ("mom", "dry", k)) for k in (0, 1, 2, 3)]
    calls += [(ALL, ("mom", "kappa", k)) for k in (1, 2)]
    three = [("rng", "dry", 2e-8, 5e-7, False), ("rng", "wet", 1e-7, 1e-4, True), ("rng", "kappa", .2, .7, True)]
    calls += [(three, ("mom", "wet", 0)), (three, ("sd_conc",)), (three, ("mom", "wet", 3))]
    behind = [("rng", "kappa", .5, 1.5, False), ("rng", "dry", 5e-9, 3e-7, True), ("water", True)]
    calls += [(behind, ("mom", "dry", 3)), (behind, ("sd_conc",))]
    nothing = [("rng", "wet", 1e-7, 1e-5, False), ("rng", "wet", 1e-3, 1., True), ("rng", "dry", 0., 1., True)]
    calls += [(nothing, ("mom", "wet", 1)), (nothing, ("sd_conc",))]
    calls += [([("water", False)], ("mom", "wet", 2)), ([("water", False)], ("sd_conc",))]
    calls += [([("rng", "wet", .5e-6, 25e-6, False)], ("mom", "wet", 3)), ([("rng", "kappa", .2, .5, False)], ("mom", "dry", 0)),
              ([("rng", "dry", 1e-8, 1e-7, False)], ("mom", "kappa", 1)),
              ([("all",), ("rng", "kappa", .5, 2., True), ("rng", "wet", 0., 1e-5, True)], ("mom", "wet", 2))]
    calls += [([("RH_ge_Sc",)], ("mom", "wet", 0)), ([("RH_ge_Sc",)], ("sd_conc",)),
              ([("rw_ge_rc",)], ("mom", "wet", 0)), ([("rw_ge_rc",)], ("sd_conc",))]
    calls += [(ALL, ("precip_rate",)), ([("rng", "wet", 1e-6, 1e-4, False)], ("precip_rate",))]
    calls += [(ALL, ("wet_mass_dens", 8e-6, .62)), ([("rng", "wet", 1e-6, 1., False)], ("wet_mass_dens", 2e-6, .4))]
    calls += [([("rng", "wet", 0., 1e-7, False)], ("max_rw",))]            # (a selection that excludes every cell's maximum)
    calls += [([], ("pressure",)), ([], ("temperature",)), ([], ("RH",)), ([], ("vel_div",))]
    return calls + list(extra)


class Case:
    def __init__(self, oi, fields, calls, setup, intended=None, dead_slots=False):
        self.oi, self.fields, self.calls, self.setup, self.intended, self.dead_slots = oi, fields, calls, setup, intended, dead_slots


def _crafted_case(oi, counts, real_t, seed, zero_rw=False):
    fields = cast_fields(h.box_fields(oi), real_t)
    args, cells = crafted(oi, fields, counts, real_t, seed, zero_rw)
    return Case(oi, fields, standard_calls(real_t, zero_rw), lambda prt: prt.set_particles(**args), cells)


def case_A(real_t, variant, api_default=False):
    oi = h.box_opts(9, 0, 30, 24)
    if api_default:
        h.api_default_opts(oi)
    counts = counts_A(variant == 2)
    # cf_cells() (lcx_core.hip) is min(64, 2048 * 4 / 5 / (N / n_cell + 1)): at most 25 per cell on average keeps all 64 cells of a
    # workgroup, which the group totals of counts_A are laid out for
    assert counts.sum() // 270 + 1 <= 25
    return _crafted_case(oi, counts, real_t, 11 + variant)


def case_B(real_t, which):
    if which == "five":                                   # mean 301: cf_cells() == 5, five cells in one group and one in the next
        oi, counts = h.box_opts(1, 2, 3, 320), np.array([300, 287, 0, 411, 350, 452])
    elif which == "big":                                  # mean 2101: cf_cells() == 1, each cell above CF_CAP
        oi, counts = h.box_opts(1, 0, 2, 2200), np.array([2100, 2100])
    else:                                                 # 0-D: one cell, moments not specific
        oi, counts = h.box_opts(0, 0, 0, 400, sedi_switch=False), np.array([300])
    return _crafted_case(oi, counts, real_t, {"five": 21, "big": 22, "parcel": 23}[which], zero_rw=which != "big")


def case_C(real_t):
    """every super-droplet carries its own bit of the multiplicity sum, so a moment 0 names the selected set exactly"""
    oi = h.box_opts(0, 0, 0, 64, sedi_switch=False)
    fields = cast_fields(h.box_fields(oi), real_t)
    T = real_t
    nb = lambda v: [np.nextafter(T(v), T(0)), T(v), np.nextafter(T(v), T(np.inf))]
    wet = nb(2. ** -40) + nb(2. ** -38)
    dry = nb(2. ** -72) + nb(2. ** -66)
    kap = nb(.5) + nb(1.)
    N = 18
    rw2 = np.array(wet + [2. ** -39] * 12, dtype=np.float64)
    rd3 = np.array([2. ** -70] * 6 + dry + [2. ** -70] * 6, dtype=np.float64)
    kpa = np.array([.75] * 12 + kap, dtype=np.float64)
    n = (2 ** np.arange(N)).astype(np.uint64)
    calls = []
    for sel in ([("rng", "wet", 2. ** -20, 2. ** -19, False)], [("rng", "dry", 2. ** -24, 2. ** -22, False)],
                [("rng", "kappa", .5, 1., False)], [("rng", "kappa", .25, .5, False)], [("rng", "dry", 2. ** -30, 2. ** -24, False)],
                [("all",), ("rng", "wet", 2. ** -20, 2. ** -19, True)],
                [("rng", "kappa", .5, 1., False), ("rng", "dry", 2. ** -24, 2. ** -22, True), ("rng", "wet", 2. ** -20, 2. ** -19, True)]):
        calls += [(sel, ("mom", "wet", 0)), (sel, ("sd_conc",))]
    # super-droplets 0-5 / 6-11 / 12-17 sit below, on and above the lower and the upper edge of the wet / dry / kappa range; the other
    # two attributes of each lie inside their ranges.  The lower bound is in, the upper bound is out.
    every = set(range(N))
    out_w, out_d, out_k = {0, 4, 5}, {6, 10, 11}, {12, 16, 17}
    picked = [every - out_w, every - out_d, every - out_k, {12}, {6}, every - out_w, every - out_w - out_d - out_k]
    expect = {}
    for j, pk in enumerate(picked):
        expect[2 * j], expect[2 * j + 1] = sum(2 ** i for i in pk), len(pk)
    c = Case(oi, fields, calls, lambda prt: prt.set_particles(n, rd3, rw2, kpa, np.zeros(N)), np.zeros(N, dtype=int))
    c.expect = expect
    return c


def case_D(real_t):
    oi = h.box_opts(4, 3, 4, 24, coal_switch=False, turb_adve_switch=True, SGS_mix_len=np.linspace(20., 40., 4))
    fields = cast_fields(h.box_fields(oi), real_t)
    th, rv, rhod, C = fields

    def setup(prt):
        opts = lgrngn.opts_t()
        opts.coal = opts.cond = False
        opts.turb_adve = True
        diss = np.full(th.shape, 1e-3, dtype=real_t)
        for _ in range(2):
            prt.step_sync(opts, th.copy(), rv.copy(), rhod, diss_rate=diss, **C)
            prt.step_async(opts)
    calls = [([("all",)], ("mom", a, k)) for a in ("up", "vp", "wp") for k in (1, 2, 3)] + [([("all",)], ("sd_conc",))]
    return Case(oi, fields, calls, setup)


def case_E(real_t):
    """tests/test_hip_parity.py::test_lazy_compaction_is_unobservable, not eager: millimetre drops fall out during six steps and
    leave dead slots; nothing reads the object before the diagnostics have run"""
    oi = h.box_opts(5, 4, 6, 48, dx=30., coal_switch=False, diag_incloud_time=True)
    fields = cast_fields(h.box_fields(oi), real_t)
    th, rv, rhod, C = fields

    def setup(prt):
        g = prt.state_real
        rw2 = g("rw2")
        rw2[::5] = (1.2e-3) ** 2
        prt.set_particles(prt.state_u64("n"), g("rd3"), rw2, g("kappa"), g("vt"), g("x"), g("y"), g("z"))
        opts = lgrngn.opts_t()
        opts.coal = opts.cond = False
        tt, rr = th.copy(), rv.copy()
        for _ in range(6):
            prt.step_sync(opts, tt, rr, rhod, **C)
            prt.step_async(opts)
    calls = standard_calls(real_t, extra=[([("all",)], ("mom", "incloud_time", 1)), ([("rw_ge_rc",)], ("mom", "incloud_time", 1))])
    return Case(oi, fields, calls, setup, dead_slots=True)


CASES = {
    "A1": lambda t: case_A(t, 1), "A2": lambda t: case_A(t, 2), "A1_api_default": lambda t: case_A(t, 1, api_default=True),
    "B_five": lambda t: case_B(t, "five"), "B_big": lambda t: case_B(t, "big"), "B_parcel": lambda t: case_B(t, "parcel"),
    "C": case_C, "D": case_D, "E": case_E,
}


# ---------------------------------------------------------------------------------------------------- running a case
def obj_select(prt, s):
    if s[0] == "all": prt.diag_all()
    elif s[0] == "rng": getattr(prt, "diag_%s_rng%s" % (s[1], "_cons" if s[4] else ""))(s[2], s[3])
    elif s[0] == "water": (prt.diag_water_cons if s[1] else prt.diag_water)()
    else: getattr(prt, "diag_" + s[0])()


def obj_count(prt, c):
    if c[0] == "mom": getattr(prt, "diag_%s_mom" % c[1])(c[2])
    elif c[0] == "wet_mass_dens": prt.diag_wet_mass_dens(c[1], c[2])
    else: getattr(prt, "diag_" + c[0])()


def collect(prt, calls):
    outs = []
    for sel, cnt in calls:
        for s in sel:
            obj_select(prt, s)
        obj_count(prt, cnt)
        outs.append(prt.outbuf_array())
    return outs


def read_state(prt):
    oi = prt.opts_init
    st = {"n": prt.state_u64("n"), "ijk": prt.state_u64("ijk")}
    names = ["rw2", "rd3", "kappa", "vt", "th", "rv", "rhod", "dv"]
    names += [nm for nm, on in (("courant_x", oi.nx), ("courant_y", oi.ny), ("courant_z", oi.nz)) if on]
    if oi.turb_adve_switch:
        names += ["up", "vp", "wp"]
    if oi.diag_incloud_time:
        names += ["incloud_time"]
    for nm in names:
        st[nm] = prt.state_real(nm)
    return st


def check(ref, case, outs, real_t, bars=None, worst=None):
    """|out - ref| per cell, eps = the real type's:
      sd_conc, and moment 0 where it is not specific and the cell's multiplicities add up exactly (below 2^53 / 2^24): exact
      every other moment, precip_rate: (N_c + 8) eps sum|term| -- N_c - 1 for the sequential sum of N_c terms, 8 for pow, T(n), the
          products and the two divisions
      wet_mass_dens: BARS eps sum|term|, plus N_c + 1 underflows (the real type's smallest normal, scaled like the value): the far
          tail of the kernel leaves the normal range in float
      T, p, RH: BARS eps |ref|;  vel_div: 8 eps sum|face term| (three differences, three divisions, two sums)
      max_rw: eps |ref| (one correctly rounded sqrt)
      RH_ge_Sc, rw_ge_rc: exact counts, with no super-droplet of the reference near its threshold
    cells without super-droplets: exactly 0.  worst (a dict) collects the largest |out - ref| / (eps * scale) of the BARS group."""
    fi = np.finfo(real_t)
    eps, tiny = LD(fi.eps), LD(fi.tiny)
    bars = BARS[real_t] if bars is None else bars
    mant = 2 ** (fi.nmant + 1)
    n_live = int((ref.n > 0).sum())
    for i, ((sel, cnt), out) in enumerate(zip(case.calls, outs)):
        tag = "call #%d %r after %r" % (i, cnt, sel)
        assert out.dtype == real_t and out.size == ref.n_cell and np.isfinite(out).all(), tag
        out = out.astype(LD)
        ref.nf = None
        for s in sel:
            if s[0] == "all": ref.all()
            elif s[0] == "rng": ref.rng(s[1], s[2], s[3], s[4])
            elif s[0] == "water": ref.water(s[1])
            else:
                # the library's critical radius is a TOMS748 root to 2^-15 of rw3 (kappa_koehler.hpp:164): it moves rc2 by 2e-5 and,
                # S being flat at its maximum, S_cr by 1e-13 -- so the margins asked here are wider than 64 eps
                margin = ref.RH_ge_Sc() if s[0] == "RH_ge_Sc" else ref.rw_ge_rc()
                assert margin > max(64 * eps, 1e-6 if s[0] == "RH_ge_Sc" else 1e-4), (tag, margin)
                picked = int((ref.nf > 0).sum())
                assert 0 < picked < n_live, (tag, "selection must be neither empty nor everything", picked, n_live)
        empty = ref.count == 0
        if cnt[0] in ("pressure", "temperature", "RH"):
            want = getattr(ref, cnt[0])()
            err = np.abs(out - want) / (eps * np.abs(want))
            if worst is not None:
                worst[cnt[0]] = max(worst.get(cnt[0], 0.), float(err.max()))
            assert (err <= bars[cnt[0]]).all(), (tag, float(err.max()), bars[cnt[0]])
            continue
        if cnt[0] == "vel_div" and ref.n_dims == 0:          # (particles_diag.ipp:503: returns at once, the buffer keeps the last result)
            assert np.array_equal(out, outs[i - 1].astype(LD)), tag
            continue
        if cnt[0] == "vel_div":
            want, mag = ref.vel_div()
            assert (np.abs(out - want) <= 8 * eps * mag).all(), (tag, float(np.max(np.abs(out - want) / (eps * mag + tiny))))
            continue
        if cnt[0] == "max_rw":
            want = ref.max_rw()
            assert (np.abs(out - want) <= eps * want).all(), tag
            assert (out[empty] == 0).all(), tag
            continue
        if cnt[0] == "sd_conc":
            want, mag, N_c = ref.sd_conc()
            tol = np.zeros(ref.n_cell, dtype=LD)
        elif cnt[0] == "mom":
            want, mag, N_c = ref.mom(cnt[1], cnt[2])
            exact = cnt[2] == 0 and ref.n_dims == 0 and (mag < mant).all()
            tol = np.zeros(ref.n_cell, dtype=LD) if exact else (N_c + 8) * eps * mag
        elif cnt[0] == "precip_rate":
            want, mag, N_c = ref.precip_rate()
            assert (ref.vt[ref.rw2 > 0] > 0).all(), "the call must leave fresh terminal velocities (hskpng_vterm_all: where rw2 > 0)"
            tol = (N_c + 8) * eps * mag
        else:
            want, mag, N_c = ref.wet_mass_dens(cnt[1], cnt[2])
            scale = mag + (N_c + 1) * tiny / eps * np.maximum(1, 2 * R.rho_w / ref.dv)
            if worst is not None and (~empty).any():
                worst["wet_mass_dens"] = max(worst.get("wet_mass_dens", 0.), float(np.max(np.abs(out - want)[~empty] / (eps * scale[~empty]))))
            tol = bars["wet_mass_dens"] * eps * scale
        err = np.abs(out - want)
        bad = err > tol
        assert not bad.any(), (tag, "cells", np.nonzero(bad)[0][:8], "err / tol", [float(e / t) if t else float(e) for e, t in zip(err[bad][:8], tol[bad][:8])])
        assert (out[empty] == 0).all(), (tag, "empty cells must give exactly 0")
        if hasattr(case, "expect"):
            assert int(out[0]) == case.expect[i], (tag, int(out[0]), case.expect[i])


def run_case(name, make, real_t, bars=None, worst=None, after=None, raw_storage=False):
    case = CASES[name](real_t)
    oi = case.oi
    th, rv, rhod, C = case.fields
    prt = make(oi, real_t)
    prt.init(th.copy(), rv.copy(), rhod.copy(), **C)
    case.setup(prt)
    outs = collect(prt, case.calls)                       # (no getter before this line in case E)
    raw = prt.state_u64("raw_n").size if case.dead_slots and raw_storage else None
    st = read_state(prt)
    if raw is not None:
        assert raw > prt.n_part, "the storage must still hold dead slots when the diagnostics run"
    if after is not None:
        after(prt)
    if case.intended is not None:
        assert np.array_equal(st["ijk"], case.intended)
    ref = R.DiagRef(st, (oi.nx, oi.ny, oi.nz), oi.dt, real_t)
    if name == "D":
        for a in ("up", "vp", "wp"):
            v = getattr(ref, a)
            assert (v < 0).any() and (v > 0).any(), a
    if name == "E":
        assert len(np.unique(st["incloud_time"])) > 1
    check(ref, case, outs, real_t, bars, worst)
    return ref


@pytest.mark.parametrize("real_t", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_diagnostics_match_the_plain_reference(name, real_t):
    run_case(name, lambda oi, t: ORACLES[t](oi), real_t)
