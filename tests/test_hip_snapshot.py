"""Checkpoint and restart (include/lcx_state.h): prtcls.snapshot() / prtcls.restore(buf).

The bar is bit identity.  Three runs of N + M steps -- A uninterrupted, B that takes a snapshot after step N and goes on, C a fresh
object restored from B's blob that runs the remaining M steps with the caller's fields as B held them -- end in the same bits: the
storage AS IT IS (raw_*: dead slots and storage order included, read first, nothing compacted on the way), every per-droplet
attribute and extra column, the caller's th / rv (and gases), diag_puddle and moments read through outbuf.  Per step the pairs that
collided, the storage extent and the coalescence launches that ranked for themselves / used a bound are equal too, and non-zero on the
production rows: the restored object went down the production path, not a settled fallback.  The mode is read back from the object
(tests/_harness.py pins strict_fp = 1 unless a test says otherwise)."""
import numpy as np
import pytest

import _harness as h
import bench
import test_hip_chemistry as chem
import test_snapshot_format as fmt
from libcloudphxx_amd import lgrngn, multi
from test_hip_coal_skip import assert_same_state

pytestmark = pytest.mark.gpu

REALS = [np.float64, np.float32]
REAL_IDS = ["double", "float"]
MODES = ["strict", "fast_lean", "api_default"]
N16, SD16 = 16, 64
_fields16 = {}


def set_mode(oi, mode):
    if mode == "strict":                        # the parity mode: IEEE order, storage in the reference's id order
        oi.strict_fp, oi.cond_solver, oi.reorder_every = True, 0, -1
    elif mode == "fast_lean":                   # what bench.py's headline runs; default re-ordering
        oi.strict_fp, oi.cond_solver = False, 0
    else:
        h.api_default_opts(oi)
    return oi


def assert_mode_is(prt, mode):
    h.assert_mode(prt, mode == "strict", 1 if mode == "api_default" else 0)


def cast(a, real_t):
    return np.array(a, dtype=real_t, order="C")


class Case:
    """a set-up: options, the caller's fields (th and rv are written by step_sync, the gases by chemistry), the step's options"""

    def __init__(self, oi, th, rv, rhod, C=None, opts=None, extra=None, gases=None, real_t=np.float64, names=()):
        self.oi, self.real_t, self.opts, self.names = oi, np.dtype(real_t), opts or lgrngn.opts_t(), tuple(names)
        self.th0, self.rv0, self.rhod = cast(th, real_t), cast(rv, real_t), cast(rhod, real_t)
        self.C = {k: cast(v, real_t) for k, v in (C or {}).items()}
        self.extra = {k: cast(v, real_t) for k, v in (extra or {}).items()}
        self.gases0 = None if gases is None else [cast(g, real_t) for g in gases]

    class Live:
        pass

    def fresh(self):
        r = Case.Live()
        r.prt = h.hip_particles(self.oi, self.real_t)
        r.th, r.rv = self.th0.copy(), self.rv0.copy()
        r.gases = None if self.gases0 is None else [g.copy() for g in self.gases0]
        r.log = []
        return r

    def amb(self, r):
        return {} if r.gases is None else dict(ambient_chem={lgrngn.chem_species_t(g): r.gases[g] for g in range(6)})

    def init(self, r):
        r.prt.init(r.th, r.rv, self.rhod, **self.C, **self.amb(r))

    def step(self, r, n=1):
        for _ in range(n):
            r.prt.step_sync(self.opts, r.th, r.rv, self.rhod, **self.C, **self.extra, **self.amb(r))
            r.prt.step_async(self.opts)
            p = r.prt
            r.log.append(dict(collided=int(p.state_u64("raw_collided")[0]), ranked=int(p.state_u64("raw_coal_ranked")[0]),
                              skip=int(p.state_u64("raw_coal_skip")[0]), storage=len(p.state_u64("raw_n")), n_part=p.n_part))

    def restored(self, blob, src):
        """a fresh object in the place of init(); the caller's own fields as `src` held them when the blob was taken"""
        r = self.fresh()
        r.prt.restore(blob)
        r.th, r.rv = src["th"].copy(), src["rv"].copy()
        if r.gases is not None:
            r.gases = [g.copy() for g in src["gases"]]
        return r

    def callers_fields(self, r):
        return dict(th=r.th.copy(), rv=r.rv.copy(), gases=None if r.gases is None else [g.copy() for g in r.gases])

    def state(self, r):
        p = r.prt
        st = {"raw_n": p.state_u64("raw_n"), "raw_ijk": p.state_u64("raw_ijk")}       # the storage as it is, first
        for nm in ("raw_rw2", "raw_rd3", "raw_kappa", "raw_vt", "raw_x", "raw_y", "raw_z"):
            st[nm] = p.state_real(nm)
        st.update(n=p.state_u64("n"), ijk=p.state_u64("ijk"), vt=p.state_real("vt"))
        for nm in ("rw2", "rd3", "kappa", "x", "y", "z"):
            st[nm] = p.get_attr(nm)
        for nm in self.names:
            st["sd." + nm] = p.state_real(nm)
        st["th"], st["rv"] = r.th.copy(), r.rv.copy()
        if r.gases is not None:
            for g in range(6):
                st["gas%d" % g] = r.gases[g].copy()
                st["ambient%d" % g] = p.state_real("ambient_" + chem.NAMES[g])
        pud = p.diag_puddle()
        st["puddle"] = np.array([pud[k] for k in sorted(pud)])
        for nm, sel in (("sd_conc", lambda: p.diag_sd_conc()), ("wet_mom0", lambda: p.diag_wet_mom(0)), ("wet_mom3", lambda: p.diag_wet_mom(3)),
                        ("dry_mom1", lambda: p.diag_dry_mom(1))):
            p.diag_all()
            sel()
            st[nm] = p.outbuf_array()
        return st


def abc(case, N, M, after_snapshot=None, before_snapshot=None, skip_may_differ=False):
    """A, B, C as in the module's docstring; returns (A, B, C, blob).  skip_may_differ: a box in which the bound skips next to nothing
    pauses collecting maxima for 32 steps (tests/test_hip_coal_skip.py); the pause is measurement state that a restored object starts
    without (include/lcx_state.h), so C's launches with a bound may differ from A's there -- the results may not"""
    A = case.fresh(); case.init(A); case.step(A, N + M)
    B = case.fresh(); case.init(B); case.step(B, N)
    if before_snapshot:
        before_snapshot(B)
    blob = B.prt.snapshot()
    held, n_part_held = case.callers_fields(B), B.prt.n_part
    assert isinstance(blob, np.ndarray) and blob.dtype == np.uint8 and blob.ndim == 1
    case.step(B, M)
    C = case.restored(blob, held)
    with pytest.raises(RuntimeError, match="init\\(\\) may be called just once"):
        case.init(C)
    assert C.prt.n_part == n_part_held
    case.step(C, M)
    print("A", A.log[N:], "\nB", B.log[N:], "\nC", C.log)
    if skip_may_differ:
        for r in (A, B, C):
            for entry in r.log:
                del entry["skip"]
    assert B.log == A.log and C.log == A.log[N:]
    sa, sb, sc = case.state(A), case.state(B), case.state(C)
    assert_same_state(sa, sb)
    assert_same_state(sa, sc)
    if after_snapshot:
        after_snapshot(A, B, C)
    return A, B, C, blob


# ---------------------------------------------------------------------------------- 1: the 16^3 boxes of bench.py, three arithmetics
def box16(workload, mode, real_t, dt, **kw):
    if not _fields16:
        _fields16["f"] = bench.make_fields(N16, N16, N16, 0, N16, np, np.float64)
    th, rv, rhod, Cx, Cy, Cz = _fields16["f"]
    oi = set_mode(bench.make_opts_init(N16, N16, N16, SD16, 40., 1, 1, 44, workload, dt), mode)
    for k, v in kw.items():
        assert hasattr(oi, k), k
        setattr(oi, k, v)
    return Case(oi, th, rv, rhod, dict(Cx=Cx, Cy=Cy, Cz=Cz), real_t=real_t)


def production_path(case, mode, N, nonzero=True):
    def check(A, B, C):
        assert_mode_is(C.prt, mode)
        assert_mode_is(B.prt, mode)
        first_b, first_c = B.log[N], C.log[0]
        assert (first_b["ranked"], first_b["skip"]) == (first_c["ranked"], first_c["skip"])
        if mode != "strict" and nonzero:
            assert first_c["ranked"] > 0 and first_c["skip"] > 0, first_c
    return check


@pytest.mark.parametrize("workload,dt", [("stratocumulus", 1.), ("coal-stress", 0.02)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_restored_run_equals_the_uninterrupted_one(real_t, mode, workload, dt):
    """cond + coal + adve + sedi, N + M = 6 + 6.  coal-stress at dt = 0.02: droplets collide in every step and the bound skips pairs
    (tests/test_hip_coal_skip.py), so the collided counts compare what the generator's call counter decides"""
    case = box16(workload, mode, real_t, dt)
    A, _, _, _ = abc(case, 6, 6, after_snapshot=production_path(case, mode, 6))
    if workload == "coal-stress":
        assert min(s["collided"] for s in A.log) >= 10


@pytest.mark.parametrize("N", [3, 4, 5])
@pytest.mark.parametrize("mode", ["fast_lean", "api_default"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_snapshot_before_on_and_after_a_reordering(real_t, mode, N):
    """reorder_every = 4: the storage is re-ordered at the end of the fourth step -- the snapshot falls on the step before, of and after"""
    case = box16("coal-stress", mode, real_t, 0.02, reorder_every=4)
    abc(case, N, 12 - N, after_snapshot=production_path(case, mode, N, nonzero=True))


# ---------------------------------------------------------------------------------- 2: dead slots in storage
@pytest.mark.parametrize("mode", ["fast_lean", "strict"])
def test_dead_slots_in_storage_are_kept(mode):
    """coal-stress at dt = 1 s, N = 6: the drizzle drops fall some 0.1 - 0.3 m a step and a few tens of them leave through the bottom of
    the 640 m box in every step; their slots stay in storage (compaction waits for 1 / 32 of it), so the storage extent exceeds n_part"""
    case = box16("coal-stress", mode, np.float64, 1.)

    def dead_slots(B):
        n = B.prt.state_u64("raw_n")
        print("storage", len(n), "living", B.prt.n_part)
        assert len(n) > B.prt.n_part and int((n == 0).sum()) == len(n) - B.prt.n_part
    _, B, C, blob = abc(case, 6, 6, before_snapshot=dead_slots, skip_may_differ=True)
    assert "n_storage = %d" % B.log[5]["storage"] in lgrngn.snapshot_describe(blob)


# ---------------------------------------------------------------------------------- 3: one case per carried extra, small boxes
def small(dims, sd, real_t, mode, opts=None, extra=None, names=(), **kw):
    oi = set_mode(h.box_opts(*dims, sd, **kw), mode)
    th, rv, rhod, C = h.box_fields(oi)
    if callable(extra):
        extra = extra(th)
    return Case(oi, th, rv, rhod, C, opts=opts, extra=extra, real_t=real_t, names=names)


def o_(**kw):
    o = lgrngn.opts_t()
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def src_opts():
    return o_(src=True, src_dry_distros={(.61, 0.): (h.lgrngn_bimodal(), 8, 3)})


def rlx_case(real_t, mode):
    oi = set_mode(h.box_opts(4, 0, 4, 32, rlx_switch=True, rlx_bins=40, rlx_sd_per_bin=2, rlx_timescale=3., supstp_rlx=2), mode)
    oi.rlx_dry_distros = {.61: [lgrngn.lognormal([.02e-6, .075e-6], [1.4, 1.6], [3 * 60e6, 3 * 40e6]), [0, 1.], [0., 120.]]}
    oi.n_sd_max = 4 * 32 * 16
    th, rv, rhod, C = h.box_fields(oi)
    return Case(oi, th, rv, rhod, C, opts=o_(rlx=True), real_t=real_t)


def chem_case(real_t, mode):
    oi = set_mode(h.box_opts(4, 3, 5, 16, chem_switch=True, chem_rho=chem.CHEM_RHO), mode)
    th, rv, rhod, C = h.box_fields(oi)
    rng = np.random.default_rng(2)
    gases = [g * (1 + 0.05 * rng.random(th.shape)) for g in chem.ICICLE_GAS]
    names = ["chem_" + nm for nm in chem.NAMES] + ["chem_V", "chem_flag"]
    return Case(oi, th, rv, rhod, C, opts=o_(chem_dsl=True, chem_dsc=True, chem_rct=True), gases=gases, real_t=real_t, names=names)


def parcel_case(real_t, mode):
    oi = set_mode(h.box_opts(0, 0, 0, 256, sedi_switch=False), mode)
    oi.dx = oi.dy = oi.dz = 1.
    oi.x1 = oi.y1 = oi.z1 = 1.
    return Case(oi, np.array([300.]), np.array([.0225]), np.array([1.1]), opts=o_(sedi=False, adve=False), real_t=real_t)


def diss(th):
    return dict(diss_rate=1e-3 * (1 + np.indices(th.shape)[-1]) * np.ones(th.shape))


# name: (case maker(real_t, mode), N, M)
EXTRAS = {
    "sstp_cond_4_per_cell": (lambda r, m: small((4, 0, 4), 32, r, m, sstp_cond=4), 3, 3),
    "exact_sstp_cond_adaptive": (lambda r, m: small((4, 0, 4), 32, r, m, names=("sstp_tmp_rv", "sstp_tmp_th", "sstp_tmp_rh", "rc2"), exact_sstp_cond=True, sstp_cond=4,
                                                    sstp_cond_act=8, sstp_cond_mix=False, adaptive_sstp_cond=True), 3, 3),
    "turbulence_with_onishi": (lambda r, m: small((4, 3, 5), 16, r, m, opts=o_(turb_adve=True, turb_cond=True, turb_coal=True), extra=diss, names=("up", "vp", "wp", "ssp", "dot_ssp"),
                                                  turb_adve_switch=True, turb_cond_switch=True, turb_coal_switch=True, kernel=lgrngn.kernel_t.onishi_hall,
                                                  kernel_parameters=np.array([66.]), SGS_mix_len=np.linspace(20., 40., 5)), 3, 3),
    "diag_incloud_time": (lambda r, m: small((4, 0, 4), 32, r, m, names=("incloud_time",), diag_incloud_time=True), 3, 3),
    "variable_dt": (lambda r, m: small((4, 0, 4), 32, r, m, opts=o_(dt=0.5), variable_dt_switch=True, sstp_cond=3, sstp_coal=2), 3, 3),
    "pred_corr": (lambda r, m: small((4, 4, 4), 16, r, m, adve_scheme=lgrngn.as_t.pred_corr), 3, 3),
    "simple_source_supstp_3": (lambda r, m: small((4, 4, 4), 16, r, m, opts=src_opts(), src_type=lgrngn.src_t.simple, src_x0=40., src_x1=120., src_y0=40., src_y1=120.,
                                                  src_z0=40., src_z1=120., n_sd_max=4 * 16 * 64), 4, 4),
    "relaxation_supstp_2": (rlx_case, 3, 3),
    "chemistry": (chem_case, 3, 3),
    "parcel_0d": (parcel_case, 3, 3),
}


@pytest.mark.parametrize("mode", ["strict", "api_default"])
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
@pytest.mark.parametrize("name", list(EXTRAS))
def test_carried_extras(name, real_t, mode):
    make, N, M = EXTRAS[name]
    case = make(real_t, mode)
    A, B, C, blob = abc(case, N, M)
    assert_mode_is(C.prt, mode)
    text = lgrngn.snapshot_describe(blob)
    if name == "simple_source_supstp_3":        # (fires in steps 0, 3, 6: the counter must survive, or C fires in its steps 0 and 3 = 4 and 7)
        grew = [i for i in range(1, 8) if A.log[i]["storage"] > A.log[i - 1]["storage"]]
        assert grew == [3, 6], (grew, A.log)
    if name == "relaxation_supstp_2":           # (fires in steps 0, 2, 4)
        assert A.log[4]["storage"] > A.log[3]["storage"], A.log
    if name == "chemistry":
        for nm in ["ambient." + g for g in chem.NAMES[:6]] + ["sd.chem_" + s for s in chem.NAMES]:
            assert "section %s:" % nm in text, nm
        assert np.any(case.state(C)["sd.chem_S_VI"] > 0)
    for nm in case.names:
        if not nm.startswith("chem_"):
            assert "section sd.%s:" % nm in text, nm


# ---------------------------------------------------------------------------------- 4: right after init()
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("real_t", REALS, ids=REAL_IDS)
def test_snapshot_right_after_init(real_t, mode):
    case = small((4, 4, 4), 32, real_t, mode)
    A = case.fresh(); case.init(A)
    C = case.restored(A.prt.snapshot(), case.callers_fields(A))
    assert_same_state(case.state(A), case.state(C))
    abc(small((4, 4, 4), 32, real_t, mode), 0, 4)


# ---------------------------------------------------------------------------------- 5: the device's checksum
@pytest.mark.parametrize("n", fmt.LENGTHS + [16, 4096 * 16 + 8, 3 * 2048 * 256 * 16 + 24])
def test_device_checksum_is_the_host_checksum(n):
    """the lengths of the host test, and lengths that leave a tail of 0, 8 and 24 - 16 bytes behind the 16-byte loads, the last one long
    enough for every workgroup of the capped grid to stride more than once"""
    import ctypes as C_
    lib = fmt._lib.load()
    a = fmt.seeded(n)
    out = C_.c_ulonglong()
    assert lib.lcx_snapshot_checksum_probe(C_.c_void_p(a.ctypes.data if a.size else None), C_.c_size_t(a.size), C_.byref(out)) == 0
    assert out.value == fmt.checksum_numpy(a) == fmt.checksum_host(lib, a)


# ---------------------------------------------------------------------------------- 6: refusals
def raises(text, fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    assert str(e.value).startswith("libcloudph++") and text in str(e.value), str(e.value)


def test_refusals(monkeypatch):
    case = small((4, 4, 4), 16, np.float64, "strict")
    B = case.fresh()
    raises("has not been initialised", B.prt.snapshot)
    case.init(B)
    case.step(B, 2)
    B.prt.step_sync(case.opts, B.th, B.rv, case.rhod, **case.C)
    raises("not between step_sync() and step_async()", B.prt.snapshot)
    B.prt.step_async(case.opts)
    B.prt.rng_replay_push(0, np.zeros(8))
    raises("replay queue is not empty", B.prt.snapshot)
    # (a fresh object of the same run for the blob: B's queue stays)
    B = case.fresh(); case.init(B); case.step(B, 3)
    held = case.callers_fields(B)
    blob = B.prt.snapshot()
    raises("init() may be called just once", lambda: B.prt.restore(blob))
    # another nx, another real kind, another arithmetic: the first field that differs is named
    raises("opts_init.nx (4 in the snapshot, 5 here)", lambda: small((5, 4, 4), 16, np.float64, "strict").fresh().prt.restore(blob))
    raises("real_kind (8 in the snapshot, 4 here)", lambda: small((4, 4, 4), 16, np.float32, "strict").fresh().prt.restore(blob))
    other = small((4, 4, 4), 16, np.float64, "strict")
    other.oi.strict_fp = False
    raises("opts_init.strict_fp (1 in the snapshot, 0 here)", lambda: other.fresh().prt.restore(blob))
    # damage: one payload byte flipped (the section is named), a truncated blob, a flipped head byte -- and the SAME object then takes the good blob
    text = lgrngn.snapshot_describe(blob)
    line = [ln for ln in text.splitlines() if ln.startswith("section rw2:")][0]
    at = int(line.split(" at ")[1].split(",")[0])
    bad = blob.copy()
    bad[at + 11] ^= 0x10
    C = case.fresh()
    raises("section 'rw2': checksum does not match", lambda: C.prt.restore(bad))
    raises("truncated", lambda: C.prt.restore(blob[:len(blob) - 64]))
    raises("truncated", lambda: C.prt.restore(blob[:100]))
    head = blob.copy()
    head[260] ^= 1
    raises("header checksum does not match", lambda: C.prt.restore(head))
    raises("wrong magic", lambda: C.prt.restore(np.zeros(4096, dtype=np.uint8)))
    C.prt.restore(bytearray(blob.tobytes()))                # (any object with the buffer protocol)
    C.th, C.rv = held["th"].copy(), held["rv"].copy()
    case.step(B, 3)
    case.step(C, 3)
    assert_same_state(case.state(B), case.state(C))
    # a decomposed domain: the multi-device object, a slab with a neighbour on its right, the SPMD front end
    text = "libcloudph++: snapshot of a decomposed domain is not built"
    monkeypatch.setenv("LCX_MULTI_DEVICE_MAP", "0,0")
    m = small((4, 4, 4), 16, np.float64, "strict")
    m.oi.dev_count = 2
    mul = lgrngn.factory(lgrngn.backend_t.multi_HIP, m.oi)
    assert mul.dev_count == 2
    raises(text, mul.snapshot)
    raises(text, lambda: mul.restore(blob))
    s = small((4, 4, 4), 16, np.float64, "strict")
    s.oi.bcond_rgt = multi.BCOND_DISTMEM
    slab = s.fresh()
    raises(text, lambda: slab.prt.restore(blob))
    raises(text, slab.prt.snapshot)
    assert multi.particles_multi_t.snapshot is not lgrngn.particles_t.snapshot


# ---------------------------------------------------------------------------------- 7: what a real blob says about itself
def test_describe_names_the_sections_that_the_options_imply():
    case = small((4, 3, 5), 16, np.float64, "api_default", names=("incloud_time",), diag_incloud_time=True)
    B = case.fresh(); case.init(B); case.step(B, 2)
    blob = B.prt.snapshot()
    text = lgrngn.snapshot_describe(blob)
    storage, n_cell = len(B.prt.state_u64("raw_n")), B.prt.n_cell
    assert "real kind 8" in text and "n_cell = %d" % n_cell in text and "n_part = %d" % B.prt.n_part in text
    for nm, bits in (("n", "uint64"), ("rd3", "real64"), ("rw2", "real64"), ("kappa", "real64"), ("vt", "real64"), ("x", "real64"), ("y", "real64"), ("z", "real64"),
                     ("sd.incloud_time", "real64"), ("ijk", "uint32"), ("rank", "uint32"), ("sorted_id", "uint32"), ("sorted_ijk", "uint32")):
        assert "section %s: %s x %d at" % (nm, bits, storage) in text, nm
    for nm in ("cell.th", "cell.rv", "cell.rhod", "cell.p", "cell.T", "cell.RH", "cell.eta", "cell.dv", "cell.sstp_tmp_rv"):
        assert "section %s: real64 x %d at" % (nm, n_cell) in text, nm
    assert "section cell_start: uint32 x %d at" % (n_cell + 1) in text
    assert "section courant_x: real64 x %d at" % (5 * 3 * 5) in text
    for absent in ("sd.up", "ambient.SO2", "cell.diss_rate", "sd.chem_H"):
        assert "section %s:" % absent not in text, absent
    two_d = small((4, 0, 4), 16, np.float32, "strict")
    Q = two_d.fresh(); two_d.init(Q)
    t2 = lgrngn.snapshot_describe(Q.prt.snapshot())
    assert "real kind 4" in t2 and "section y:" not in t2 and "section rw2: real32 x %d at" % len(Q.prt.state_u64("raw_n")) in t2
