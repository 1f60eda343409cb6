"""Shared test plumbing.

* oracle_particles(opts_init): the CPU oracle (oracle/liblcx_oracle.so, test infrastructure) driven
  through the SAME ctypes mirror as the product (libcloudphxx_amd.lgrngn.particles_t), prefix orc_.
* hip_particles(opts_init): the product (HIP library through the C ABI).
* small numpy restatements of the helpers the reference's python tests take from its `common` module.
"""
import ctypes
import os
import subprocess

import numpy as np

from libcloudphxx_amd import lgrngn

# The tests were written against the PARITY mode -- IEEE operation order, the reference's TOMS748 iterates, its ordered per-cell
# sums: opts_init.strict_fp = 1, the API default of rounds 1-4 -- and they keep pinning it: every opts_init_t() made under the test
# suite (this module is imported by every test module and by the worker scripts) starts from strict_fp = True, cond_solver = 0, and a
# test that wants another arithmetic says so (strict_fp = False, cond_solver = 1: the ARITH parameter of the condensation tests).  The
# API default since round 5 -- fast arithmetic with the reference's iterates -- is tested as such by tests/test_abi.py and
# tests/test_hip_parity.py::test_the_api_default_mode_keeps_the_strict_bars (API_DEFAULTS below).
_opts_init_ctor = lgrngn.opts_init_t.__init__
API_DEFAULTS = {}


def _parity_mode_opts_init(self, *a, **k):
    _opts_init_ctor(self, *a, **k)
    if not API_DEFAULTS:
        API_DEFAULTS.update(strict_fp=self.strict_fp, cond_solver=self.cond_solver)
    self.strict_fp = True
    self.cond_solver = 0


lgrngn.opts_init_t.__init__ = _parity_mode_opts_init


def api_default_opts(oi):
    """puts the two arithmetic options of an opts_init_t back to what the mirror's constructor sets"""
    if not API_DEFAULTS:
        lgrngn.opts_init_t()
    oi.strict_fp, oi.cond_solver = API_DEFAULTS["strict_fp"], API_DEFAULTS["cond_solver"]
    return oi


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "liblcx_oracle.so")
_oracle = None


def oracle_lib():
    global _oracle
    if _oracle is None:
        srcs = [os.path.join(ORACLE_DIR, f) for f in ("lcx_oracle.c", "orc_physics.h", "orc_toms748.h", "orc_tables.h")]
        fm = os.path.join(ORACLE_DIR, "liblcx_oracle_fastmath.so")
        omp = os.path.join(ORACLE_DIR, "liblcx_oracle_omp.so")
        f32 = os.path.join(ORACLE_DIR, "liblcx_oracle_f32.so")
        if (not os.path.exists(ORACLE_SO)) or (not os.path.exists(fm)) or (not os.path.exists(omp)) or (not os.path.exists(f32)) or any(os.path.getmtime(s) > os.path.getmtime(ORACLE_SO) for s in srcs):
            subprocess.check_call(["make", "-C", ORACLE_DIR, "-s"])
        os.environ.setdefault("LCX_DATA_DIR", os.path.join(ROOT, "libcloudphxx_amd", "data"))
        _oracle = ctypes.CDLL(ORACLE_SO)
    return _oracle


def oracle_particles(opts_init):
    return lgrngn.particles_t(opts_init, np.float64, lib=oracle_lib(), prefix="orc_")


_oracle_fm = None


def oracle_fastmath_particles(opts_init):
    """the oracle source compiled with -O3 -ffast-math (how the reference's Release build is compiled);
    only for pinning against the reference's committed refdata"""
    global _oracle_fm
    if _oracle_fm is None:
        oracle_lib()
        _oracle_fm = ctypes.CDLL(os.path.join(ORACLE_DIR, "liblcx_oracle_fastmath.so"))
    return lgrngn.particles_t(opts_init, np.float64, lib=_oracle_fm, prefix="orc_")


_oracle_omp = None


def cpu_quota():
    """CPUs this process may use at once: the cgroup's CFS quota (cpu.max, or cpu.cfs_quota_us / cpu.cfs_period_us) if one is set, and
    never more than the affinity mask.  A GPU box that shows 256 hardware threads but grants 16 CPUs of run time is throttled, not
    sped up, by 128 OpenMP threads (measured: 1.2e7 super-droplets/s on 128 threads, 2.0e7 on 16)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(float(q) / float(per) + .5)))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, int(q / per + .5)))
        except (OSError, ValueError):
            pass
    return n


def oracle_omp_lib():
    """the strict oracle source with its elementwise loops spread over the host cores (-fopenmp); bench.py's CPU baseline"""
    global _oracle_omp
    if _oracle_omp is None:
        oracle_lib()
        _oracle_omp = ctypes.CDLL(os.path.join(ORACLE_DIR, "liblcx_oracle_omp.so"))
        _oracle_omp.orc_num_threads.restype = ctypes.c_int
        _oracle_omp.orc_set_num_threads(ctypes.c_int(min(cpu_quota(), int(_oracle_omp.orc_num_threads()))))
    return _oracle_omp


_oracle_f32 = None


def oracle_f32_lib():
    """the oracle's float flavour (oracle/Makefile: the same source with real = float)"""
    global _oracle_f32
    if _oracle_f32 is None:
        oracle_lib()
        _oracle_f32 = ctypes.CDLL(os.path.join(ORACLE_DIR, "liblcx_oracle_f32.so"))
    return _oracle_f32


def oracle_f32_particles(opts_init):
    return lgrngn.particles_t(opts_init, np.float32, lib=oracle_f32_lib(), prefix="orc_")


def oracle_omp_particles(opts_init):
    return lgrngn.particles_t(opts_init, np.float64, lib=oracle_omp_lib(), prefix="orc_")


def hip_particles(opts_init, real_t=np.float64):
    return lgrngn.factory(lgrngn.backend_t.HIP, opts_init, real_t)


def assert_mode(prt, strict_fp, cond_solver=None, kernel=None, no_dbg=()):
    """What the OBJECT runs, read back from it (lcx_get_state_u64 "raw_mode"), not what the test meant to set: arithmetic, solver, the
    kernel of its last condensation launch (lgrngn.cond_kernel names, one or several) and measurement switches that must be off.  Round 5's
    production-size replay ran the strict kernels for most of the round because the suite pins the parity mode and nothing looked."""
    sfp, solver, ck, flags = prt.mode()
    assert sfp == bool(strict_fp), ("strict_fp", sfp)
    if cond_solver is not None:
        assert solver == cond_solver, ("cond_solver", solver)
    if kernel is not None:
        names = (kernel,) if isinstance(kernel, str) else tuple(kernel)
        assert ck.name in names, ("condensation kernel", ck.name, names)
    for name in no_dbg:
        assert not flags & lgrngn.dbg[name], ("dbg_flags", flags)


def oracle_rng_preview(prt, calls):
    """calls: list of (kind, length); returns list of arrays = what the oracle's engine will generate next."""
    kinds = (ctypes.c_int * len(calls))(*[k for k, _ in calls])
    lens = (ctypes.c_size_t * len(calls))(*[n for _, n in calls])
    tot = sum(n for _, n in calls)
    out = np.empty(tot, dtype=np.float64)
    f = prt._lib.orc_rng_preview           # (the library the object was made by: serial, fast-math or OpenMP build)
    rc = f(prt._h, kinds, lens, ctypes.c_int(len(calls)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == 0
    res, o = [], 0
    for _, n in calls:
        res.append(out[o:o + n].copy())
        o += n
    return res


# ---- the reference's `common` python module (bindings/python/common.hpp), restated with numpy
c_pd = 1005.
M_d = 0.02897
M_v = 1e-3 + 17e-3
R_d = 8.3144621 / M_d
R_v = 8.3144621 / M_v
p_1000 = 1e5


def T_of(th, rhod):          # common::theta_dry::T, theta_dry.hpp:24-41
    return (th * (rhod * R_d / p_1000) ** (R_d / c_pd)) ** (c_pd / (c_pd - R_d))


def p_of(rhod, rv, T):       # common::theta_dry::p, theta_dry.hpp:43-55
    return rhod * (R_d + rv * R_v) * T


def th_dry2std(th, rv):      # theta_dry.hpp:101-113
    return th / (1 + rv * R_v / R_d) ** (R_d / c_pd)


def lognormal_fn(mean_r, stdev, n_tot):
    """the exact python expression the reference's tests use for n(ln r)"""
    from math import exp, log, sqrt, pi

    def f(lnr):
        return n_tot * exp(-pow((lnr - log(mean_r)), 2) / 2 / pow(log(stdev), 2)) / log(stdev) / sqrt(2 * pi)
    return f


# ------------------------------------------------------------------ parity bars after step_cond
def cond_bars(strict_fp):
    """(rtol of th, rtol of rv, bound on the MEDIAN relative difference of rw2) after one step_cond against the oracle.

    strict arithmetic (the API default) reproduces the reference's TOMS748 iterates: th 1e-8 and rv 1e-7 (SURVEY 8a asks 1e-7 of both;
    measured 1.2e-11 and 1.5e-10 on the stress box of test_cond_step, tools/strict_bar_probe.py), and rw2 identical for almost every
    droplet (median < 1e-10; the maximum is the root finder's tolerance, 1e-4, where an ulp moves a stopping decision).

    fast arithmetic (opts_init.strict_fp = 0, cond_solver = 0) solves the same backward-Euler equation on the same bracket to the same
    tolerance 2^-15 with its own solver and returns the ROOT.  The reference's answer is the MIDPOINT of TOMS748's last bracket, which
    lies up to 1.5e-5 (in rw2, relative) from the root it brackets, to one side for all droplets of a kind.  So every droplet still
    agrees to 1e-4, but the typical distance is the reference's own (1e-9 in a settled cloud, 1e-6 ... 1e-5 where fresh aerosol
    activates), and it adds up over the droplets of a cell: in th by (th's change in the step / th) x 3 x 1e-5.  On the production-size
    boxes (test_hip_configs.py: 2^25 droplets, C5) that is 4e-11 ... 1e-9, inside SURVEY 8a's 1e-7; in the small stress boxes of
    test_hip_parity.py, where a step of activation moves th by 0.8 K (3e-3 of it), it reaches 1.2e-7 in th and 1.2e-6 in rv: held to
    3e-7 / 3e-6 there.  cond_solver = 1 (TOMS748 iterates in fast arithmetic: 1.2e-11 / 1.4e-10 there) is held to the strict bars."""
    return (1e-8, 1e-7, 1e-10) if strict_fp else (3e-7, 3e-6, 3e-5)


# ------------------------------------------------------------------ oracle <-> HIP pairing helpers
def box_opts(nx=4, ny=4, nz=4, sd_conc=64, dx=40., **kw):
    """a small periodic 3-D (or 2-D if ny=0) box in the spirit of BASELINE config 3"""
    oi = lgrngn.opts_init_t()
    oi.nx, oi.ny, oi.nz = nx, ny, nz
    oi.dx = oi.dy = oi.dz = dx
    oi.x1, oi.y1, oi.z1 = max(nx, 1) * dx, max(ny, 1) * dx, max(nz, 1) * dx
    if ny == 0:
        oi.dy, oi.y1 = 1., 1.
    oi.dt = 1.
    oi.sd_conc = sd_conc
    oi.n_sd_max = int(sd_conc * max(nx, 1) * max(ny, 1) * max(nz, 1) * 1.2) + 16
    oi.dry_distros = {(.61, 0.): lgrngn_bimodal()}
    oi.kernel = lgrngn.kernel_t.geometric
    oi.terminal_velocity = lgrngn.vt_t.beard77fast
    oi.adve_scheme = lgrngn.as_t.euler
    for k, v in kw.items():
        assert hasattr(oi, k), k
        setattr(oi, k, v)
    return oi


def lgrngn_bimodal():
    """icicle's bimodal lognormal aerosol (models/kinematic_2D/src/opts_common.hpp:56-62) as a python callable,
    so that oracle and HIP evaluate the very same host function"""
    f1 = lognormal_fn(.02e-6, 1.4, 60e6)
    f2 = lognormal_fn(.075e-6, 1.6, 40e6)
    return lambda lnr: f1(lnr) + f2(lnr)


def box_fields(oi, seed=0, supersat=True):
    """th, rv, rhod, Cx, Cy, Cz for a box: smooth, non-uniform, |C| <= 0.3.  Supersaturated throughout: the object's own RH reads
    1.23 .. 1.64 on box_opts(4, 4, 6, 64), with supersat=True and with False (th 289 K at rhod 1.1 is T = 278 K, where 8 g/kg is 1.2
    times saturation).  The fields stay as they are -- every measured bar of the parity tests rests on them; a box with RH < 1 (0.80 ..
    1.03 by level, crafted from the target RH) is tests/test_oracle_cond.py crafted_fields."""
    nx, ny, nz = max(oi.nx, 1), max(oi.ny, 1), max(oi.nz, 1)
    shp = tuple(n for n, f in zip((oi.nx, oi.ny, oi.nz), (1, 1, 1)) if n > 0)
    rng = np.random.default_rng(seed)
    ii = np.indices(shp if shp else (1,)).astype(float)
    th = 289. + 0.3 * rng.random(shp if shp else (1,))
    rhod = 1.1 - 0.01 * (ii[-1] / max(1, shp[-1] if shp else 1))
    rv = 8.0e-3 + (2.2e-3 if supersat else 0.) * (ii[-1] / max(1, shp[-1] if shp else 1)) + 1e-4 * rng.random(shp if shp else (1,))
    C = {}
    if oi.nx:
        if oi.ny:
            C["Cx"] = 0.3 * np.sin(2 * np.pi * np.indices((nx + 1, ny, nz))[1] / ny) + 0.05
            C["Cy"] = 0.2 * np.cos(2 * np.pi * np.indices((nx, ny + 1, nz))[0] / nx)
            C["Cz"] = 0.1 * np.sin(2 * np.pi * np.indices((nx, ny, nz + 1))[0] / nx) * np.sin(np.pi * np.indices((nx, ny, nz + 1))[2] / nz)
        elif oi.nz:
            C["Cx"] = 0.3 * np.sin(np.pi * (np.indices((nx + 1, nz))[1] + 0.5) / nz) + 0.05
            C["Cz"] = 0.1 * np.sin(2 * np.pi * np.indices((nx, nz + 1))[0] / nx) * np.sin(np.pi * np.indices((nx, nz + 1))[1] / nz)
        else:
            C["Cx"] = 0.3 * np.ones((nx + 1,))
    return (np.ascontiguousarray(th), np.ascontiguousarray(rv), np.ascontiguousarray(rhod),
            {k: np.ascontiguousarray(v) for k, v in C.items()})


def init_replay_calls(oi):
    """random arrays consumed by init() for a single-distro sd_conc run"""
    n_new = int(oi.sd_conc) * max(oi.nx, 1) * max(oi.ny, 1) * max(oi.nz, 1)
    ndim = sum(1 for n in (oi.nx, oi.ny, oi.nz) if n > 0)
    return [(0, n_new)] * (1 + ndim)


def make_pair(oi, fields, force_state=True, make_oracle=None, real_t=np.float64):
    """oracle and HIP objects initialised from the same inputs and the same (oracle) random stream
    (make_oracle: another build of the oracle, e.g. oracle_omp_particles for the large cases)"""
    th, rv, rhod, C = fields
    orc = (make_oracle or oracle_particles)(oi)
    hip = hip_particles(oi, real_t)
    for arr in oracle_rng_preview(orc, init_replay_calls(oi)):
        hip.rng_replay_push(0, arr)
    orc.init(th.copy(), rv.copy(), rhod.copy(), **C)
    hip.init(th.copy(), rv.copy(), rhod.copy(), **C)
    if force_state:
        copy_state(orc, hip)
    return orc, hip


def copy_state(orc, hip):
    """overwrite the device particle state with the oracle's (so later stages start bit-identical)"""
    g = lambda nm: orc.state_real(nm)
    oi = orc.opts_init
    hip.set_particles(orc.state_u64("n"), g("rd3"), g("rw2"), g("kappa"), g("vt"),
                      g("x") if oi.nx else None, g("y") if oi.ny else None, g("z") if oi.nz else None)


def push_coal_replay(orc, hip, sstp_coal=1):
    n = orc.n_part
    calls = [(1, n), (0, n)] * sstp_coal
    for (kind, _), arr in zip(calls, oracle_rng_preview(orc, calls)):
        hip.rng_replay_push(kind, arr)


# ------------------------------------------------------------------ in-process ring of slabs (drives the migration primitives)
class LocalRing:
    """N slabs of one periodic domain held by N particle objects in ONE process; migrants are moved with the same
    pack / unpack / finish primitives the multi-process wrapper (libcloudphxx_amd/multi.py) uses, without
    torch.distributed.  make(oi) -> particles object; alloc(nbytes) -> (keepalive, address)."""

    def __init__(self, oi_global, size, make, alloc):
        from libcloudphxx_amd import multi
        self.size, self.alloc, self.oi = size, alloc, oi_global
        self.prts, self.bfr, self.nxl = [], [], []
        for r in range(size):
            o, b = multi.distmem_opts(oi_global, r, size)
            o.n_x_bfr = 0
            o.n_x_tot = o.nx
            o.rng_seed = oi_global.rng_seed + r
            self.prts.append(make(o))
            self.bfr.append(b)
            self.nxl.append(o.nx)

    def slab(self, arr, r, ext=0):
        return np.ascontiguousarray(arr[self.bfr[r]:self.bfr[r] + self.nxl[r] + ext])

    def init(self, th, rv, rhod, Cx=None, Cy=None, Cz=None):
        for r, p in enumerate(self.prts):
            kw = {}
            if Cx is not None: kw["Cx"] = self.slab(Cx, r, 1)
            if Cy is not None: kw["Cy"] = self.slab(Cy, r)
            if Cz is not None: kw["Cz"] = self.slab(Cz, r)
            p.init(self.slab(th, r), self.slab(rv, r), self.slab(rhod, r), **kw)

    def step(self, opts, th, rv, rhod, Cx=None, Cy=None, Cz=None):
        self.step_sync(opts, th, rv, rhod, Cx, Cy, Cz)
        self.step_async(opts)

    def step_sync(self, opts, th, rv, rhod, Cx=None, Cy=None, Cz=None):
        for r, p in enumerate(self.prts):
            a = [self.slab(th, r), self.slab(rv, r), self.slab(rhod, r),
                 None if Cx is None else self.slab(Cx, r, 1), None if Cy is None else self.slab(Cy, r), None if Cz is None else self.slab(Cz, r)]
            p.step_sync(opts, *a)
            th[self.bfr[r]:self.bfr[r] + self.nxl[r]] = a[0]
            rv[self.bfr[r]:self.bfr[r] + self.nxl[r]] = a[1]
        n = self.size
        # Courant halo of pred_corr (multi.py _exchange_courant_halo): pack on every slab, then unpack
        isz = 8
        for which in (0, 1, 2):
            cnt = self.prts[0].courant_halo_count(which)
            if not cnt:
                continue
            bufs = []
            for p in self.prts:
                kl, pl = self.alloc(cnt * isz)
                kr, pr_ = self.alloc(cnt * isz)
                p.courant_halo_pack(which, 0, pl)
                p.courant_halo_pack(which, 1, pr_)
                bufs.append((pl, kl, pr_, kr))
            for r, p in enumerate(self.prts):
                p.courant_halo_unpack(which, 0, bufs[(r - 1) % n][2])     # left halo <- left neighbour's right-edge planes
                p.courant_halo_unpack(which, 1, bufs[(r + 1) % n][0])     # right halo <- right neighbour's left-edge planes

    def step_async(self, opts):
        n = self.size
        for p in self.prts:
            p.step_async(opts)
        packs = []
        open_walls = bool(self.oi.open_side_walls)           # no neighbour beyond the ends: what leaves there is gone (bcnd.ipp:160-205)
        for r, p in enumerate(self.prts):
            nl, nr = p.migrate_counts()
            rec = p.migrate_record_bytes()
            lft, rgt = (r - 1) % n, (r + 1) % n
            if open_walls and r == 0: nl = 0
            if open_walls and r == n - 1: nr = 0
            lft_x1 = self.prts[lft].opts_init.x1
            rgt_x0 = self.prts[rgt].opts_init.x0
            kl, pl = self.alloc(max(nl * rec, 8))
            kr, pr_ = self.alloc(max(nr * rec, 8))
            if nl: p.migrate_pack(0, lft_x1, pl, nl * rec)
            if nr: p.migrate_pack(1, rgt_x0, pr_, nr * rec)
            packs.append((nl, pl, kl, nr, pr_, kr))
        for r, p in enumerate(self.prts):
            lft, rgt = (r - 1) % n, (r + 1) % n
            n_from_l, p_from_l = packs[lft][3], packs[lft][4]      # left neighbour's right-going
            n_from_r, p_from_r = packs[rgt][0], packs[rgt][1]      # right neighbour's left-going
            if open_walls and r == 0: n_from_l = 0
            if open_walls and r == n - 1: n_from_r = 0
            if n_from_l: p.migrate_unpack(p_from_l, n_from_l)
            if n_from_r: p.migrate_unpack(p_from_r, n_from_r)
        for p in self.prts:
            p.migrate_finish(opts)

    def gather(self, fn):
        return np.concatenate([fn(p) for p in self.prts])


def host_alloc(nbytes):
    a = np.zeros(nbytes, dtype=np.uint8)
    return a, a.ctypes.data


def dev_alloc(nbytes):
    import torch
    t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    # the fill runs on torch's stream, the library packs into the buffer on its own (non-blocking) stream: without this
    # synchronisation the zero fill can land AFTER the packed records and wipe them (seen as lost super-droplets, rarely)
    torch.cuda.synchronize()
    return t, t.data_ptr()
